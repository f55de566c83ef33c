// host_dict_pieces.h -- the anchor dictionary as independently coded PIECES, on host threads.  Compiles without HIP.
// Anchors in address order are cut into pieces of P anchors (the last one holds the rest); piece p is exactly what AnchorDictCoder
// writes for its slice: a fresh 5-symbol model, a fresh coder, the 8 flush bytes.  The stream is the pieces back to back; piece_off
// (n_pieces + 1 entries) says where each begins.  These functions are the VERDICT for the device calls of dict_kernels.hip: the same
// arguments are refused with the same code and the same words (dict_pieces_*_refusal, shared by both).
#pragma once
#include "host_rc.h"

#include <atomic>
#include <string>

namespace leon {

constexpr uint32_t kDictPieceAnchorsDefault = 1024;
constexpr uint32_t kDictPieceAnchorsMax = 1u << 20;           // every total 5 + t of a piece stays below 5 + 63 * 2^20 < 2^26 (RC_MAX_TOTAL is 2^30)
constexpr int kDictPiecesInvalid = -1, kDictPiecesOverflow = -5;   // LEON_E_INVALID, LEON_E_OVERFLOW (this header does not see leon_dna.h)

inline uint32_t dict_piece_anchors(uint32_t piece_anchors) { return piece_anchors ? piece_anchors : kDictPieceAnchorsDefault; }
inline uint64_t dict_piece_count(uint64_t n_anchors, uint32_t P) { return (n_anchors + P - 1) / P; }

// what both encoders refuse before anything is touched; nullptr = the arguments are in order
inline const char* dict_pieces_encode_refusal(const uint64_t* kmers, uint64_t n_anchors, uint32_t k, uint32_t piece_anchors, const uint8_t* out,
                                              uint64_t out_cap, const uint64_t* piece_off, const uint64_t* size) {
    if ((!kmers && n_anchors) || (!out && out_cap) || !piece_off || !size) return "anchor dictionary pieces: null argument";
    if (k < 1 || k > 63) return "anchor dictionary pieces: kmer_size must be in 1..63";
    if (piece_anchors > kDictPieceAnchorsMax) return "anchor dictionary pieces: piece_anchors must be in 1..2^20 (0 = 1024)";
    if (n_anchors > (1ull << 40)) return "anchor dictionary pieces: more than 2^40 anchors";
    return nullptr;
}
// ... and both decoders, in this order
inline const char* dict_pieces_decode_refusal(const uint8_t* payload, const uint64_t* piece_off, uint64_t n_pieces, uint64_t n_anchors, uint32_t k,
                                              uint32_t piece_anchors, const uint64_t* out_kmers) {
    if (!piece_off || (!out_kmers && n_anchors)) return "anchor dictionary pieces: null argument";
    if (k < 1 || k > 63) return "anchor dictionary pieces: kmer_size must be in 1..63";
    if (piece_anchors > kDictPieceAnchorsMax) return "anchor dictionary pieces: piece_anchors must be in 1..2^20 (0 = 1024)";
    if (n_anchors > (1ull << 40)) return "anchor dictionary pieces: more than 2^40 anchors";
    if (n_pieces != dict_piece_count(n_anchors, dict_piece_anchors(piece_anchors))) return "piece table does not match the anchor count";
    for (uint64_t p = 0; p < n_pieces; p++)
        if (piece_off[p + 1] < piece_off[p]) return "piece offsets run backwards";
    if (!payload && piece_off[n_pieces] != 0) return "anchor dictionary pieces: null argument";
    return nullptr;
}
inline std::string dict_piece_refusal(uint64_t piece) { return "anchor dictionary piece " + std::to_string(piece) + " does not decode"; }

inline uint32_t dict_pieces_threads(uint32_t n_threads, uint64_t n_pieces) {
    uint32_t n = n_threads;
    if (!n) {
        cpu_set_t set;
        const int c = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
        n = c > 0 ? (uint32_t)c : 1u;
    }
    n = std::min<uint32_t>(n, 64);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, n_pieces));
}
// one piece per task: fn(p) for every p in [0, n_pieces), on n threads
template <typename Fn> inline void dict_pieces_run(uint32_t n_threads, uint64_t n_pieces, Fn fn) {
    const uint32_t n = dict_pieces_threads(n_threads, n_pieces);
    if (n <= 1) { for (uint64_t p = 0; p < n_pieces; p++) fn(p); return; }
    std::atomic<uint64_t> next{0};
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n; i++) th.emplace_back([&] { for (uint64_t p; (p = next.fetch_add(1)) < n_pieces;) fn(p); });
    for (auto& t : th) t.join();
}

// Returns 0, or a negative code with `why` set.  piece_off[0 .. n_pieces] is filled whenever the arguments are in order, *size = the
// stream's bytes; kDictPiecesOverflow when out_cap is smaller (nothing written to out).
inline int host_dict_encode_pieces(const uint64_t* kmers, uint64_t n_anchors, uint32_t k, uint32_t piece_anchors, uint8_t* out, uint64_t out_cap,
                                   uint64_t* piece_off, uint64_t* size, uint32_t n_threads, std::string& why) {
    if (const char* r = dict_pieces_encode_refusal(kmers, n_anchors, k, piece_anchors, out, out_cap, piece_off, size)) { why = r; return kDictPiecesInvalid; }
    const uint32_t P = dict_piece_anchors(piece_anchors), W = k >= 32 ? 2u : 1u;
    const uint64_t n_pieces = dict_piece_count(n_anchors, P);
    std::vector<std::vector<uint8_t>> piece(n_pieces);
    dict_pieces_run(n_threads, n_pieces, [&](uint64_t p) {
        const uint64_t a0 = p * P, na = std::min<uint64_t>(P, n_anchors - a0);
        AnchorDictCoder coder;
        coder.encode_kmers(kmers + a0 * W, na, k);
        coder.flush();
        piece[p].assign(coder.data(), coder.data() + coder.size());
    });
    piece_off[0] = 0;
    for (uint64_t p = 0; p < n_pieces; p++) piece_off[p + 1] = piece_off[p] + piece[p].size();
    *size = piece_off[n_pieces];
    if (*size > out_cap) { why = "anchor dictionary pieces: out_cap too small"; return kDictPiecesOverflow; }
    dict_pieces_run(n_threads, n_pieces, [&](uint64_t p) { if (!piece[p].empty()) memcpy(out + piece_off[p], piece[p].data(), piece[p].size()); });
    return 0;
}

// out_kmers (n_anchors * W words) is written only when every piece has decoded; else the SMALLEST failing piece is named
inline int host_dict_decode_pieces(const uint8_t* payload, const uint64_t* piece_off, uint64_t n_pieces, uint64_t n_anchors, uint32_t k,
                                   uint32_t piece_anchors, uint64_t* out_kmers, uint32_t n_threads, std::string& why) {
    if (const char* r = dict_pieces_decode_refusal(payload, piece_off, n_pieces, n_anchors, k, piece_anchors, out_kmers)) { why = r; return kDictPiecesInvalid; }
    const uint32_t P = dict_piece_anchors(piece_anchors), W = k >= 32 ? 2u : 1u;
    std::vector<uint64_t> tmp(n_anchors * W);
    std::atomic<uint64_t> bad{~0ull};
    dict_pieces_run(n_threads, n_pieces, [&](uint64_t p) {
        const uint64_t a0 = p * P, na = std::min<uint64_t>(P, n_anchors - a0);
        if (decode_anchor_dict(payload + piece_off[p], piece_off[p + 1] - piece_off[p], na, k, tmp.data() + a0 * W)) return;
        uint64_t cur = bad.load();
        while (p < cur && !bad.compare_exchange_weak(cur, p)) {}
    });
    if (bad.load() != ~0ull) { why = dict_piece_refusal(bad.load()); return kDictPiecesInvalid; }
    if (n_anchors) memcpy(out_kmers, tmp.data(), n_anchors * W * sizeof(uint64_t));
    return 0;
}

}  // namespace leon
