// dict_pieces_selftest.cpp -- leon_amd/csrc/host_dict_pieces.h as a program of its own (no HIP, no library): the piece encoder and decoder
// on host threads against AnchorDictCoder / decode_anchor_dict on every slice, the refusals with their words, and corrupted pieces.
// Built by tests/test_dict_pieces_cpu.py with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, and run as a child process.
#include "../leon_amd/csrc/host_dict_pieces.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace leon;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                           // splitmix64
    uint64_t z = (rnd_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<uint64_t> random_kmers(uint64_t n, uint32_t k) {
    const uint32_t W = k >= 32 ? 2u : 1u;
    std::vector<uint64_t> v(n * W);
    for (uint64_t a = 0; a < n; a++) {
        if (W == 1) v[a] = k == 32 ? rnd() : rnd() & ((1ull << (2 * k)) - 1);
        else { v[2 * a] = rnd(); v[2 * a + 1] = k == 32 ? 0 : rnd() & ((1ull << (2 * (k - 32))) - 1); }
    }
    return v;
}

static void round_trip(uint32_t k, uint32_t P, uint64_t n, uint32_t threads) {
    const uint32_t W = k >= 32 ? 2u : 1u, Pe = dict_piece_anchors(P);
    const std::vector<uint64_t> kmers = random_kmers(n, k);
    const uint64_t n_pieces = dict_piece_count(n, Pe);
    std::vector<uint64_t> off(n_pieces + 1, 77);
    uint64_t size = 0;
    std::string why;
    // the size first (nothing written), then the stream
    int rc = host_dict_encode_pieces(kmers.data(), n, k, P, nullptr, 0, off.data(), &size, threads, why);
    CHECK(n ? rc == kDictPiecesOverflow && why.find("out_cap too small") != std::string::npos : rc == 0);
    std::vector<uint8_t> out(size);                              // exactly the need: a byte past it is the sanitizer's to find
    rc = host_dict_encode_pieces(kmers.data(), n, k, P, out.data(), size, off.data(), &size, threads, why);
    CHECK(rc == 0 && off[0] == 0 && off[n_pieces] == size && size == out.size());
    for (uint64_t p = 0; p < n_pieces; p++) {
        const uint64_t a0 = p * Pe, na = std::min<uint64_t>(Pe, n - a0);
        AnchorDictCoder coder;
        coder.encode_kmers(kmers.data() + a0 * W, na, k);
        coder.flush();
        CHECK(off[p + 1] - off[p] == coder.size() && coder.size() >= 8);
        CHECK(!memcmp(out.data() + off[p], coder.data(), coder.size()));
    }
    std::vector<uint64_t> back(n * W, 0x5EED);
    rc = host_dict_decode_pieces(out.data(), off.data(), n_pieces, n, k, P, back.data(), threads, why);
    CHECK(rc == 0 && back == kmers);
    if (n_pieces >= 3) {
        // piece 1 cut to its first half: its offsets shrink, the bytes behind move up.  Whatever the verdict, nothing outside a piece is read
        std::vector<uint8_t> cut(out.begin(), out.begin() + off[1] + (off[2] - off[1]) / 2);
        cut.insert(cut.end(), out.begin() + off[2], out.end());
        std::vector<uint64_t> coff(off);
        for (uint64_t p = 2; p <= n_pieces; p++) coff[p] -= (off[2] - off[1]) - (off[2] - off[1]) / 2;
        std::vector<uint64_t> left(n * W, 0x5EED);
        rc = host_dict_decode_pieces(cut.data(), coff.data(), n_pieces, n, k, P, left.data(), threads, why);
        if (rc) { CHECK(rc == kDictPiecesInvalid && why == dict_piece_refusal(1)); for (uint64_t x : left) CHECK(x == 0x5EED); }
        // every piece empty: zeros stand in for the bytes, at most 16 of them past a piece's end
        std::vector<uint64_t> zoff(n_pieces + 1, 0);
        rc = host_dict_decode_pieces(out.data(), zoff.data(), n_pieces, n, k, P, left.data(), threads, why);
        if (rc) { CHECK(why == dict_piece_refusal(0)); for (uint64_t x : left) CHECK(x == 0x5EED); }
    }
}

int main() {
    const uint32_t ks[] = {3, 31, 32, 63}, Ps[] = {1, 3, 64, 1024};
    for (uint32_t k : ks)
        for (uint32_t P : Ps) {
            const uint64_t ns[] = {0, 1, (uint64_t)P - 1, P, (uint64_t)P + 1, 5ull * P + 2};
            for (uint64_t n : ns) round_trip(k, P, n, (uint32_t)(1 + (n + k) % 4));
        }
    round_trip(31, 0, 2 * 1024 + 5, 0);                           // the default piece size, all the CPUs
    // the refusals, in the decoder's order
    std::string why;
    uint64_t off[4] = {0, 8, 16, 24}, size = 0, km[8] = {};
    uint8_t bytes[32] = {};
    CHECK(host_dict_decode_pieces(bytes, nullptr, 3, 3, 31, 1, km, 1, why) == kDictPiecesInvalid && why.find("null argument") != std::string::npos);
    CHECK(host_dict_decode_pieces(bytes, off, 3, 3, 64, 1, km, 1, why) == kDictPiecesInvalid && why.find("kmer_size must be in 1..63") != std::string::npos);
    CHECK(host_dict_decode_pieces(bytes, off, 3, 3, 31, kDictPieceAnchorsMax + 1, km, 1, why) == kDictPiecesInvalid && why.find("piece_anchors must be in 1..2^20") != std::string::npos);
    CHECK(host_dict_decode_pieces(bytes, off, 3, 4, 31, 1, km, 1, why) == kDictPiecesInvalid && why == "piece table does not match the anchor count");
    CHECK(host_dict_decode_pieces(bytes, off, 2, 3, 31, 1, km, 1, why) == kDictPiecesInvalid && why == "piece table does not match the anchor count");
    uint64_t back[4] = {0, 16, 8, 24};
    CHECK(host_dict_decode_pieces(bytes, back, 3, 3, 31, 1, km, 1, why) == kDictPiecesInvalid && why == "piece offsets run backwards");
    CHECK(host_dict_encode_pieces(nullptr, 3, 31, 1, bytes, 32, off, &size, 1, why) == kDictPiecesInvalid && why.find("null argument") != std::string::npos);
    CHECK(host_dict_encode_pieces(km, 3, 0, 1, bytes, 32, off, &size, 1, why) == kDictPiecesInvalid && why.find("kmer_size must be in 1..63") != std::string::npos);
    printf("dict pieces selftest: ok\n");
    return 0;
}
