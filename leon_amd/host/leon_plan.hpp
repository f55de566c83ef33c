// leon_plan.hpp -- the arithmetic of `-d` that needs no device: how long a record's text is, a round's share of the letter tables, and
// the checks a container's metadata must pass before anything is sized from it.  Depends on <vector>, Exception and the layout
// constants only and calls no entry point of the library, so a CPU program can include it and link against nothing
// (tests/host_plan_check.cpp does).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "leon_container.hpp"
#include "leon_host.hpp"

namespace leon_host {
namespace plan {

// n + 1 offsets from n sizes, first[0], first[stride], ...
inline std::vector<uint64_t> prefix_sums(const uint64_t* first, uint64_t n, uint64_t stride = 1) {
    std::vector<uint64_t> off(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + first[stride * i];
    return off;
}

// ---------------------------------------------------------------------------------------------- record lengths
// a sequence of len bases as text: its lines' bytes and newlines (wrap: the width the original wrapped at, 0 = one line)
inline uint64_t seq_text_len(uint64_t len, uint64_t wrap) { return wrap && len > wrap ? len + (len + wrap - 1) / wrap : len + 1; }
// what a record without a header carries in its place: its index in the file, in decimal
inline uint64_t index_text_len(uint64_t read_index) { return std::to_string(read_index).size(); }
// bytes a '+' line has after the '+': nothing (kind 0), its header again (1), or its own text (2)
inline uint64_t plus_extra_len(uint8_t kind, uint64_t hdr_len, uint64_t own_text_len) { return kind == 1 ? hdr_len : kind == 2 ? own_text_len : 0; }
// n records at once: hdr_total header bytes, seq_text bytes of sequence lines (seq_text_len summed), `bases` bases, every '+' line of
// one kind (0 or 1).  Per record: lead byte, header, newline, sequence lines; FASTQ: '+', [header], newline, qualities, newline.
inline uint64_t records_text_len(uint64_t n, uint64_t hdr_total, uint64_t seq_text, uint64_t bases, bool fastq, uint8_t plus_kind) {
    return 2 * n + hdr_total + seq_text + (fastq ? 3 * n + bases + (plus_kind == 1 ? hdr_total : 0) : 0);
}
// one record; plus_extra: plus_extra_len of its '+' line
inline uint64_t record_text_len(uint64_t hdr_len, uint64_t len, uint64_t wrap, bool fastq, uint64_t plus_extra) {
    return records_text_len(1, hdr_len, seq_text_len(len, wrap), len, fastq, 0) + plus_extra;
}

// ---------------------------------------------------------------------------------------------- letter tables, round by round
// The share of the letter tables that falls into the bases [b0, b1): runs clipped to the range, everything counted
// from b0.  The positions' bytes are the table's at [first_pos, first_pos + pos.size()).
struct LetterSlice {
    std::vector<uint64_t> runs, pos;              // begin, end pairs; positions
    size_t first_pos = 0;
};
inline LetterSlice clip_letters(const std::vector<uint64_t>& all_runs, const std::vector<uint64_t>& all_pos, uint64_t b0, uint64_t b1) {
    LetterSlice s;
    const uint64_t n_all = all_runs.size() / 2;
    uint64_t ra = 0, rb = n_all;                  // the first run that ends behind b0 .. the first that begins at or behind b1
    for (uint64_t hi = n_all; ra < hi;) { const uint64_t mid = ra + (hi - ra) / 2; if (all_runs[2 * mid + 1] > b0) hi = mid; else ra = mid + 1; }
    for (uint64_t lo = ra; lo < rb;) { const uint64_t mid = lo + (rb - lo) / 2; if (all_runs[2 * mid] >= b1) rb = mid; else lo = mid + 1; }
    for (uint64_t r = ra; r < rb; r++) { s.runs.push_back(std::max(all_runs[2 * r], b0) - b0); s.runs.push_back(std::min(all_runs[2 * r + 1], b1) - b0); }
    const size_t pa = std::lower_bound(all_pos.begin(), all_pos.end(), b0) - all_pos.begin(), pb = std::lower_bound(all_pos.begin(), all_pos.end(), b1) - all_pos.begin();
    s.pos.assign(all_pos.begin() + pa, all_pos.begin() + pb);
    for (uint64_t& p : s.pos) p -= b0;
    s.first_pos = pa;
    return s;
}

// ---------------------------------------------------------------------------------------------- validators
// `file`: the container's name, as the messages begin with it
struct Params {
    uint64_t k = 0, rpb = 0, n_reads = 0, n_anchors = 0, tai = 0, n_hash = 0, nbits = 0, total_bases = 0, n_blocks = 0;
    uint64_t rev = 1;                             // the container's own revision (layout::CONTAINER_REV): files of revision 1 have no such word
    uint64_t fasta_line_width = 0;
    uint8_t info = 0;
};
inline Params check_params(const std::string& file, const std::vector<uint8_t>& infov, const std::vector<uint64_t>& params) {
    using namespace layout;
    if (infov.size() != 1 || params.size() < PARAM_COUNT_REV1) throw Exception(file + ": metadata is not what this build writes");
    Params p;
    p.info = infov[0];
    p.k = params[P_KMER_SIZE]; p.rpb = params[P_READS_PER_BLOCK]; p.n_reads = params[P_N_READS]; p.n_anchors = params[P_N_ANCHORS];
    p.tai = params[P_BLOOM_TAI]; p.n_hash = params[P_BLOOM_N_HASH]; p.nbits = params[P_BLOOM_BLOCK_NBITS]; p.total_bases = params[P_TOTAL_BASES];
    p.fasta_line_width = params[P_FASTA_LINE_WIDTH];
    if (params[P_VERSION_MAJOR] != 1) throw Exception(file + " was written by an incompatible version");
    p.rev = params.size() > P_CONTAINER_REV ? params[P_CONTAINER_REV] : 1;
    if (p.rev < 1 || p.rev > CONTAINER_REV)
        throw Exception(file + " was written by a later build (container revision " + std::to_string(p.rev) + ", this build reads up to " + std::to_string(CONTAINER_REV) + ")");
    if (p.k < 3 || p.k > 63 || p.rpb == 0 || p.rpb > (1u << 30) || p.n_hash < 1 || p.n_hash > 10 || p.nbits < 4 || p.nbits > 16 || p.n_anchors > (1ull << 32) ||
        p.n_reads > (1ull << 40) || p.total_bases > (1ull << 46))
        throw Exception(file + ": implausible parameters in the metadata");
    p.n_blocks = (p.n_reads + p.rpb - 1) / p.rpb;
    return p;
}
// block tables (3 words per block), checked against the parameters' totals before anything is sized from them
inline void check_dna_table(const std::string& file, const std::vector<uint64_t>& tdna, const Params& p) {
    if (tdna.size() != 3 * p.n_blocks) throw Exception(file + ": the DNA block table does not match the read count");
    uint64_t sum_reads = 0, sum_bases = 0;
    for (uint64_t b = 0; b < p.n_blocks; b++) {
        if (tdna[3 * b + 1] > p.rpb || tdna[3 * b + 2] > p.total_bases - sum_bases) throw Exception(file + ": the DNA block table does not add up");
        sum_reads += tdna[3 * b + 1]; sum_bases += tdna[3 * b + 2];
    }
    if (sum_reads != p.n_reads || sum_bases != p.total_bases) throw Exception(file + ": the DNA block table does not add up");
}
inline void check_header_table(const std::string& file, std::vector<uint64_t>& thdr, const std::vector<uint64_t>& tdna, const Params& p) {
    // revision 1 before the text-bytes column existed: 2 words per block (payload bytes, reads).  Such a file decodes like any
    // other: its text buffers start from a guess (64 bytes per header) and the decoder asks for more where that falls short.
    if (p.rev == 1 && thdr.size() == 2 * p.n_blocks && p.n_blocks) {
        std::vector<uint64_t> t3(3 * p.n_blocks);
        for (uint64_t b = 0; b < p.n_blocks; b++) { t3[3 * b] = thdr[2 * b]; t3[3 * b + 1] = thdr[2 * b + 1]; t3[3 * b + 2] = 64 * std::min<uint64_t>(thdr[2 * b + 1], p.rpb); }
        thdr.swap(t3);
    }
    if (thdr.size() != 3 * p.n_blocks) throw Exception(file + ": the header block table does not match the read count");
    for (uint64_t b = 0; b < p.n_blocks; b++) {
        if (thdr[3 * b + 1] != tdna[3 * b + 1]) throw Exception(file + ": header and DNA blocks disagree");
        if (thdr[3 * b + 2] > (1ull << 40)) throw Exception(file + ": the header block table does not add up");      // (buffers are sized from it)
    }
}
inline void check_qual_table(const std::string& file, const std::vector<uint64_t>& tqual, const std::vector<uint64_t>& tdna, const Params& p) {
    if (tqual.size() != 3 * p.n_blocks) throw Exception(file + ": the quality block table does not match the read count");
    for (uint64_t b = 0; b < p.n_blocks; b++)
        if (tqual[3 * b + 1] != tdna[3 * b + 1] || tqual[3 * b + 2] != tdna[3 * b + 2]) throw Exception(file + ": quality and DNA blocks disagree");
}
inline void check_checksum_table(const std::string& file, const std::vector<uint64_t>& tsum, uint64_t n_blocks) {
    using namespace layout;
    if (tsum.empty()) throw Exception(file + ": the checksum table does not match the read count");
    if (tsum[0] != CHECKSUM_CRC32) throw Exception(file + ": unknown checksum kind " + std::to_string(tsum[0]) + " in " + DS_CHECKSUMS + " (this build knows 1 = CRC-32)");
    if (tsum.size() != 1 + 3 * n_blocks) throw Exception(file + ": the checksum table does not match the read count");
}
// `-c -dict-pieces`: the piece table against the parameters and the bytes of leon/anchors/dict_pieces.  has_single / has_pieces / has_table:
// which of leon/anchors/dict, dict_pieces and dict_piece_table the file holds.  Returns false for a file of the single-stream form (the
// table is then not looked at), true for a checked pieced one; the piece sizes are table[2 ...].
inline bool check_dict_pieces(const std::string& file, bool has_single, bool has_pieces, bool has_table, const std::vector<uint64_t>& table,
                              uint64_t piece_bytes, uint64_t n_anchors) {
    using namespace layout;
    auto refuse = [&](const std::string& what) { return Exception(file + ": dictionary pieces: " + what); };
    if (!has_pieces && !has_table) return false;
    if (has_pieces != has_table) throw refuse(std::string(has_pieces ? DS_ANCHOR_DICT_PIECE_TABLE : DS_ANCHOR_DICT_PIECES) + " is missing");
    if (has_single) throw refuse(std::string("the file holds ") + DS_ANCHOR_DICT + " as well");
    if (table.size() < 2) throw refuse("the piece table is too short");
    if (table[0] != DICT_PIECES_ORDER0) throw refuse("unknown kind " + std::to_string(table[0]) + " in " + DS_ANCHOR_DICT_PIECE_TABLE + " (this build knows 1)");
    const uint64_t P = table[1];
    if (P < 1 || P > DICT_PIECE_ANCHORS_MAX) throw refuse(std::to_string(P) + " anchors per piece (1 .. 1048576)");
    const uint64_t n_pieces = (n_anchors + P - 1) / P;
    if (table.size() - 2 != n_pieces)
        throw refuse("the table holds " + std::to_string(table.size() - 2) + " pieces, " + std::to_string(n_anchors) + " anchors in pieces of " + std::to_string(P) + " make " + std::to_string(n_pieces));
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n_pieces; i++) {
        const uint64_t sz = table[2 + i];
        if (sz < 8) throw refuse("piece " + std::to_string(i) + " has " + std::to_string(sz) + " bytes (a piece ends with 8 flush bytes)");
        if (sz > piece_bytes - sum) throw refuse("the piece sizes add up to more than the " + std::to_string(piece_bytes) + " bytes of " + DS_ANCHOR_DICT_PIECES);
        sum += sz;
    }
    if (sum != piece_bytes) throw refuse("the piece sizes add up to " + std::to_string(sum) + ", " + DS_ANCHOR_DICT_PIECES + " holds " + std::to_string(piece_bytes) + " bytes");
    return true;
}
inline Exception letters_error(const char* ds, const std::string& what) { return Exception(std::string("letters: ") + ds + " " + what); }
// the runs as stored (the kind word first); on return the kind word is taken off
inline void check_letter_runs(std::vector<uint64_t>& runs, uint64_t total_bases) {
    using namespace layout;
    if (runs.empty()) throw letters_error(DS_LETTER_RUNS, "is empty");
    if (runs[0] != LETTERS_RUNS_AND_BYTES) throw letters_error(DS_LETTER_RUNS, "is of unknown kind " + std::to_string(runs[0]) + " (this build knows 1)");
    if (runs.size() % 2 != 1) throw letters_error(DS_LETTER_RUNS, "does not hold pairs");
    runs.erase(runs.begin());
    for (size_t r = 0; r < runs.size(); r += 2) {
        if (runs[r] >= runs[r + 1]) throw letters_error(DS_LETTER_RUNS, "run " + std::to_string(r / 2) + " is empty or runs backwards");
        if (runs[r + 1] > total_bases) throw letters_error(DS_LETTER_RUNS, "run " + std::to_string(r / 2) + " ends behind the file's " + std::to_string(total_bases) + " bases");
        if (r && runs[r - 1] > runs[r]) throw letters_error(DS_LETTER_RUNS, "run " + std::to_string(r / 2) + " overlaps the run before it");
    }
}
inline void check_letter_bytes(const std::vector<uint64_t>& pos, const std::vector<uint8_t>& bytes, uint64_t total_bases) {
    using namespace layout;
    if (pos.size() != bytes.size()) throw letters_error(DS_LETTER_ODD_BYTES, "holds " + std::to_string(bytes.size()) + " bytes for " + std::to_string(pos.size()) + " positions");
    for (size_t i = 0; i < pos.size(); i++) {
        if (pos[i] >= total_bases) throw letters_error(DS_LETTER_ODD_POS, "position " + std::to_string(i) + " lies behind the file's " + std::to_string(total_bases) + " bases");
        if (i && pos[i - 1] >= pos[i]) throw letters_error(DS_LETTER_ODD_POS, "position " + std::to_string(i) + " is not behind the one before it");
    }
}

}  // namespace plan
}  // namespace leon_host
