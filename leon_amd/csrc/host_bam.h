// host_bam.h -- unaligned BAM records in plain code (leon_host_records_bam, leon_bam_header: host_streams.cpp), and what that form shares
// with the device's (leon_records_bam_device, bam_kernels.hip): the record's shape, the base codes, the refusals' words.  DESIGN.md 4.19.
// Needs nothing but include/leon_dna.h; compiles with and without HIP.
//
// The uncompressed content of the file: "BAM\1", l_text, the text "@HD\tVN:1.6\tSO:unsorted\n", n_ref = 0; then one record per read,
// little-endian:
//     block_size (the bytes that follow)  refID -1  pos -1  l_read_name (with its NUL)  mapq 0  bin 4680  n_cigar_op 0  flag 4
//     l_seq  next_refID -1  next_pos -1  tlen 0                                  -- 4 + 32 bytes
//     the name and a NUL | (l_seq + 1) / 2 bytes of base codes, the first base in the high nybble | l_seq quality bytes
//     'C' 'O' 'Z' the comment and a NUL, when there is a comment
// The name is the header up to its first space or tab ("*" when that is empty, the decimal read index without a header stream), the
// comment what follows that one byte.  [RECALLED from the SAM/BAM specification; parity with htslib's reader is unpinned.]
#pragma once
#include "../../include/leon_dna.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#ifdef __HIPCC__
#define LEON_BAM_HD __host__ __device__
#else
#define LEON_BAM_HD
#endif

namespace leon {

constexpr uint32_t BAM_FIXED = 36;                              // block_size and the 32 bytes from refID to tlen
constexpr uint32_t BAM_MAX_NAME = 254;                          // l_read_name is a byte and counts the NUL
constexpr uint32_t BAM_BIN_UNMAPPED = 4680, BAM_FLAG_UNMAPPED = 4;
constexpr uint32_t BAM_MIN_RECORD = BAM_FIXED + 2;              // "*" and its NUL, no bases

// "=ACMGRSVTWYHKDBN", case folded; every other byte is N (15)
LEON_BAM_HD inline uint32_t bam_base_code(uint32_t c) {
    if (c >= 'a' && c <= 'z') c -= 32;
    const uint64_t lo = 0x565352474D43413Dull, hi = 0x4E42444B48595754ull;      // the table's bytes, codes 0..7 and 8..15
    uint32_t code = 15;
    for (uint32_t k = 0; k < 16; k++)
        if ((uint32_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFF) == c) code = k;
    return code;
}

// word w (0..8) of a record's first 36 bytes
LEON_BAM_HD inline uint32_t bam_fixed_word(uint32_t w, uint32_t block_size, uint32_t l_read_name, uint32_t l_seq) {
    switch (w) {
        case 0: return block_size;
        case 3: return l_read_name | (BAM_BIN_UNMAPPED << 16);    // l_read_name, mapq 0, bin
        case 4: return BAM_FLAG_UNMAPPED << 16;                  // n_cigar_op 0, flag
        case 5: return l_seq;
        case 8: return 0;                                        // tlen
        default: return 0xFFFFFFFFu;                             // refID, pos, next_refID, next_pos
    }
}

// a record's bytes: nl = the name's bytes as the header gives them (0: "*" is written), hl = the header's bytes (hl > nl: a separator
// and hl - nl - 1 bytes of comment behind it)
LEON_BAM_HD inline uint64_t bam_record_size(uint64_t nl, uint64_t hl, uint64_t len) {
    const uint64_t cl = hl > nl ? hl - nl - 1 : 0;
    return BAM_FIXED + (nl ? nl : 1) + 1 + (len + 1) / 2 + len + (cl ? 3 + cl + 1 : 0);
}

inline uint32_t bam_dec_digits(uint64_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; n++; } return n; }

inline std::string bam_header_bytes() {
    const std::string text = "@HD\tVN:1.6\tSO:unsorted\n";
    std::string h("BAM\1", 4);
    for (int b = 0; b < 4; b++) h.push_back((char)((uint32_t)text.size() >> (8 * b)));
    h += text;
    h.append(4, '\0');                                           // n_ref
    return h;
}

// the refusals' words, the same from both forms
inline std::string bam_offsets_backwards(const char* who) { return std::string(who) + ": the header offsets (d_hdr_off) run backwards"; }
inline std::string bam_offsets_end(const char* who, uint64_t hdr_bytes) {
    return std::string(who) + ": the header offsets (d_hdr_off) do not end at the " + std::to_string(hdr_bytes) + " header bytes given";
}
inline std::string bam_lengths_sum(const char* who, uint64_t sum, uint64_t n_bases) {
    return std::string(who) + ": the lengths (d_len) add up to " + std::to_string(sum) + " bases, not the " + std::to_string(n_bases) + " given";
}
inline std::string bam_name_refusal(const char* who, uint64_t read, uint64_t bytes) {
    return std::string(who) + ": read " + std::to_string(read) + ": its name has " + std::to_string(bytes) + " bytes, BAM allows " + std::to_string(BAM_MAX_NAME);
}
inline std::string bam_qual_refusal(const char* who, uint64_t read) { return std::string(who) + ": read " + std::to_string(read) + ": a quality byte below 33"; }
inline std::string bam_need(const char* who, uint64_t bytes) { return std::string(who) + ": the records need " + std::to_string(bytes) + " bytes"; }
// what both forms refuse before anything is touched; empty = the arguments will do
inline std::string bam_args_refusal(const char* who, const leon_record_layout* lay, const void* bases, const void* len, uint64_t n_reads, uint64_t n_bases,
                                    const void* hdr_text, const void* hdr_off, const void* out_size) {
    const std::string w(who);
    if (!lay || !out_size) return w + ": null argument";
    if (lay->struct_size != sizeof(leon_record_layout)) return w + ": unknown struct_size " + std::to_string(lay->struct_size) + " of leon_record_layout";
    if (n_reads > (1ull << 40) || n_bases > (1ull << 46)) return w + ": implausible sizes";
    if ((n_reads && !len) || (n_bases && !bases)) return w + ": null argument";
    if (hdr_text && !hdr_off) return w + ": headers without their offsets (d_hdr_off)";
    return std::string();
}

// the host form: LEON_OK or a code with *why; the verdicts in the device form's order.  Reads are formatted by n_threads threads
// (0: one per 4 096 reads, at most 16), each its own run of records.
inline int bam_records_host(const char* who, const leon_record_layout* lay, const uint8_t* bases, const uint32_t* len, uint64_t n_reads, uint64_t n_bases,
                            const uint8_t* hdr_text, const uint64_t* hdr_off_in, const uint8_t* quals, uint8_t* out, uint64_t out_cap, uint64_t* rec_off,
                            uint64_t* out_size, uint32_t n_threads, std::string& why) {
    *out_size = 0;
    const uint64_t* hdr_off = hdr_text ? hdr_off_in : nullptr;
    const uint64_t first = lay->first_read_index;
    if (!n_reads) { if (rec_off) rec_off[0] = 0; return LEON_OK; }
    if (hdr_off) {
        for (uint64_t r = 0; r < n_reads; r++) if (hdr_off[r + 1] < hdr_off[r]) { why = bam_offsets_backwards(who); return LEON_E_INVALID; }
        if (hdr_off[n_reads] - hdr_off[0] != lay->hdr_bytes) { why = bam_offsets_end(who, lay->hdr_bytes); return LEON_E_INVALID; }
    }
    const uint8_t* const hdr = hdr_off ? hdr_text - hdr_off[0] : nullptr;       // header r is hdr[hdr_off[r] .. hdr_off[r + 1])
    std::vector<uint64_t> off(n_reads + 1, 0), base_at(n_reads + 1, 0);
    std::vector<uint32_t> name_len(n_reads, 0);
    uint64_t bad_name = ~0ull;
    for (uint64_t r = 0; r < n_reads; r++) {
        uint64_t hl, nl;
        if (hdr_off) {
            const uint8_t* h = hdr + hdr_off[r];
            hl = hdr_off[r + 1] - hdr_off[r];
            for (nl = 0; nl < hl && h[nl] != ' ' && h[nl] != '\t'; nl++) {}
        } else hl = nl = bam_dec_digits(first + r);
        if (nl > BAM_MAX_NAME && bad_name == ~0ull) bad_name = r;
        name_len[r] = (uint32_t)std::min<uint64_t>(nl, 0xFFFFFFFFull);
        off[r + 1] = off[r] + bam_record_size(nl, hl, len[r]);
        base_at[r + 1] = base_at[r] + len[r];
    }
    if (base_at[n_reads] != n_bases) { why = bam_lengths_sum(who, base_at[n_reads], n_bases); return LEON_E_INVALID; }
    if (bad_name != ~0ull) { why = bam_name_refusal(who, first + bad_name, name_len[bad_name]); return LEON_E_INVALID; }
    *out_size = off[n_reads];
    if (off[n_reads] > out_cap || !out) { why = bam_need(who, off[n_reads]); return LEON_E_OVERFLOW; }
    const bool with_quals = lay->fastq && quals;
    std::atomic<uint64_t> bad_qual{~0ull};
    auto format = [&](uint64_t ra, uint64_t rb) {
        uint8_t code[256];
        for (uint32_t c = 0; c < 256; c++) code[c] = (uint8_t)bam_base_code(c);
        for (uint64_t r = ra; r < rb; r++) {
            uint8_t* w = out + off[r];
            const uint64_t l = len[r], nl = name_len[r], hl = hdr_off ? hdr_off[r + 1] - hdr_off[r] : nl;
            const uint32_t l_name = (uint32_t)(nl ? nl : 1) + 1;
            for (uint32_t k = 0; k < BAM_FIXED / 4; k++) {
                const uint32_t v = bam_fixed_word(k, (uint32_t)(off[r + 1] - off[r] - 4), l_name, (uint32_t)l);
                for (int b = 0; b < 4; b++) *w++ = (uint8_t)(v >> (8 * b));
            }
            if (!nl) *w++ = '*';
            else if (hdr_off) { memcpy(w, hdr + hdr_off[r], nl); w += nl; }
            else { const std::string idx = std::to_string(first + r); memcpy(w, idx.data(), nl); w += nl; }
            *w++ = 0;
            const uint8_t* s = bases + base_at[r];
            for (uint64_t j = 0; j + 1 < l; j += 2) *w++ = (uint8_t)(code[s[j]] << 4 | code[s[j + 1]]);
            if (l & 1) *w++ = (uint8_t)(code[s[l - 1]] << 4);
            if (with_quals) {
                const uint8_t* q = quals + base_at[r];
                bool low = false;
                for (uint64_t j = 0; j < l; j++) { low |= q[j] < 33; w[j] = (uint8_t)(q[j] - 33); }
                if (low) { uint64_t seen = bad_qual.load(); while (r < seen && !bad_qual.compare_exchange_weak(seen, r)) {} }
            } else memset(w, 0xFF, l);
            w += l;
            if (hl > nl + 1) {
                *w++ = 'C'; *w++ = 'O'; *w++ = 'Z';
                memcpy(w, hdr + hdr_off[r] + nl + 1, hl - nl - 1); w += hl - nl - 1;
                *w++ = 0;
            }
        }
    };
    if (n_threads == 0) n_threads = 16;
    n_threads = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_threads, n_reads / 4096 + 1));
    if (n_threads <= 1) format(0, n_reads);
    else {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < n_threads; t++) th.emplace_back(format, n_reads * t / n_threads, n_reads * (t + 1) / n_threads);
        for (auto& t : th) t.join();
    }
    if (rec_off) memcpy(rec_off, off.data(), (n_reads + 1) * 8);
    if (bad_qual.load() != ~0ull) { why = bam_qual_refusal(who, first + bad_qual.load()); return LEON_E_INVALID; }
    return LEON_OK;
}

}  // namespace leon
