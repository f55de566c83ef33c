// host_fasta.h -- the FASTA record split in plain serial code (leon_host_fasta_split, host_streams.cpp): the contract of
// leon_fasta_split_device (fastq_kernels.hip) as a loop someone can read, DESIGN.md 4.17.  Needs nothing but include/leon_dna.h.
#pragma once
#include "../../include/leon_dna.h"

#include <string.h>

namespace leon {

// what both forms refuse before anything is touched; nullptr = the arguments will do
inline const char* fasta_split_refusal(const void* text, uint64_t n_text, const void* headers, const void* header_off, const void* bases, const void* base_off,
                                       const void* res) {
    if (!res) return "fasta split: res is NULL";
    if (n_text >> 32) return "fasta split: n_text is 2^32 or more";
    if (n_text && !text) return "fasta split: text is NULL with text given";
    if (!headers || !header_off || !bases || !base_off) return "fasta split: a NULL output";
    return nullptr;
}

// the line that begins at `at` (< n_text): [at, e) without its terminator, `next` the first byte behind it; false when the text has
// no '\n' from `at` on and the end of the text ends no line
inline bool fasta_line(const uint8_t* text, uint64_t n_text, int last, uint64_t at, uint64_t& e, uint64_t& next) {
    const uint8_t* nl = (const uint8_t*)memchr(text + at, '\n', n_text - at);
    if (!nl && !last) return false;
    e = nl ? (uint64_t)(nl - text) : n_text;
    next = nl ? e + 1 : n_text;
    if (nl && e > at && text[e - 1] == '\r') e--;
    return true;
}

// LEON_OK or LEON_E_OVERFLOW (the arguments have passed fasta_split_refusal)
inline int fasta_split(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap, uint8_t* headers, uint64_t* header_off,
                       uint8_t* bases, uint64_t* base_off, uint64_t bytes_cap, uint64_t records_cap, leon_fasta_split_result* res) {
    leon_fasta_split_result R;
    memset(&R, 0, sizeof R);
    bool fits = records_cap >= 1;
    if (fits) header_off[0] = base_off[0] = 0;
    const bool any = wrap == LEON_FASTA_ANY_WIDTH;
    uint64_t at = 0;                                            // where record n_records begins
    for (;;) {
        R.consumed = at;
        if (R.n_records == max_records) { R.stop = LEON_FASTA_MAX; break; }
        if (at >= n_text) { R.stop = LEON_FASTA_END; break; }
        if (text[at] != '>') {                                  // (only the text's first byte can: every other record begins where a '>' was seen)
            R.stop = LEON_FASTA_IRREGULAR; R.reason = LEON_FASTA_R_HEADER;
            for (R.next_header = n_text;;) {                    // the first line that begins with '>'
                const uint8_t* nl = (const uint8_t*)memchr(text + at, '\n', n_text - at);
                if (!nl || (at = (uint64_t)(nl - text) + 1) >= n_text) break;
                if (text[at] == '>') { R.next_header = at; break; }
            }
            break;
        }
        // first walk: is the record whole, which of its lines offends first, how long are its parts
        uint64_t e, next, n_lines = 0, len = 0, seq_bytes = 0;
        uint32_t why = LEON_FASTA_R_NONE;
        bool whole = fasta_line(text, n_text, last, at, e, next);
        const uint64_t hl = whole ? e - at - 1 : 0, seq_at = next;
        while (whole && next < n_text && text[next] != '>') {
            const uint64_t b = next;
            if (!(whole = fasta_line(text, n_text, last, b, e, next))) break;
            len = e - b; n_lines++; seq_bytes += len;
            const bool ends = next >= n_text || text[next] == '>';
            if (why || any) continue;
            if (len == 0) why = LEON_FASTA_R_EMPTY_LINE;
            else if (wrap == 0) { if (!ends) why = LEON_FASTA_R_MULTILINE; }
            else if (ends ? len > wrap : len != wrap) why = LEON_FASTA_R_WIDTH;
        }
        if (whole && next >= n_text && !last) whole = false;   // no header line behind it, and the text may go on
        if (!whole) { R.stop = LEON_FASTA_END; break; }
        if (!n_lines && !any) why = LEON_FASTA_R_NO_SEQUENCE;   // (the header line offends: in front of every other line)
        if (why) { R.stop = LEON_FASTA_IRREGULAR; R.reason = why; R.next_header = next; break; }
        fits = fits && R.n_records + 2 <= records_cap && R.header_bytes + hl <= bytes_cap && R.base_bytes + seq_bytes <= bytes_cap;
        if (fits) {                                             // second walk: the lines joined
            if (hl) memcpy(headers + R.header_bytes, text + at + 1, hl);
            uint64_t to = R.base_bytes;
            for (uint64_t b = seq_at; b < next;) {
                uint64_t le = b, ln = next;
                (void)fasta_line(text, n_text, last, b, le, ln);
                if (le > b) memcpy(bases + to, text + b, le - b);
                to += le - b; b = ln;
            }
            header_off[R.n_records + 1] = R.header_bytes + hl;
            base_off[R.n_records + 1] = R.base_bytes + seq_bytes;
        }
        if (n_lines == 1 && len > R.single_max) R.single_max = len;
        R.header_bytes += hl; R.base_bytes += seq_bytes;
        R.n_records++; at = next;
    }
    *res = R;
    return fits ? LEON_OK : LEON_E_OVERFLOW;
}

}  // namespace leon
