// host_fastq.h -- the FASTQ record split in plain serial code (leon_host_fastq_split, host_streams.cpp): the contract of
// leon_fastq_split_device (fastq_kernels.hip) as a loop someone can read, DESIGN.md 4.16.  Needs nothing but include/leon_dna.h.
#pragma once
#include "../../include/leon_dna.h"

#include <string.h>

namespace leon {

// what both forms refuse before anything is touched; nullptr = the arguments will do
inline const char* fastq_split_refusal(const void* text, uint64_t n_text, int plus_kind, const void* headers, const void* header_off, const void* bases,
                                       const void* base_off, const void* quals, const void* res) {
    if (!res) return "fastq split: res is NULL";
    if (n_text >> 32) return "fastq split: n_text is 2^32 or more";
    if (n_text && !text) return "fastq split: text is NULL with text given";
    if (plus_kind < -1 || plus_kind > 1) return "fastq split: plus_kind is none of -1, 0, 1";
    if (!headers || !header_off || !bases || !base_off || !quals) return "fastq split: a NULL output";
    return nullptr;
}

// LEON_OK or LEON_E_OVERFLOW (the arguments have passed fastq_split_refusal)
inline int fastq_split(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, int plus_kind, uint8_t* headers, uint64_t* header_off,
                       uint8_t* bases, uint64_t* base_off, uint8_t* quals, uint64_t bytes_cap, uint64_t records_cap, leon_fastq_split_result* res) {
    leon_fastq_split_result R;
    memset(&R, 0, sizeof R);
    bool fits = records_cap >= 1;
    if (fits) header_off[0] = base_off[0] = 0;
    for (;;) {
        if (R.n_records == max_records) { R.stop = LEON_FASTQ_MAX; break; }
        uint64_t b[4], e[4], at = R.consumed;                   // the next four lines: [b, e) without the terminator
        int got = 0;
        bool all_empty = true;
        for (; got < 4; got++) {
            const uint8_t* nl = at < n_text ? (const uint8_t*)memchr(text + at, '\n', n_text - at) : nullptr;
            if (!nl && !(last && at < n_text)) break;
            b[got] = at; e[got] = nl ? (uint64_t)(nl - text) : n_text;
            at = nl ? e[got] + 1 : n_text;
            if (nl && e[got] > b[got] && text[e[got] - 1] == '\r') e[got]--;
            if (e[got] > b[got]) all_empty = false;
        }
        if (got < 4) {                                          // the text ran out
            if (last && !all_empty) { R.stop = LEON_FASTQ_IRREGULAR; R.reason = LEON_FASTQ_R_PARTIAL; }
            else { R.stop = LEON_FASTQ_END; if (last) R.consumed = n_text; }
            break;
        }
        const uint64_t hl = e[0] - b[0] - (e[0] > b[0]), sl = e[1] - b[1], pl = e[2] - b[2];     // header without '@', sequence, '+' line
        uint32_t why = LEON_FASTQ_R_NONE;
        int kind = -1;                                          // of the '+' line: 0 bare, 1 the header again, -1 both
        if (e[0] == b[0] || text[b[0]] != '@') why = LEON_FASTQ_R_HEADER;
        else if (pl == 0 || text[b[2]] != '+') why = LEON_FASTQ_R_PLUS;
        else if (e[3] - b[3] != sl) why = LEON_FASTQ_R_LENGTH;
        else if (pl == 1) kind = hl ? 0 : -1;
        else if (pl - 1 == hl && memcmp(text + b[2] + 1, text + b[0] + 1, hl) == 0) kind = 1;
        else why = LEON_FASTQ_R_PLUS_TEXT;
        if (!why && kind >= 0) {
            if (plus_kind < 0) plus_kind = kind;                // the first record that says which: the rest must say the same
            if (kind != plus_kind) why = LEON_FASTQ_R_PLUS_TEXT;
        }
        if (why) { R.stop = LEON_FASTQ_IRREGULAR; R.reason = why; break; }
        fits = fits && R.n_records + 2 <= records_cap && R.header_bytes + hl <= bytes_cap && R.base_bytes + sl <= bytes_cap;
        if (fits) {
            if (hl) memcpy(headers + R.header_bytes, text + b[0] + 1, hl);
            if (sl) { memcpy(bases + R.base_bytes, text + b[1], sl); memcpy(quals + R.base_bytes, text + b[3], sl); }
            header_off[R.n_records + 1] = R.header_bytes + hl;
            base_off[R.n_records + 1] = R.base_bytes + sl;
        }
        R.header_bytes += hl; R.base_bytes += sl;
        R.plus_bare += kind == 0; R.plus_header += kind == 1;
        R.n_records++; R.consumed = at;
    }
    *res = R;
    return fits ? LEON_OK : LEON_E_OVERFLOW;
}

}  // namespace leon
