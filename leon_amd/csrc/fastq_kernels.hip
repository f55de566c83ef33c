// fastq_kernels.hip -- FASTQ text split into records on the device (leon_fastq_split_device): the mirror of
// fmt_kernels.hip on the encode side.  The contract is include/leon_dna.h's; host_fastq.h states it as a serial loop.
//
//   k_fq_newlines   the text in tiles of FASTQ_TILE bytes cut at 16-byte aligned ADDRESSES, a lane per 16 bytes (one 16-byte load; the
//                   text's first and last partial 16 bytes byte-wise).  First pass: the '\n' of every tile are counted.  A device-wide
//                   exclusive scan of the counts says where a tile's positions go; second pass: every '\n' writes its position to nl[].
//                   A workgroup walks ceil(tiles / FASTQ_MAX_GROUPS) consecutive tiles.
//   k_fq_check      a lane per record r < min(whole records, max_records): its four lines from nl[4r - 1 .. 4r + 3], the '\r' rule, the
//                   four rules; the lengths of its header and sequence and the kind of its '+' line go to in[r], the first record
//                   that breaks a rule and the first records with a bare '+' and with a repeated header to three minima across the
//                   grid (reduced per wave first).  One more lane looks at the lines behind the last whole record.
//   (host)          reads the minima back, fixes n_records, scans in[0 .. n_records] into offsets and totals.
//   k_fq_offsets    the two offset tables from that scan.
//   k_fq_split      a wave per record: the header, the bases and the qualities copied byte by byte, lane i the bytes i, i + 64, ... --
//                   both the source and the destination of a field are contiguous per wave, at whatever alignment either has.
//
// ... and FASTA text (leon_fasta_split_device; host_fasta.h is its serial statement).  A record has any number of
// lines, so everything is per LINE: the header blob is the header lines back to back, the bases blob the sequence lines back to back, and
// one scan over the lines gives every line's destination and its record.
//
//   k_fq_newlines   as above, unchanged: nl[].
//   k_fa_lines      a lane per line: its bounds under the '\r' rule, header or sequence from its first byte, whether the line behind
//                   it is a header (that line's first byte); {header bytes, base bytes, 1 if header} to in[], the rule of the call's
//                   `wrap` it breaks to why[].
//   (scan)          prim::ExclusiveSum of in[] over the lines.
//   k_fa_heads      a lane per line, its record now known from the scan: a header line writes {scan, line, first byte} to rec[its
//                   record]; the first offending line among the records that count goes to two minima across the grid (per wave first).
//   (host)          reads the minima and the header count back, fixes n_records, reads rec[n_records] and rec[n_records + 1].
//   k_fa_offsets    a lane per record: the two offset tables from rec[]; the longest one-line record through a per-wave maximum.
//   k_fa_split      FA_LANES lanes per line: the line's bytes copied contiguously to headers + scan.hdr (behind the '>') or to
//                   bases + scan.base -- a contig of a million lines spreads over the grid like a million reads.
#include "kernels.h"
#include "prim.h"
#include "device_call.h"
#include "host_fastq.h"
#include "host_fasta.h"

#include <algorithm>

namespace leon {

struct FqSum {                                                  // what the scan carries: header bytes, bases, '+' lines of the two kinds
    uint64_t hdr, base;
    uint32_t bare, rep;
    FqSum() = default;
    __host__ __device__ FqSum(int v) : hdr((uint64_t)v), base((uint64_t)v), bare((uint32_t)v), rep((uint32_t)v) {}
    __host__ __device__ FqSum(uint64_t h, uint64_t b, uint32_t p0, uint32_t p1) : hdr(h), base(b), bare(p0), rep(p1) {}
    __host__ __device__ FqSum operator+(const FqSum& o) const { return FqSum(hdr + o.hdr, base + o.base, bare + o.bare, rep + o.rep); }
};
struct FqFound {                                                // the grid's minima, all ones = none
    unsigned long long first_bad;                               // (record << 8) | the rule it broke
    unsigned long long first_bare, first_rep;                   // the first record whose '+' line is bare / repeats a non-empty header
    uint32_t tail_nonempty, pad;                                // a non-empty line behind the last whole record
};
struct FaSum {                                                  // FASTA, per line: header bytes (without the '>'), bases, 1 for a header line
    uint64_t hdr, base;
    uint32_t cnt, pad;
    FaSum() = default;
    __host__ __device__ FaSum(int v) : hdr((uint64_t)v), base((uint64_t)v), cnt((uint32_t)v), pad(0) {}
    __host__ __device__ FaSum(uint64_t h, uint64_t b, uint32_t c) : hdr(h), base(b), cnt(c), pad(0) {}
    __host__ __device__ FaSum operator+(const FaSum& o) const { return FaSum(hdr + o.hdr, base + o.base, cnt + o.cnt); }
};
struct FaRec {                                                  // per record: the scan at its header line, that line and its first byte
    uint64_t hdr, base;
    uint32_t line, begin;
};
struct FaFound {
    unsigned long long first_bad_line;                          // (line << 8) | the reason, all ones = none; and that line's record
    unsigned long long first_bad_rec;
    unsigned long long n_headers, single_max;
};

namespace {

constexpr uint32_t FQ_THREADS = 256;
static_assert(FASTQ_TILE == FQ_THREADS * 16, "a lane of k_fq_newlines takes 16 bytes");
constexpr unsigned long long FQ_NONE = ~0ull;

__device__ __forceinline__ uint64_t fq_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// bit 7 of every byte of w that is '\n' (exact: no carry leaves a byte)
__device__ __forceinline__ uint32_t nl_bits(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// Bounds: text is read at [0, n_text) only -- a 16-byte load is made for a chunk that lies whole inside, every other byte is loaded
// alone after its position was tested; cnt[] is indexed below n_tiles; nl[] below n_nl (tested before every store).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_fq_newlines(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t n_tiles, uint64_t tiles_per_group,
                                                     uint32_t* __restrict__ cnt /* per tile: its count (out) / its first place in nl (in) */,
                                                     uint32_t* __restrict__ nl, uint64_t n_nl) {
    __shared__ uint32_t s_wave[2][4];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t mis = (uint32_t)((uintptr_t)text & 15);      // virtual position v is text byte v - mis: v = 0 is the aligned address below the text
    uint32_t par = 0;
    for (uint64_t k = 0; k < tiles_per_group; k++) {
        const uint64_t tile = blockIdx.x * tiles_per_group + k;
        if (tile >= n_tiles) break;                             // (uniform)
        const uint64_t cv = tile * FASTQ_TILE + t * 16u;
        uint64_t lo = cv > mis ? cv - mis : 0, hi = fq_min(cv + 16 - mis, n_text);
        if (lo > hi) lo = hi;
        uint32_t m[4] = {0, 0, 0, 0};
        if (hi - lo == 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(text + lo);
            m[0] = nl_bits(v.x); m[1] = nl_bits(v.y); m[2] = nl_bits(v.z); m[3] = nl_bits(v.w);
        } else {
            for (uint64_t p = lo; p < hi; p++) {
                const uint32_t j = (uint32_t)(p + mis - cv);
                if (text[p] == '\n') m[j >> 2] |= 0x80u << (8 * (j & 3));
            }
        }
        const uint32_t c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
        uint32_t incl = c;
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d); if (lane >= d) incl += o; }
        if (lane == 63) s_wave[par][wave] = incl;
        __syncthreads();                                        // (s_wave has two halves: the next tile's writes do not meet this tile's reads)
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; w++) { const uint32_t x = s_wave[par][w]; if (w < wave) before += x; total += x; }
        par ^= 1;
        if (!WRITE) {
            if (t == 0) cnt[tile] = total;
        } else {
            uint64_t at = (uint64_t)cnt[tile] + before + incl - c;
#pragma unroll
            for (uint32_t w = 0; w < 4; w++)
                for (uint32_t mm = m[w]; mm; mm &= mm - 1) {
                    const uint32_t j = 4 * w + ((uint32_t)(__ffs((int)mm) - 1) >> 3);
                    if (at < n_nl) nl[at] = (uint32_t)(cv + j - mis);
                    at++;
                }
        }
    }
}

// line i of the text: [begin, end) without its '\n'; i < n_lines (n_lines is n_nl, or n_nl + 1 when an unterminated line ends the text).
// What nl[] holds is bounded by n_text before it is used.
__device__ __forceinline__ uint64_t fq_line_begin(const uint32_t* __restrict__ nl, uint64_t n_nl, uint64_t n_text, uint64_t i) {
    const uint64_t k = fq_min(i, n_nl);
    return k == 0 ? 0 : fq_min((uint64_t)nl[k - 1] + 1, n_text);
}
__device__ __forceinline__ uint64_t fq_line_end(const uint32_t* __restrict__ nl, uint64_t n_nl, uint64_t n_text, uint64_t i) {
    return i < n_nl ? fq_min(nl[i], n_text) : n_text;
}
// ... and its end under the '\r' rule
__device__ __forceinline__ uint64_t fq_line_end_cr(const uint8_t* __restrict__ text, const uint32_t* __restrict__ nl, uint64_t n_nl, uint64_t n_text,
                                                   uint64_t i, uint64_t begin) {
    uint64_t e = fq_line_end(nl, n_nl, n_text, i);
    if (e < begin) e = begin;
    if (i < n_nl && e > begin && text[e - 1] == '\r') e--;
    return e;
}

__device__ __forceinline__ void fq_wave_min(unsigned long long v, unsigned long long* dst) {
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); if (o < v) v = o; }
    if ((threadIdx.x & 63) == 0 && v != FQ_NONE && v < *dst) atomicMin(dst, v);     // (a stale *dst only costs an atomic)
}

// Bounds: nl[] below n_nl, text below n_text (every line bound is clamped to it), in[] up to rec_n.
__global__ __launch_bounds__(256) void k_fq_check(const uint8_t* __restrict__ text, uint64_t n_text, const uint32_t* __restrict__ nl, uint64_t n_nl,
                                                  uint64_t n_lines, uint64_t rec_n, int tail, FqSum* __restrict__ in, FqFound* __restrict__ found) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    unsigned long long bad = FQ_NONE, bare = FQ_NONE, rep = FQ_NONE;
    if (r < rec_n) {
        uint64_t b[4], e[4];
        for (uint32_t i = 0; i < 4; i++) { b[i] = fq_line_begin(nl, n_nl, n_text, 4 * r + i); e[i] = fq_line_end_cr(text, nl, n_nl, n_text, 4 * r + i, b[i]); }
        const uint64_t hl = e[0] - b[0] - (e[0] > b[0]), sl = e[1] - b[1], pl = e[2] - b[2];
        uint32_t why = LEON_FASTQ_R_NONE;
        int kind = -1;
        if (e[0] == b[0] || text[b[0]] != '@') why = LEON_FASTQ_R_HEADER;
        else if (pl == 0 || text[b[2]] != '+') why = LEON_FASTQ_R_PLUS;
        else if (e[3] - b[3] != sl) why = LEON_FASTQ_R_LENGTH;
        else if (pl == 1) kind = hl ? 0 : -1;
        else if (pl - 1 == hl) {
            bool same = true;
            for (uint64_t i = 0; i < hl && same; i++) same = text[b[2] + 1 + i] == text[b[0] + 1 + i];
            if (same) kind = 1; else why = LEON_FASTQ_R_PLUS_TEXT;
        } else why = LEON_FASTQ_R_PLUS_TEXT;
        in[r] = FqSum(hl, sl, kind == 0, kind == 1);
        if (why) bad = ((unsigned long long)r << 8) | why;
        else if (kind == 0) bare = r;
        else if (kind == 1) rep = r;
    } else if (r == rec_n) {
        in[r] = FqSum(0);
        if (tail)                                               // the lines behind the last whole record (fewer than four)
            for (uint64_t i = 4 * rec_n; i < n_lines; i++) {
                const uint64_t lb = fq_line_begin(nl, n_nl, n_text, i);
                if (fq_line_end_cr(text, nl, n_nl, n_text, i, lb) > lb) found->tail_nonempty = 1;
            }
    }
    fq_wave_min(bad, &found->first_bad);
    fq_wave_min(bare, &found->first_bare);
    fq_wave_min(rep, &found->first_rep);
}

__global__ __launch_bounds__(256) void k_fq_offsets(const FqSum* __restrict__ off, uint64_t n, uint64_t* __restrict__ header_off, uint64_t* __restrict__ base_off) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r <= n) { header_off[r] = off[r].hdr; base_off[r] = off[r].base; }
}

// A wave per record.  Bounds: the record is below n_records; its lines begin below n_text and a field's length is cut to what the text
// has behind its line's first byte; the destinations end at off[n_records], which the caller has tested against the capacities.
__global__ __launch_bounds__(256) void k_fq_split(const uint8_t* __restrict__ text, uint64_t n_text, const uint32_t* __restrict__ nl, uint64_t n_nl,
                                                  const FqSum* __restrict__ off, uint64_t n_records, uint8_t* __restrict__ headers,
                                                  uint8_t* __restrict__ bases, uint8_t* __restrict__ quals) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = blockIdx.x * (uint64_t)(blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= n_records) return;                                 // (uniform in the wave)
    const FqSum o0 = off[r], o1 = off[r + 1];
    const uint64_t b0 = fq_min(fq_line_begin(nl, n_nl, n_text, 4 * r) + 1, n_text);          // behind the '@'
    const uint64_t b1 = fq_line_begin(nl, n_nl, n_text, 4 * r + 1), b3 = fq_line_begin(nl, n_nl, n_text, 4 * r + 3);
    const uint64_t hl = fq_min(o1.hdr - o0.hdr, n_text - b0), sl = fq_min(o1.base - o0.base, fq_min(n_text - b1, n_text - b3));
    const uint8_t* __restrict__ sh = text + b0; uint8_t* __restrict__ dh = headers + o0.hdr;
    for (uint64_t i = lane; i < hl; i += 64) dh[i] = sh[i];
    const uint8_t* __restrict__ sb = text + b1; uint8_t* __restrict__ db = bases + o0.base;
    const uint8_t* __restrict__ sq = text + b3; uint8_t* __restrict__ dq = quals + o0.base;
    for (uint64_t i = lane; i < sl; i += 64) { const uint8_t x = sb[i], y = sq[i]; db[i] = x; dq[i] = y; }
}

hipError_t fq_count_scan(void* tmp, size_t& bytes, const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t s) { return prim::ExclusiveSum(tmp, bytes, in, out, n, s); }
hipError_t fq_sum_scan(void* tmp, size_t& bytes, const FqSum* in, FqSum* out, uint64_t n, hipStream_t s) { return prim::ExclusiveSum(tmp, bytes, in, out, n, s); }

// ---- FASTA ----
constexpr uint32_t FA_LANES = 16;                               // lanes of k_fa_split that share a line: four lines a wave

__device__ __forceinline__ void fa_wave_max(unsigned long long v, unsigned long long* dst) {
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); if (o > v) v = o; }
    if ((threadIdx.x & 63) == 0 && v > *dst) atomicMax(dst, v);                     // (a stale *dst only costs an atomic)
}

// A lane per line i < n_lines (n_lines is n_nl, + 1 when bytes lie behind the last '\n': that line's length is only known with `last`, its
// first byte always); lane n_lines writes the scan's closing zero.  Bounds: nl[] below n_nl, text below n_text (every line bound is
// cut to it, the byte behind a '\n' is tested against it before it is read), in[] up to n_lines, why[] below n_lines.
__global__ __launch_bounds__(256) void k_fa_lines(const uint8_t* __restrict__ text, uint64_t n_text, const uint32_t* __restrict__ nl, uint64_t n_nl,
                                                  uint64_t n_lines, int last, uint64_t wrap, FaSum* __restrict__ in, uint8_t* __restrict__ why) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i > n_lines) return;
    if (i == n_lines) { in[i] = FaSum(0); return; }
    const uint64_t b = fq_line_begin(nl, n_nl, n_text, i), e = fq_line_end_cr(text, nl, n_nl, n_text, i, b), len = e - b;
    const bool header = len && text[b] == '>';
    bool ends = last && i + 1 == n_lines;                       // the record's last line: a header line follows, or the text ends and that ends it
    if (i < n_nl) { const uint64_t nb = (uint64_t)nl[i] + 1; if (nb < n_text && text[nb] == '>') ends = true; }
    uint32_t w = LEON_FASTA_R_NONE;
    if (wrap != LEON_FASTA_ANY_WIDTH) {
        if (header) { if (ends) w = LEON_FASTA_R_NO_SEQUENCE; }
        else if (len == 0) w = LEON_FASTA_R_EMPTY_LINE;
        else if (wrap == 0) { if (!ends) w = LEON_FASTA_R_MULTILINE; }
        else if (ends ? len > wrap : len != wrap) w = LEON_FASTA_R_WIDTH;
    }
    in[i] = header ? FaSum(len - 1, 0, 1) : FaSum(0, len, 0);
    why[i] = (uint8_t)w;
}

// A lane per line, behind the scan.  The records that count are the whole ones (all with `last`, else all but the last) below
// max_records.  Bounds: in[], off[] up to n_lines; a record index is below the header count off[n_lines].cnt <= n_lines, and rec[] has
// n_lines + 2 entries; nl[] and n_text as in k_fa_lines.
__global__ __launch_bounds__(256) void k_fa_heads(const uint32_t* __restrict__ nl, uint64_t n_nl, uint64_t n_text, uint64_t n_lines, int last, uint64_t max_records,
                                                  const FaSum* __restrict__ in, const FaSum* __restrict__ off, const uint8_t* __restrict__ why,
                                                  FaRec* __restrict__ rec, FaFound* __restrict__ found) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t n_headers = off[n_lines].cnt, whole = last ? n_headers : n_headers ? n_headers - 1 : 0, rec_n = fq_min(whole, max_records);
    unsigned long long bad_line = FQ_NONE, bad_rec = FQ_NONE;
    if (i < n_lines) {
        const FaSum o = off[i];
        const uint32_t header = in[i].cnt;
        if (header) rec[o.cnt] = FaRec{o.hdr, o.base, (uint32_t)i, (uint32_t)fq_line_begin(nl, n_nl, n_text, i)};
        const uint64_t r = (uint64_t)o.cnt + header;            // 1 + the line's record; 0: a line in front of the first header line
        if (why[i] && r && r - 1 < rec_n) { bad_line = ((unsigned long long)i << 8) | why[i]; bad_rec = r - 1; }
    } else if (i == n_lines) {
        const FaSum o = off[i];
        rec[n_headers] = rec[n_headers + 1] = FaRec{o.hdr, o.base, (uint32_t)n_lines, (uint32_t)n_text};
        found->n_headers = n_headers;
    }
    fq_wave_min(bad_line, &found->first_bad_line);
    fq_wave_min(bad_rec, &found->first_bad_rec);
}

// A lane per record r <= n.  Bounds: rec[] up to n + 1 (it has two entries behind the last header's); the tables' n + 1 entries, which
// the caller has tested against records_cap (tables == 0: they did not fit, only the maximum is taken).
__global__ __launch_bounds__(256) void k_fa_offsets(const FaRec* __restrict__ rec, uint64_t n, int tables, uint64_t* __restrict__ header_off,
                                                    uint64_t* __restrict__ base_off, FaFound* __restrict__ found) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    unsigned long long single = 0;
    if (r <= n) {
        const FaRec a = rec[r];
        if (tables) { header_off[r] = a.hdr; base_off[r] = a.base - rec[0].base; }       // (rec[0].base: what lies in front of the first header line; then n is 0)
        if (r < n) { const FaRec b = rec[r + 1]; if (b.line - a.line == 2) single = b.base - a.base; }
    }
    fa_wave_max(single, &found->single_max);
}

// FA_LANES lanes per line i < n_split_lines (the lines of the records that are split).  Bounds: in[], off[] below n_split_lines; a line
// begins below n_text and its length is cut to what the text has behind its first byte; a destination ends at or below the scan at
// line n_split_lines, which the caller has tested against the capacities.
__global__ __launch_bounds__(256) void k_fa_split(const uint8_t* __restrict__ text, uint64_t n_text, const uint32_t* __restrict__ nl, uint64_t n_nl,
                                                  const FaSum* __restrict__ in, const FaSum* __restrict__ off, uint64_t n_split_lines,
                                                  uint8_t* __restrict__ headers, uint8_t* __restrict__ bases) {
    const uint32_t lane = threadIdx.x % FA_LANES;
    const uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / FA_LANES;
    if (i >= n_split_lines) return;
    const FaSum a = in[i], o = off[i];
    const uint64_t b = fq_min(fq_line_begin(nl, n_nl, n_text, i) + a.cnt, n_text);       // a header: behind the '>'
    const uint64_t len = fq_min(a.cnt ? a.hdr : a.base, n_text - b);
    const uint8_t* __restrict__ src = text + b;
    uint8_t* __restrict__ dst = a.cnt ? headers + o.hdr : bases + o.base;
    for (uint64_t k = lane; k < len; k += FA_LANES) dst[k] = src[k];
}

hipError_t fa_sum_scan(void* tmp, size_t& bytes, const FaSum* in, FaSum* out, uint64_t n, hipStream_t s) { return prim::ExclusiveSum(tmp, bytes, in, out, n, s); }

}  // namespace
}  // namespace leon

using namespace leon;

extern "C" int leon_fastq_split_device(int device_id, const uint8_t* d_text, uint64_t n_text, int last, uint64_t max_records, int plus_kind,
                                       uint8_t* d_headers, uint64_t* d_header_off, uint8_t* d_bases, uint64_t* d_base_off, uint8_t* d_quals,
                                       uint64_t bytes_cap, uint64_t records_cap, leon_fastq_split_result* res) {
    if (const char* why = fastq_split_refusal(d_text, n_text, plus_kind, d_headers, d_header_off, d_bases, d_base_off, d_quals, res))
        return dev_fail(LEON_E_INVALID, std::string("leon_fastq_split_device: ") + why);
    leon_fastq_split_result R{};
    *res = R;
    CallStream st;
    if (const int rc = dev_open("leon_fastq_split_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    OwnBuf d_cnt, d_first, d_nl, d_in, d_off, d_found, d_tmp;
    size_t tmp_bytes = 0;
    // every '\n' of the text, in order
    const uint64_t n_tiles = n_text ? (((uintptr_t)d_text & 15) + n_text + FASTQ_TILE - 1) / FASTQ_TILE : 0;
    const uint64_t per = std::max<uint64_t>((n_tiles + FASTQ_MAX_GROUPS - 1) / FASTQ_MAX_GROUPS, 1), groups = (n_tiles + per - 1) / per;
    uint32_t n_nl32 = 0;
    uint8_t last_byte = '\n';
    if (n_tiles) {
        DEVCHK(d_cnt.ensure((n_tiles + 1) * sizeof(uint32_t))); DEVCHK(d_first.ensure((n_tiles + 1) * sizeof(uint32_t)));
        DEVCHK(hipMemsetAsync(d_cnt.as<uint32_t>() + n_tiles, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_fq_newlines<false>, dim3((uint32_t)groups), dim3(FQ_THREADS), 0, s, d_text, n_text, n_tiles, per, d_cnt.as<uint32_t>(), nullptr, 0);
        DEVCHK(hipGetLastError());
        DEVCHK(fq_count_scan(nullptr, tmp_bytes, d_cnt.as<uint32_t>(), d_first.as<uint32_t>(), n_tiles + 1, s));
        DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        DEVCHK(fq_count_scan(d_tmp.p, tmp_bytes, d_cnt.as<uint32_t>(), d_first.as<uint32_t>(), n_tiles + 1, s));
        DEVCHK(hipMemcpyAsync(&n_nl32, d_first.as<uint32_t>() + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        DEVCHK(hipMemcpyAsync(&last_byte, d_text + n_text - 1, 1, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
    }
    const uint64_t n_nl = std::min<uint64_t>(n_nl32, n_text);
    DEVCHK(d_nl.ensure((n_nl + 1) * sizeof(uint32_t)));
    if (n_nl) {
        hipLaunchKernelGGL(k_fq_newlines<true>, dim3((uint32_t)groups), dim3(FQ_THREADS), 0, s, d_text, n_text, n_tiles, per, d_first.as<uint32_t>(), d_nl.as<uint32_t>(), n_nl);
        DEVCHK(hipGetLastError());
    }
    // the records the text has whole, and which of them are regular
    const uint64_t n_lines = n_nl + (last && n_text && last_byte != '\n' ? 1 : 0), whole = n_lines / 4, rec_n = std::min(whole, max_records);
    DEVCHK(d_in.ensure((rec_n + 1) * sizeof(FqSum))); DEVCHK(d_off.ensure((rec_n + 1) * sizeof(FqSum)));
    DEVCHK(d_found.ensure(sizeof(FqFound)));
    DEVCHK(hipMemsetAsync(d_found.p, 0xFF, offsetof(FqFound, tail_nonempty), s));
    DEVCHK(hipMemsetAsync(d_found.as<uint8_t>() + offsetof(FqFound, tail_nonempty), 0, sizeof(FqFound) - offsetof(FqFound, tail_nonempty), s));
    hipLaunchKernelGGL(k_fq_check, dim3((uint32_t)((rec_n + 1 + 255) / 256)), dim3(256), 0, s, d_text, n_text, d_nl.as<uint32_t>(), n_nl, n_lines, rec_n,
                       last && rec_n == whole ? 1 : 0, d_in.as<FqSum>(), d_found.as<FqFound>());
    DEVCHK(hipGetLastError());
    FqFound F;
    DEVCHK(hipMemcpyAsync(&F, d_found.p, sizeof F, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    // the first record that is not regular: by a rule of its own, or by a '+' line that is the other of the two kinds
    uint64_t first_irregular = F.first_bad == FQ_NONE ? ~0ull : F.first_bad >> 8;
    uint32_t why = F.first_bad == FQ_NONE ? LEON_FASTQ_R_NONE : (uint32_t)(F.first_bad & 255);
    const uint64_t other = plus_kind == 0 ? F.first_rep : plus_kind == 1 ? F.first_bare
                         : F.first_bare != FQ_NONE && F.first_rep != FQ_NONE ? std::max(F.first_bare, F.first_rep) : FQ_NONE;
    if (other < first_irregular) { first_irregular = other; why = LEON_FASTQ_R_PLUS_TEXT; }
    R.n_records = std::min(first_irregular, rec_n);
    if (R.n_records == max_records) R.stop = LEON_FASTQ_MAX;
    else if (R.n_records < rec_n) { R.stop = LEON_FASTQ_IRREGULAR; R.reason = why; }
    else if (last && F.tail_nonempty) { R.stop = LEON_FASTQ_IRREGULAR; R.reason = LEON_FASTQ_R_PARTIAL; }
    else R.stop = LEON_FASTQ_END;
    // offsets and totals
    const uint64_t n = R.n_records;
    DEVCHK(fq_sum_scan(nullptr, tmp_bytes, d_in.as<FqSum>(), d_off.as<FqSum>(), n + 1, s));
    DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    DEVCHK(fq_sum_scan(d_tmp.p, tmp_bytes, d_in.as<FqSum>(), d_off.as<FqSum>(), n + 1, s));
    FqSum total;
    uint32_t end_nl = 0;
    DEVCHK(hipMemcpyAsync(&total, d_off.as<FqSum>() + n, sizeof total, hipMemcpyDeviceToHost, s));
    if (n && 4 * n - 1 < n_nl) DEVCHK(hipMemcpyAsync(&end_nl, d_nl.as<uint32_t>() + (4 * n - 1), sizeof end_nl, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    R.consumed = !n ? 0 : 4 * n - 1 < n_nl ? std::min<uint64_t>((uint64_t)end_nl + 1, n_text) : n_text;
    if (R.stop == LEON_FASTQ_END && last) R.consumed = n_text;
    R.header_bytes = total.hdr; R.base_bytes = total.base; R.plus_bare = total.bare; R.plus_header = total.rep;
    *res = R;
    if (n + 1 > records_cap || total.hdr > bytes_cap || total.base > bytes_cap)
        return dev_fail(LEON_E_OVERFLOW, "leon_fastq_split_device: " + std::to_string(n) + " records need " + std::to_string(total.hdr) + " header bytes, " +
                                             std::to_string(total.base) + " bases and " + std::to_string(n + 1) + " table entries");
    hipLaunchKernelGGL(k_fq_offsets, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, s, d_off.as<FqSum>(), n, d_header_off, d_base_off);
    DEVCHK(hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(k_fq_split, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, d_text, n_text, d_nl.as<uint32_t>(), n_nl, d_off.as<FqSum>(), n, d_headers, d_bases, d_quals);
        DEVCHK(hipGetLastError());
    }
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}

extern "C" int leon_fasta_split_device(int device_id, const uint8_t* d_text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap, uint8_t* d_headers,
                                       uint64_t* d_header_off, uint8_t* d_bases, uint64_t* d_base_off, uint64_t bytes_cap, uint64_t records_cap,
                                       leon_fasta_split_result* res) {
    if (const char* why = fasta_split_refusal(d_text, n_text, d_headers, d_header_off, d_bases, d_base_off, res))
        return dev_fail(LEON_E_INVALID, std::string("leon_fasta_split_device: ") + why);
    leon_fasta_split_result R{};
    *res = R;
    CallStream st;
    if (const int rc = dev_open("leon_fasta_split_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    OwnBuf d_cnt, d_first, d_nl, d_in, d_off, d_why, d_rec, d_found, d_tmp;
    size_t tmp_bytes = 0;
    // every '\n' of the text, in order (as leon_fastq_split_device finds them)
    const uint64_t n_tiles = n_text ? (((uintptr_t)d_text & 15) + n_text + FASTQ_TILE - 1) / FASTQ_TILE : 0;
    const uint64_t per = std::max<uint64_t>((n_tiles + FASTQ_MAX_GROUPS - 1) / FASTQ_MAX_GROUPS, 1), groups = (n_tiles + per - 1) / per;
    uint32_t n_nl32 = 0;
    uint8_t first_byte = '>', last_byte = '\n';
    if (n_tiles) {
        DEVCHK(d_cnt.ensure((n_tiles + 1) * sizeof(uint32_t))); DEVCHK(d_first.ensure((n_tiles + 1) * sizeof(uint32_t)));
        DEVCHK(hipMemsetAsync(d_cnt.as<uint32_t>() + n_tiles, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_fq_newlines<false>, dim3((uint32_t)groups), dim3(FQ_THREADS), 0, s, d_text, n_text, n_tiles, per, d_cnt.as<uint32_t>(), nullptr, 0);
        DEVCHK(hipGetLastError());
        DEVCHK(fq_count_scan(nullptr, tmp_bytes, d_cnt.as<uint32_t>(), d_first.as<uint32_t>(), n_tiles + 1, s));
        DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        DEVCHK(fq_count_scan(d_tmp.p, tmp_bytes, d_cnt.as<uint32_t>(), d_first.as<uint32_t>(), n_tiles + 1, s));
        DEVCHK(hipMemcpyAsync(&n_nl32, d_first.as<uint32_t>() + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        DEVCHK(hipMemcpyAsync(&first_byte, d_text, 1, hipMemcpyDeviceToHost, s));
        DEVCHK(hipMemcpyAsync(&last_byte, d_text + n_text - 1, 1, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
    }
    const uint64_t n_nl = std::min<uint64_t>(n_nl32, n_text);
    DEVCHK(d_nl.ensure((n_nl + 1) * sizeof(uint32_t)));
    if (n_nl) {
        hipLaunchKernelGGL(k_fq_newlines<true>, dim3((uint32_t)groups), dim3(FQ_THREADS), 0, s, d_text, n_text, n_tiles, per, d_first.as<uint32_t>(), d_nl.as<uint32_t>(), n_nl);
        DEVCHK(hipGetLastError());
    }
    // the lines, their scan, the records
    const uint64_t n_lines = n_nl + (n_text && last_byte != '\n' ? 1 : 0);
    DEVCHK(d_in.ensure((n_lines + 1) * sizeof(FaSum))); DEVCHK(d_off.ensure((n_lines + 1) * sizeof(FaSum)));
    DEVCHK(d_why.ensure(n_lines + 1)); DEVCHK(d_rec.ensure((n_lines + 2) * sizeof(FaRec)));
    DEVCHK(d_found.ensure(sizeof(FaFound)));
    DEVCHK(hipMemsetAsync(d_found.p, 0xFF, offsetof(FaFound, n_headers), s));
    DEVCHK(hipMemsetAsync(d_found.as<uint8_t>() + offsetof(FaFound, n_headers), 0, sizeof(FaFound) - offsetof(FaFound, n_headers), s));
    const dim3 line_grid((uint32_t)((n_lines + 1 + 255) / 256));
    hipLaunchKernelGGL(k_fa_lines, line_grid, dim3(256), 0, s, d_text, n_text, d_nl.as<uint32_t>(), n_nl, n_lines, last ? 1 : 0, wrap, d_in.as<FaSum>(), d_why.as<uint8_t>());
    DEVCHK(hipGetLastError());
    DEVCHK(fa_sum_scan(nullptr, tmp_bytes, d_in.as<FaSum>(), d_off.as<FaSum>(), n_lines + 1, s));
    DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    DEVCHK(fa_sum_scan(d_tmp.p, tmp_bytes, d_in.as<FaSum>(), d_off.as<FaSum>(), n_lines + 1, s));
    hipLaunchKernelGGL(k_fa_heads, line_grid, dim3(256), 0, s, d_nl.as<uint32_t>(), n_nl, n_text, n_lines, last ? 1 : 0, max_records, d_in.as<FaSum>(), d_off.as<FaSum>(),
                       d_why.as<uint8_t>(), d_rec.as<FaRec>(), d_found.as<FaFound>());
    DEVCHK(hipGetLastError());
    FaFound F;
    DEVCHK(hipMemcpyAsync(&F, d_found.p, sizeof F, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    const uint64_t n_headers = std::min<uint64_t>(F.n_headers, n_lines);
    const uint64_t whole = last ? n_headers : n_headers ? n_headers - 1 : 0, rec_n = std::min(whole, max_records);
    const bool no_header = n_text && first_byte != '>';          // the text does not begin with a header line: record 0 is what lies in front of the first
    R.n_records = no_header ? 0 : std::min<uint64_t>(F.first_bad_rec, rec_n);
    if (R.n_records == max_records) R.stop = LEON_FASTA_MAX;
    else if (no_header) { R.stop = LEON_FASTA_IRREGULAR; R.reason = LEON_FASTA_R_HEADER; }
    else if (R.n_records < rec_n) { R.stop = LEON_FASTA_IRREGULAR; R.reason = (uint32_t)(F.first_bad_line & 255); }
    else R.stop = LEON_FASTA_END;
    // totals, where the split ends, where the record behind it ends
    const uint64_t n = R.n_records;
    FaRec at[2];
    DEVCHK(hipMemcpyAsync(at, d_rec.as<FaRec>() + n, sizeof at, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    if (!no_header) {
        R.consumed = std::min<uint64_t>(at[0].begin, n_text); R.header_bytes = at[0].hdr; R.base_bytes = at[0].base;
        if (R.stop == LEON_FASTA_IRREGULAR) R.next_header = std::min<uint64_t>(at[1].begin, n_text);
    } else if (R.stop == LEON_FASTA_IRREGULAR) R.next_header = std::min<uint64_t>(at[0].begin, n_text);
    const bool fits = n + 1 <= records_cap && R.header_bytes <= bytes_cap && R.base_bytes <= bytes_cap;
    hipLaunchKernelGGL(k_fa_offsets, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, s, d_rec.as<FaRec>(), n, fits ? 1 : 0, d_header_off, d_base_off, d_found.as<FaFound>());
    DEVCHK(hipGetLastError());
    const uint64_t n_split_lines = n ? std::min<uint64_t>(at[0].line, n_lines) : 0;
    if (fits && n_split_lines) {
        hipLaunchKernelGGL(k_fa_split, dim3((uint32_t)((n_split_lines * FA_LANES + 255) / 256)), dim3(256), 0, s, d_text, n_text, d_nl.as<uint32_t>(), n_nl, d_in.as<FaSum>(),
                           d_off.as<FaSum>(), n_split_lines, d_headers, d_bases);
        DEVCHK(hipGetLastError());
    }
    // (the longest one-line record comes back with the wait for the split: no synchronising read-back of its own)
    DEVCHK(hipMemcpyAsync(&F.single_max, d_found.as<uint8_t>() + offsetof(FaFound, single_max), sizeof F.single_max, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    R.single_max = F.single_max;
    *res = R;
    if (!fits)
        return dev_fail(LEON_E_OVERFLOW, "leon_fasta_split_device: " + std::to_string(n) + " records need " + std::to_string(R.header_bytes) + " header bytes, " +
                                             std::to_string(R.base_bytes) + " bases and " + std::to_string(n + 1) + " table entries");
    return LEON_OK;
}
