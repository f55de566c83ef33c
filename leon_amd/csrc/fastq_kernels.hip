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
#include "kernels.h"
#include "prim.h"
#include "device_call.h"
#include "host_fastq.h"

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
