// letters_kernels.hip -- what the DNA coder cannot carry, found and put back where the bases lie (`-c -letters`).
//
// For a buffer of bases b[0..n):  a RUN is a maximal interval of bytes in 'a'..'z';  an ODD byte is one that, folded to upper case
// when it is lower-case, is none of A C G T N;  the FOLDED buffer holds upper(b) where that is one of A C G T N and 'N' elsewhere.
//   k_letters_count  a workgroup of 256 walks K consecutive 4 KiB tiles (cut at 16-byte aligned ADDRESSES, as k_crc32_tiles): a lane
//                    loads 16 bytes and forms a 16-bit lower-case mask and a 16-bit odd mask.  A position starts a run when it is
//                    lower-case and the byte before it is not: that bit comes from the lane before (a ballot of the lanes' last
//                    bits), the wave before (LDS), the tile before (a register) or, for the workgroup's first byte, from the buffer
//                    itself -- this kernel writes nothing, so every byte is still the original.  Per workgroup: the run starts, the
//                    odd bytes, and that first bit (`before`).
//   k_letters_scan   one workgroup: the exclusive prefix over the workgroups' totals, and the totals.
//   k_letters_take   the masks again; starts, ends (a position that is not lower-case behind one that is; position n counts) and odd
//                    bytes ranked by a wave scan plus an LDS prefix over the four waves, carried from tile to tile; runs[2k],
//                    runs[2k+1], odd_pos, odd_byte stored; the folded 16 bytes written back by the lanes whose masks are not zero.
//                    It folds IN PLACE, so it never looks at a byte outside its own tiles: the workgroup's first bit is the one
//                    k_letters_count recorded.  The k-th start and the k-th end belong to one run: the ends' first rank is the
//                    starts' first rank minus one where a run is open at the workgroup's first byte.
//   k_letters_case   per tile two uniform binary searches in runs (the first run that ends behind the tile's first byte, the first
//                    that begins at or behind its end): equal = nothing to do, no byte loaded; else every lane looks through that
//                    range for its 16 bytes and sets bit 0x20 of the bytes in 'A'..'Z' inside a run.
//   k_letters_odd    a thread per record: the original byte back in its place (after k_letters_case, on the same stream).
// Bounds: a 16-byte load or store is made only by a lane whose 16 bytes lie whole inside [0, n); every other byte is touched alone
// after its position was tested.  The tables are indexed below the counts the launch was given.
#include "kernels.h"
#include "device_call.h"

#include <algorithm>
#include <string>

namespace leon {

// host_streams.cpp: what both forms of apply refuse, in the same words; nullptr = the tables are in order
const char* letters_tables_refusal(const uint8_t* bases, uint64_t n_bytes, const uint64_t* runs, uint64_t n_runs, const uint64_t* odd_pos,
                                   const uint8_t* odd_byte, uint64_t n_odd);

namespace {

constexpr uint32_t LT_TILE = 4096, LT_THREADS = 256;
typedef unsigned long long ull;

__device__ __forceinline__ bool lt_is_lower(uint32_t b) { return b - 'a' < 26u; }
__device__ __forceinline__ uint64_t lt_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// the lane's 16 bytes at position p0 (a multiple of 16 as an address) into w; the mask of those that lie inside [0, n)
__device__ __forceinline__ uint32_t lt_load16(const uint8_t* __restrict__ bytes, int64_t p0, uint64_t n, uint32_t w[4]) {
    if (p0 >= 0 && (uint64_t)p0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(bytes + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return 0xFFFFu;
    }
    uint32_t valid = 0;
    w[0] = w[1] = w[2] = w[3] = 0;
    for (uint32_t j = 0; j < 16; j++) {
        const int64_t pj = p0 + j;
        if (pj < 0 || (uint64_t)pj >= n) continue;
        w[j >> 2] |= (uint32_t)bytes[pj] << (8 * (j & 3));
        valid |= 1u << j;
    }
    return valid;
}

// bit j of low: byte j is in 'a'..'z'; of odd: its upper-case form is none of A C G T N.  Bytes outside `valid` have neither.
__device__ __forceinline__ void lt_masks(const uint32_t w[4], uint32_t valid, uint32_t& low, uint32_t& odd) {
    low = 0; odd = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        const uint32_t l = lt_is_lower(b) ? 1u : 0u;
        const uint32_t i = b - (l ? 'a' : 'A');
        const uint32_t base = i < 26u ? (0x82045u >> i) & 1u : 0u;       // A C G N T
        low |= l << j;
        odd |= (base ^ 1u) << j;
    }
    low &= valid; odd &= valid;
}

// The lower-case bit of the byte in front of the lane's 16: the lane before, the wave before, or `carry` (the tile before).  Holds a
// barrier: called by all 256.  carry becomes the bit of the tile's last byte.  s_hi: one of two halves, the caller alternates them
// (a wave may write the next tile's word while another still reads this tile's).
__device__ __forceinline__ uint32_t lt_prev_bit(uint32_t low, ull* s_hi, uint32_t& carry) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const ull hi = __ballot((low >> 15) & 1u);
    if (lane == 0) s_hi[wave] = hi;
    __syncthreads();
    const uint32_t prev = lane ? (uint32_t)(hi >> (lane - 1)) & 1u : wave ? (uint32_t)(s_hi[wave - 1] >> 63) : carry;
    carry = (uint32_t)(s_hi[3] >> 63);
    return prev;
}

__global__ __launch_bounds__(256) void k_letters_count(const uint8_t* __restrict__ bytes, uint64_t n, uint64_t n_tiles, uint64_t tiles_per_group,
                                                       ull* __restrict__ cnt, uint32_t* __restrict__ before) {
    __shared__ ull s_hi[2][4];
    __shared__ ull s_red[4][2];
    const uint32_t t = threadIdx.x;
    const int64_t origin = -(int64_t)((uintptr_t)bytes & 15);    // position of tile 0's first byte
    const uint64_t tile0 = blockIdx.x * tiles_per_group;
    const int64_t first = origin + (int64_t)(tile0 * LT_TILE);
    uint32_t carry = first > 0 && (uint64_t)(first - 1) < n ? (lt_is_lower(bytes[first - 1]) ? 1u : 0u) : 0u;
    if (t == 0) before[blockIdx.x] = carry;
    ull n_start = 0, n_odd = 0;
    uint32_t par = 0;
    for (uint64_t k = 0; k < tiles_per_group; k++, par ^= 1) {
        const uint64_t tile = tile0 + k;
        if (tile >= n_tiles) break;
        const int64_t p0 = origin + (int64_t)(tile * LT_TILE) + (int64_t)(t * 16u);
        uint32_t w[4], low, odd;
        const uint32_t valid = lt_load16(bytes, p0, n, w);
        lt_masks(w, valid, low, odd);
        const uint32_t prev = lt_prev_bit(low, s_hi[par], carry);
        n_start += __popc(low & ~((low << 1) | prev));
        n_odd += __popc(odd);
    }
    for (int d = 32; d; d >>= 1) { n_start += __shfl_xor(n_start, d); n_odd += __shfl_xor(n_odd, d); }
    if ((t & 63u) == 0) { s_red[t >> 6][0] = n_start; s_red[t >> 6][1] = n_odd; }
    __syncthreads();
    if (t == 0) {
        cnt[2 * (uint64_t)blockIdx.x] = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
        cnt[2 * (uint64_t)blockIdx.x + 1] = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
    }
}

// base[2 g], base[2 g + 1]: the run starts and odd bytes in front of workgroup g; total[0..2): all of them
__global__ __launch_bounds__(256) void k_letters_scan(const ull* __restrict__ cnt, uint32_t groups, ull* __restrict__ base, ull* __restrict__ total) {
    __shared__ ull s[256][2];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (groups + 255u) / 256u;
    const uint32_t a = t * chunk < groups ? t * chunk : groups, b = a + chunk < groups ? a + chunk : groups;
    ull s0 = 0, s1 = 0;
    for (uint32_t g = a; g < b; g++) { s0 += cnt[2 * g]; s1 += cnt[2 * g + 1]; }
    s[t][0] = s0; s[t][1] = s1;
    __syncthreads();
    if (t == 0) {
        ull a0 = 0, a1 = 0;
        for (uint32_t i = 0; i < 256; i++) { const ull x0 = s[i][0], x1 = s[i][1]; s[i][0] = a0; s[i][1] = a1; a0 += x0; a1 += x1; }
        total[0] = a0; total[1] = a1;
    }
    __syncthreads();
    s0 = s[t][0]; s1 = s[t][1];
    for (uint32_t g = a; g < b; g++) { base[2 * g] = s0; base[2 * g + 1] = s1; s0 += cnt[2 * g]; s1 += cnt[2 * g + 1]; }
}

__global__ __launch_bounds__(256) void k_letters_take(uint8_t* __restrict__ bytes, uint64_t n, uint64_t n_tiles, uint64_t tiles_per_group,
                                                      const ull* __restrict__ base, const uint32_t* __restrict__ before,
                                                      uint64_t* __restrict__ runs, uint64_t n_runs, uint64_t* __restrict__ odd_pos,
                                                      uint8_t* __restrict__ odd_byte, uint64_t n_odd) {
    __shared__ ull s_hi[2][4];
    __shared__ uint32_t s_tot[4][3];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const int64_t origin = -(int64_t)((uintptr_t)bytes & 15);
    const uint64_t tile0 = blockIdx.x * tiles_per_group;
    uint32_t carry = before[blockIdx.x];                         // (recorded while every byte was the original: the neighbour may be folded by now)
    // the ranks of the next start, end and odd byte (uniform)
    uint64_t run_s = base[2 * (uint64_t)blockIdx.x], run_e = run_s - carry, run_o = base[2 * (uint64_t)blockIdx.x + 1];
    uint32_t par = 0;
    for (uint64_t k = 0; k < tiles_per_group; k++, par ^= 1) {
        const uint64_t tile = tile0 + k;
        if (tile >= n_tiles) break;
        const int64_t p0 = origin + (int64_t)(tile * LT_TILE) + (int64_t)(t * 16u);
        uint32_t w[4], low, odd;
        const uint32_t valid = lt_load16(bytes, p0, n, w);
        lt_masks(w, valid, low, odd);
        const uint32_t carry_in = carry;
        const uint32_t prev = lt_prev_bit(low, s_hi[par], carry);
        const uint32_t behind = ((low << 1) | prev) & 0xFFFFu;  // bit j: the byte in front of byte j is lower-case
        const uint32_t starts = low & ~behind;
        // an end is the position behind a run's last byte: position n is one (its `low` bit is 0), nothing behind it is
        const uint32_t ends = behind & ~low;
        if (!__syncthreads_or((int)(low | odd)) && !carry_in) continue;   // (uniform) the usual tile: nothing to rank, nothing to fold
        const uint32_t cs = __popc(starts), ce = __popc(ends), co = __popc(odd);
        uint32_t se = cs | (ce << 16), o = co;                    // inclusive scans over the wave: at most 1 024 per field
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t a = __shfl_up(se, d), b = __shfl_up(o, d);
            if (lane >= d) { se += a; o += b; }
        }
        if (lane == 63) { s_tot[wave][0] = se & 0xFFFFu; s_tot[wave][1] = se >> 16; s_tot[wave][2] = o; }
        __syncthreads();                                          // (the next write of s_tot lies behind the next tile's first barrier)
        uint32_t ws = 0, we = 0, wo = 0, ts = 0, te = 0, to = 0;
        for (uint32_t v = 0; v < 4; v++) {
            if (v < wave) { ws += s_tot[v][0]; we += s_tot[v][1]; wo += s_tot[v][2]; }
            ts += s_tot[v][0]; te += s_tot[v][1]; to += s_tot[v][2];
        }
        uint64_t rs = run_s + ws + (se & 0xFFFFu) - cs, re = run_e + we + (se >> 16) - ce, ro = run_o + wo + o - co;
        run_s += ts; run_e += te; run_o += to;
        for (uint32_t m = starts; m; m &= m - 1, rs++)
            if (rs < n_runs) runs[2 * rs] = (uint64_t)(p0 + (__ffs(m) - 1));
        for (uint32_t m = ends; m; m &= m - 1, re++)
            if (re < n_runs) runs[2 * re + 1] = (uint64_t)(p0 + (__ffs(m) - 1));
        for (uint32_t m = odd; m; m &= m - 1, ro++) {
            const uint32_t j = __ffs(m) - 1;
            if (ro < n_odd) { odd_pos[ro] = (uint64_t)(p0 + j); odd_byte[ro] = (uint8_t)(w[j >> 2] >> (8 * (j & 3))); }
        }
        const uint32_t change = low | odd;
        if (!change) continue;
        uint32_t f[4] = {w[0], w[1], w[2], w[3]};
        for (uint32_t m = change; m; m &= m - 1) {
            const uint32_t j = __ffs(m) - 1, sh = 8 * (j & 3);
            const uint32_t b = (w[j >> 2] >> sh) & 255u;
            const uint32_t nb = (odd >> j) & 1u ? (uint32_t)'N' : b - 32u;
            f[j >> 2] = (f[j >> 2] & ~(255u << sh)) | (nb << sh);
        }
        if (valid == 0xFFFFu) *reinterpret_cast<uint4*>(bytes + p0) = make_uint4(f[0], f[1], f[2], f[3]);
        else
            for (uint32_t m = change; m; m &= m - 1) { const uint32_t j = __ffs(m) - 1; bytes[p0 + j] = (uint8_t)(f[j >> 2] >> (8 * (j & 3))); }   // (change lies inside valid)
    }
}

// the first run of [lo, hi) that ends behind pos (hi: none)
__device__ __forceinline__ uint64_t lt_first_end_behind(const uint64_t* __restrict__ runs, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (runs[2 * mid + 1] > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// the first run of [lo, hi) that begins at or behind pos (hi: none)
__device__ __forceinline__ uint64_t lt_first_begin_from(const uint64_t* __restrict__ runs, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (runs[2 * mid] >= pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_letters_case(uint8_t* __restrict__ bytes, uint64_t n, uint64_t n_tiles, uint64_t tiles_per_group,
                                                      const uint64_t* __restrict__ runs, uint64_t n_runs) {
    const uint32_t t = threadIdx.x;
    const int64_t origin = -(int64_t)((uintptr_t)bytes & 15);
    for (uint64_t k = 0; k < tiles_per_group; k++) {
        const uint64_t tile = blockIdx.x * tiles_per_group + k;
        if (tile >= n_tiles) break;
        const int64_t t0 = origin + (int64_t)(tile * LT_TILE);
        const uint64_t lo = t0 < 0 ? 0 : (uint64_t)t0, hi = lt_min((uint64_t)(t0 + LT_TILE), n);
        if (lo >= hi) continue;
        const uint64_t ra = lt_first_end_behind(runs, 0, n_runs, lo), rb = lt_first_begin_from(runs, ra, n_runs, hi);   // (uniform)
        if (ra == rb) continue;                                   // no run touches the tile: not a byte of it is loaded
        const int64_t p0 = t0 + (int64_t)(t * 16u);
        const uint64_t c0 = p0 < (int64_t)lo ? lo : (uint64_t)p0, c1 = lt_min((uint64_t)(p0 + 16), hi);
        if (c0 >= c1) continue;
        uint32_t in_run = 0;
        for (uint64_t r = lt_first_end_behind(runs, ra, rb, c0); r < rb; r++) {
            const uint64_t b = runs[2 * r], e = runs[2 * r + 1];
            if (b >= c1) break;
            const uint32_t j0 = (uint32_t)((int64_t)(b > c0 ? b : c0) - p0), j1 = (uint32_t)((int64_t)(e < c1 ? e : c1) - p0);   // 0 <= j0 < j1 <= 16
            in_run |= ((1u << j1) - 1u) & ~((1u << j0) - 1u);
        }
        if (!in_run) continue;
        uint32_t w[4];
        const uint32_t valid = lt_load16(bytes, p0, n, w);
        uint32_t change = 0;
        for (uint32_t m = in_run & valid; m; m &= m - 1) {
            const uint32_t j = __ffs(m) - 1, sh = 8 * (j & 3);
            if (((w[j >> 2] >> sh) & 255u) - 'A' < 26u) { w[j >> 2] |= 0x20u << sh; change |= 1u << j; }
        }
        if (!change) continue;
        if (valid == 0xFFFFu) *reinterpret_cast<uint4*>(bytes + p0) = make_uint4(w[0], w[1], w[2], w[3]);
        else
            for (uint32_t m = change; m; m &= m - 1) { const uint32_t j = __ffs(m) - 1; bytes[p0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3))); }
    }
}

__global__ __launch_bounds__(256) void k_letters_odd(uint8_t* __restrict__ bytes, uint64_t n, const uint64_t* __restrict__ odd_pos,
                                                     const uint8_t* __restrict__ odd_byte, uint64_t n_odd) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_odd; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = odd_pos[i];
        if (p < n) bytes[p] = odd_byte[i];
    }
}

// the tiles of n bytes at d: `extra` = 1 covers position n too (the end of a run that reaches the last byte lies there)
struct Tiles { uint64_t n_tiles, per; uint32_t groups; };
Tiles lt_tiles(const uint8_t* d, uint64_t n, uint32_t extra) {
    const uint64_t lead = (uint64_t)((uintptr_t)d & 15);
    Tiles T;
    T.n_tiles = (lead + n + extra + LT_TILE - 1) / LT_TILE;
    T.per = (T.n_tiles + LETTERS_MAX_GROUPS - 1) / LETTERS_MAX_GROUPS;
    T.groups = (uint32_t)((T.n_tiles + T.per - 1) / T.per);
    return T;
}

// k_letters_count and k_letters_scan over the buffer: the totals to the host, the per-workgroup words left on the device for take
struct Counted { OwnBuf cnt, before, base, total; Tiles T; uint64_t totals[2] = {0, 0}; };
int lt_count(hipStream_t s, const uint8_t* d_bases, uint64_t n_bytes, Counted& C) {
    C.T = lt_tiles(d_bases, n_bytes, 1);
    DEVCHK(C.cnt.ensure(C.T.groups * 16ull)); DEVCHK(C.before.ensure(C.T.groups * 4ull)); DEVCHK(C.base.ensure(C.T.groups * 16ull)); DEVCHK(C.total.ensure(16));
    hipLaunchKernelGGL(k_letters_count, dim3(C.T.groups), dim3(LT_THREADS), 0, s, d_bases, n_bytes, C.T.n_tiles, C.T.per, C.cnt.as<ull>(), C.before.as<uint32_t>());
    DEVCHK(hipGetLastError());
    hipLaunchKernelGGL(k_letters_scan, dim3(1), dim3(256), 0, s, C.cnt.as<ull>(), C.T.groups, C.base.as<ull>(), C.total.as<ull>());
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpyAsync(C.totals, C.total.p, 16, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}

}  // namespace
}  // namespace leon

using namespace leon;

extern "C" {

int leon_letters_count_device(int device_id, const uint8_t* d_bases, uint64_t n_bytes, uint64_t* n_runs, uint64_t* n_odd) {
    if (!n_runs || !n_odd || (n_bytes && !d_bases)) return dev_fail(LEON_E_INVALID, "letters: null argument");
    if (n_bytes >> 62) return dev_fail(LEON_E_INVALID, "letters: implausible sizes");
    *n_runs = *n_odd = 0;
    if (!n_bytes) return LEON_OK;
    CallStream st;
    if (const int rc = dev_open("leon_letters_count_device", device_id, st)) return rc;
    Counted C;
    if (const int rc = lt_count(st.s, d_bases, n_bytes, C)) return rc;
    *n_runs = C.totals[0]; *n_odd = C.totals[1];
    return LEON_OK;
}

int leon_letters_take_device(int device_id, uint8_t* d_bases, uint64_t n_bytes, uint64_t* runs, uint64_t n_runs, uint64_t* odd_pos, uint8_t* odd_byte,
                             uint64_t n_odd) {
    if ((n_bytes && !d_bases) || (n_runs && !runs) || (n_odd && (!odd_pos || !odd_byte))) return dev_fail(LEON_E_INVALID, "letters: null argument");
    if ((n_bytes >> 62) || (n_runs >> 58) || (n_odd >> 58)) return dev_fail(LEON_E_INVALID, "letters: implausible sizes");
    auto differs = [&](uint64_t r, uint64_t x) {
        return dev_fail(LEON_E_STATE, "letters: the buffer holds " + std::to_string(r) + " run(s) and " + std::to_string(x) + " other byte(s), not the " +
                                         std::to_string(n_runs) + " and " + std::to_string(n_odd) + " the tables were sized for");
    };
    if (!n_bytes) return n_runs || n_odd ? differs(0, 0) : LEON_OK;
    CallStream st;
    if (const int rc = dev_open("leon_letters_take_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    Counted C;
    if (const int rc = lt_count(s, d_bases, n_bytes, C)) return rc;
    if (C.totals[0] != n_runs || C.totals[1] != n_odd) return differs(C.totals[0], C.totals[1]);      // (nothing was written so far)
    if (!n_runs && !n_odd) return LEON_OK;                        // the bytes are their own folded form
    OwnBuf d_runs, d_pos, d_byte;
    // (at least 8 bytes each: a kernel argument is never null, even for an empty table)
    DEVCHK(d_runs.ensure(std::max<uint64_t>(n_runs * 16, 8))); DEVCHK(d_pos.ensure(std::max<uint64_t>(n_odd * 8, 8))); DEVCHK(d_byte.ensure(std::max<uint64_t>(n_odd, 8)));
    hipLaunchKernelGGL(k_letters_take, dim3(C.T.groups), dim3(LT_THREADS), 0, s, d_bases, n_bytes, C.T.n_tiles, C.T.per, C.base.as<ull>(), C.before.as<uint32_t>(),
                       d_runs.as<uint64_t>(), n_runs, d_pos.as<uint64_t>(), d_byte.as<uint8_t>(), n_odd);
    DEVCHK(hipGetLastError());
    if (n_runs) DEVCHK(hipMemcpyAsync(runs, d_runs.p, n_runs * 16, hipMemcpyDeviceToHost, s));
    if (n_odd) { DEVCHK(hipMemcpyAsync(odd_pos, d_pos.p, n_odd * 8, hipMemcpyDeviceToHost, s)); DEVCHK(hipMemcpyAsync(odd_byte, d_byte.p, n_odd, hipMemcpyDeviceToHost, s)); }
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}

int leon_letters_apply_device(int device_id, uint8_t* d_bases, uint64_t n_bytes, const uint64_t* runs, uint64_t n_runs, const uint64_t* odd_pos,
                              const uint8_t* odd_byte, uint64_t n_odd) {
    if (const char* why = letters_tables_refusal(d_bases, n_bytes, runs, n_runs, odd_pos, odd_byte, n_odd)) return dev_fail(LEON_E_INVALID, why);
    if (!n_bytes || (!n_runs && !n_odd)) return LEON_OK;
    CallStream st;
    if (const int rc = dev_open("leon_letters_apply_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    OwnBuf d_runs, d_pos, d_byte;
    if (n_runs) {
        DEVCHK(d_runs.ensure(n_runs * 16));
        DEVCHK(hipMemcpyAsync(d_runs.p, runs, n_runs * 16, hipMemcpyHostToDevice, s));
        const Tiles T = lt_tiles(d_bases, n_bytes, 0);
        hipLaunchKernelGGL(k_letters_case, dim3(T.groups), dim3(LT_THREADS), 0, s, d_bases, n_bytes, T.n_tiles, T.per, d_runs.as<uint64_t>(), n_runs);
        DEVCHK(hipGetLastError());
    }
    if (n_odd) {
        DEVCHK(d_pos.ensure(n_odd * 8)); DEVCHK(d_byte.ensure(n_odd));
        DEVCHK(hipMemcpyAsync(d_pos.p, odd_pos, n_odd * 8, hipMemcpyHostToDevice, s));
        DEVCHK(hipMemcpyAsync(d_byte.p, odd_byte, n_odd, hipMemcpyHostToDevice, s));
        const uint32_t groups = (uint32_t)std::min<uint64_t>((n_odd + 255) / 256, LETTERS_MAX_GROUPS);
        hipLaunchKernelGGL(k_letters_odd, dim3(groups), dim3(256), 0, s, d_bases, n_bytes, d_pos.as<uint64_t>(), d_byte.as<uint8_t>(), n_odd);
        DEVCHK(hipGetLastError());
    }
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}

}  // extern "C"
