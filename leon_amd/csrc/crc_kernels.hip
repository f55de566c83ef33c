// crc_kernels.hip -- zlib's CRC-32 of many segments of one device buffer (leon_crc32_segments_device).
//
// With raw(M) = the CRC register run over M from 0 without the final XOR, and (*) = multiplication mod P of the reflected form:
//     raw(A | B) = raw(A) (*) x^(8 |B|)  ^  raw(B)                       crc32(M) = raw(M) ^ (0xFFFFFFFF (*) x^(8 |M|)) ^ 0xFFFFFFFF
// so a segment's raw is the XOR, over any cut of its bytes into pieces, of raw(piece) (*) x^(8 * bytes of the segment behind the piece).
//   k_crc32_tiles   a workgroup of 256 walks K consecutive 4 KiB tiles (cut at 16-byte aligned ADDRESSES).  A tile that lies inside one
//                   segment: a lane loads 16 bytes, forms their raw from 16 look-up tables in LDS (slicing), multiplies it by
//                   x^(8 * bytes of the tile behind it) and the workgroup XORs the products: the tile's raw.  Thread 0 carries it
//                   through the segment (acc = acc (*) x^(8 * 4096) ^ tile) and, when the segment or the workgroup's tiles end, issues
//                   ONE atomicXor of acc (*) x^(8 * bytes of the segment behind) into the segment's word.
//                   Any other tile (a segment boundary inside, or the buffer's first and last tile): byte-wise, every lane for
//                   the segments its 16 bytes touch, an atomicXor per (lane, segment) that has bytes.
//   k_crc32_final   a thread per segment: the initial value's term and the final XOR.
// XOR atomics on integers: the words do not depend on the order of arrival; nothing waits for anything.
#include "kernels.h"
#include "device_call.h"

#include <cstring>

namespace leon {

// host_streams.cpp: what both forms refuse, in the same words; nullptr = the segments are in order
const char* crc32_segments_refusal(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, const uint32_t* crc);

namespace {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_TILE = 4096, CRC_THREADS = 256;

// a (*) b: bit 31 is the coefficient of x^0 (zlib's multmodp, without its early exit)
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; i++) {
        p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & CRC_POLY);
    }
    return p;
}

struct CrcPow {
    uint32_t x2n[64];           // x^(8 * 2^j)
    uint32_t lane[256];         // x^(8 * 16 * i): what lies behind the lane that has i lanes of the tile after it
    constexpr CrcPow() : x2n(), lane() {
        uint32_t p = 0x80000000u >> 8;
        for (int j = 0; j < 64; j++) { x2n[j] = p; p = crc_mul(p, p); }
        lane[0] = 0x80000000u;
        for (int i = 1; i < 256; i++) lane[i] = crc_mul(lane[i - 1], x2n[4]);
    }
};
constexpr CrcPow kPowHost{};
__constant__ CrcPow kPow = kPowHost;
constexpr uint32_t CRC_XTILE = kPowHost.x2n[12];                  // x^(8 * 4096)
static_assert(crc_mul(kPowHost.lane[255], kPowHost.x2n[4]) == CRC_XTILE, "256 lanes of 16 bytes are a tile");

// x^(8 n)
__device__ __forceinline__ uint32_t crc_xpow8(uint64_t n) {
    uint32_t r = 0x80000000u;
    for (uint32_t j = 0; n; j++, n >>= 1)
        if (n & 1) r = crc_mul(r, kPow.x2n[j]);
    return r;
}

// the last s with off[s] <= pos (pos in [off[0], off[n_seg])): the segment that holds byte pos
__device__ __forceinline__ uint64_t crc_seg_of(const uint64_t* __restrict__ off, uint64_t n_seg, uint64_t pos) {
    uint64_t lo = 0, hi = n_seg;                                  // off[lo] <= pos < off[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

// Bounds: bytes is read at [off[0], off[n_seg]) only -- a 16-byte load is made by a lane of a tile that lies whole inside that range,
// every other byte is loaded alone after its position was tested; off is indexed up to n_seg, acc below n_seg.
__global__ __launch_bounds__(256) void k_crc32_tiles(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n_seg,
                                                     uint64_t n_tiles, uint64_t tiles_per_group, uint32_t* __restrict__ acc) {
    __shared__ uint32_t s_T[16][256];                             // s_T[k][b] = raw(b, then k zero bytes)
    __shared__ uint32_t s_red[2][4];
    const uint32_t t = threadIdx.x;
    {
        uint32_t c = t;
        for (int i = 0; i < 8; i++) c = (c >> 1) ^ ((0u - (c & 1u)) & CRC_POLY);
        s_T[0][t] = c;
        __syncthreads();
        for (int k = 1; k < 16; k++) { c = s_T[0][c & 255u] ^ (c >> 8); s_T[k][t] = c; }
        __syncthreads();
    }
    // this lane's factor, times x^0 .. x^31: the products below are 32 selects and XORs
    uint32_t bx[32];
    {
        uint32_t b = kPow.lane[255 - t];
#pragma unroll
        for (int i = 0; i < 32; i++) { bx[i] = b; b = (b >> 1) ^ ((0u - (b & 1u)) & CRC_POLY); }
    }
    const uint64_t lo = off[0], hi = off[n_seg];
    const int64_t origin = (int64_t)lo - (int64_t)((uintptr_t)(bytes + lo) & 15);          // position of tile 0's first byte (may lie before lo)
    // thread 0: the raw of the bytes [.., cur_end) of segment cur_seg that this workgroup has seen and not yet issued
    bool cur = false;
    uint64_t cur_seg = 0, cur_end = 0;
    uint32_t cur_acc = 0;
    auto flush = [&] {
        if (t == 0 && cur && cur_acc) atomicXor(&acc[cur_seg], crc_mul(cur_acc, crc_xpow8(off[cur_seg + 1] - cur_end)));
        cur = false;
    };
    uint64_t seg = 0, seg_end = 0;                                // uniform: the segment the last tile began in (seg_end == 0: none yet)
    uint32_t par = 0;                                             // which half of s_red the next whole tile uses: thread 0 reads one half
                                                                  // while the other waves may already write the next tile's
    for (uint64_t k = 0; k < tiles_per_group; k++) {
        const uint64_t tile = blockIdx.x * tiles_per_group + k;
        if (tile >= n_tiles) break;
        const int64_t t0 = origin + (int64_t)(tile * CRC_TILE), t1 = t0 + CRC_TILE;
        const bool whole = t0 >= (int64_t)lo && t1 <= (int64_t)hi;
        const uint64_t first = whole ? (uint64_t)t0 : (uint64_t)(t0 < (int64_t)lo ? (int64_t)lo : t0);    // the tile's first byte of the range
        if (!(seg_end > first && off[seg] <= first)) { seg = crc_seg_of(off, n_seg, first); seg_end = off[seg + 1]; }
        if (whole && seg_end >= (uint64_t)t1) {
            const uint4 v = *reinterpret_cast<const uint4*>(bytes + (uint64_t)t0 + t * 16u);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t r = 0;
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) r ^= s_T[15 - j][(w[j >> 2] >> (8 * (j & 3))) & 255u];
            uint32_t p = 0;
#pragma unroll
            for (int i = 0; i < 32; i++) p ^= (uint32_t)((int32_t)(r << i) >> 31) & bx[i];
            for (int d = 32; d; d >>= 1) p ^= __shfl_xor(p, d);
            if ((t & 63) == 0) s_red[par][t >> 6] = p;
            __syncthreads();                                      // (uniform: the branch depends on the tile alone)
            if (t == 0) {
                const uint32_t* q = s_red[par];
                const uint32_t tr = q[0] ^ q[1] ^ q[2] ^ q[3];
                if (cur && cur_seg == seg) cur_acc = crc_mul(cur_acc, CRC_XTILE) ^ tr;
                else { flush(); cur = true; cur_seg = seg; cur_acc = tr; }
                cur_end = (uint64_t)t1;
            }
            par ^= 1;
        } else {
            flush();
            // byte-wise: the lane's bytes of the range, segment by segment
            const int64_t p0 = t0 + (int64_t)(t * 16u);
            bool have = false;
            uint64_t s = 0, s_end = 0;
            uint32_t r = 0;
            for (uint32_t j = 0; j < 16; j++) {
                const int64_t pj = p0 + j;
                if (pj < (int64_t)lo || pj >= (int64_t)hi) continue;
                const uint64_t pos = (uint64_t)pj;
                if (!s_end) { s = crc_seg_of(off, n_seg, pos); s_end = off[s + 1]; }
                while (pos >= s_end) {                            // (have: the segment ends at pos, nothing of it lies behind)
                    if (have && r) atomicXor(&acc[s], r);
                    have = false; r = 0;
                    s++; s_end = off[s + 1];
                }
                r = s_T[0][(r ^ bytes[pos]) & 255u] ^ (r >> 8);
                have = true;
                if (j == 15 || pos + 1 == hi) {
                    if (r) atomicXor(&acc[s], crc_mul(r, crc_xpow8(s_end - (pos + 1))));
                    have = false;
                }
            }
        }
    }
    flush();
}

__global__ __launch_bounds__(256) void k_crc32_final(const uint64_t* __restrict__ off, uint64_t n_seg, uint32_t* __restrict__ acc) {
    const uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    acc[s] ^= crc_mul(0xFFFFFFFFu, crc_xpow8(off[s + 1] - off[s])) ^ 0xFFFFFFFFu;
}

}  // namespace

uint64_t crc32_tile_count(const uint8_t* bytes, uint64_t first, uint64_t last) {
    if (last <= first) return 0;
    const uint64_t lead = (uint64_t)((uintptr_t)(bytes + first) & 15);
    return (lead + (last - first) + CRC_TILE - 1) / CRC_TILE;
}

void launch_crc32_segments(hipStream_t s, const uint8_t* bytes, const uint64_t* off, uint64_t n_seg, uint64_t n_tiles, uint32_t* acc) {
    if (!n_seg) return;
    if (n_tiles) {
        const uint64_t per = (n_tiles + CRC32_MAX_GROUPS - 1) / CRC32_MAX_GROUPS;
        const uint64_t groups = (n_tiles + per - 1) / per;
        hipLaunchKernelGGL(k_crc32_tiles, dim3((uint32_t)groups), dim3(CRC_THREADS), 0, s, bytes, off, n_seg, n_tiles, per, acc);
    }
    hipLaunchKernelGGL(k_crc32_final, dim3((uint32_t)((n_seg + 255) / 256)), dim3(256), 0, s, off, n_seg, acc);
}

}  // namespace leon

using namespace leon;

extern "C" int leon_crc32_segments_device(int device_id, const uint8_t* d_bytes, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, uint32_t* crc) {
    if (const char* why = crc32_segments_refusal(d_bytes, n_bytes, seg_off, n_seg, crc)) return dev_fail(LEON_E_INVALID, why);
    if (!n_seg) return LEON_OK;
    const uint64_t n_tiles = crc32_tile_count(d_bytes, seg_off[0], seg_off[n_seg]);
    if (!n_tiles) { memset(crc, 0, n_seg * sizeof(uint32_t)); return LEON_OK; }      // nothing but empty segments: no device is asked
    CallStream st;
    if (const int rc = dev_open("leon_crc32_segments_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    OwnBuf d_off, d_acc;
    DEVCHK(d_off.ensure((n_seg + 1) * sizeof(uint64_t))); DEVCHK(d_acc.ensure(n_seg * sizeof(uint32_t)));
    DEVCHK(hipMemcpyAsync(d_off.p, seg_off, (n_seg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    DEVCHK(hipMemsetAsync(d_acc.p, 0, n_seg * sizeof(uint32_t), s));
    launch_crc32_segments(s, d_bytes, d_off.as<uint64_t>(), n_seg, n_tiles, d_acc.as<uint32_t>());
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpyAsync(crc, d_acc.p, n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}
