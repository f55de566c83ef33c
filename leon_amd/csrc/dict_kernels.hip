// dict_kernels.hip -- the anchor dictionary as independently coded pieces, coded and decoded on the device.
// A piece is P anchors through a fresh 5-symbol Order0Model and a fresh coder, with the 8 flush bytes (host_dict_pieces.h is the
// host form and the verdict).  LANE = PIECE: 64 chains per wave, a wave per workgroup, the grid capped and walked with a loop.
//   * inside a piece the model's total at symbol t is 5 + t whatever the data, so it is the same number in every lane: its
//     reciprocal floor((2^64 - 1) / total) is made once per 64 steps -- lane l divides for step t0 + l, off the chains -- and handed
//     to the wave with a readlane per step; the quotient is rc_coder_tile's truncated multiply-high with its 32-bit fix-up;
//   * the model is four counts in registers; there is no LDS, no modeler wave, no barrier.
// Totals stay below 5 + 63 * 2^20 < 2^26 (P <= 2^20), far below RC_MAX_TOTAL: no exact-division path.
#include "kernels.h"
#include "rc_model.h"
#include "prim.h"
#include "staging.h"
#include "host_dict_pieces.h"
#include "device_call.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace leon {
namespace {

constexpr uint64_t DP_TOP = 1ull << 56;

__device__ inline uint64_t dp_lane64(uint64_t v, uint32_t l) {           // l is wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// floor(range / tot) with b = floor((2^64 - 1) / tot), tot < 2^26.  With M = floor(range * b / 2^64): b * tot >= 2^64 - tot gives
// range * b / 2^64 > range / tot - 1, so M >= Q - 1 (Q the quotient); the estimate below leaves out r0 * b0 and the carries of the two
// middle products' low halves, three fractions below 1 each: qe >= M - 2 >= Q - 3 and qe <= Q.  The true remainder range - qe * tot
// is then below 4 * tot < 2^28, so its low 32 bits are all of it and three compares give what the estimate was short by.
__device__ inline uint64_t dp_quot(uint64_t range, uint32_t tot, uint64_t b) {
    const uint32_t r0 = (uint32_t)range, r1 = (uint32_t)(range >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    uint64_t qe = (uint64_t)r1 * b1 + __umulhi(r1, b0);
    qe += __umulhi(r0, b1);
    const uint32_t rem = r0 - (uint32_t)qe * tot;
    const uint32_t t2 = tot << 1, t3 = t2 + tot;
    return qe + ((rem >= tot ? 1u : 0u) + (rem >= t2 ? 1u : 0u) + (rem >= t3 ? 1u : 0u));
}

// Piece p's bytes go to scratch[p * stride .. + stride).  Nothing is ever stored outside that slot: the usual step's 4-byte store
// is clamped to the slot's last four bytes and the byte stores of the rare path and of the flush are dropped from `stride` on.  A
// clamped store may overwrite bytes of the slot that were right, so a piece whose size comes within 4 bytes of the stride counts
// as overflowed (*err = 1; the byte count only grows, so every clamped store ends there) and the caller codes again with a wider
// stride.  8 bytes per symbol plus 12 is the widest it asks for: a step shifts at most 64 bits out (AnchorDictCoder::encode_records
// reserves the same), the flush is 8 bytes and the test keeps 4 back.
template <uint32_t W>
__global__ void __launch_bounds__(64) k_dict_encode_pieces(const uint64_t* __restrict__ kmers, uint64_t n_anchors, uint32_t k, uint32_t P,
                                                           uint64_t n_pieces, uint8_t* __restrict__ scratch, uint64_t stride,
                                                           uint64_t* __restrict__ sizes, int* err) {
    const uint32_t lane = threadIdx.x;
    const uint64_t cap = stride, cap4 = stride - 4;                        // (stride >= 64: launch_dict_encode_pieces)
    for (uint64_t base = blockIdx.x * 64ull; base < n_pieces; base += gridDim.x * 64ull) {
        const uint64_t p = base + lane;
        const bool mine = p < n_pieces;                                    // lanes past n_pieces run the wave's steps and do nothing in them
        const uint64_t a0 = mine ? p * P : 0;
        const uint32_t na = mine ? (uint32_t)(n_anchors - a0 < P ? n_anchors - a0 : P) : 0u;
        const uint32_t na_wave = (uint32_t)(n_anchors - base * P < P ? n_anchors - base * P : P);   // lane 0's piece: none of the wave is longer
        uint8_t* const dst = scratch + (mine ? p : 0) * stride;
        uint64_t low = 0, range = ~0ull, nout = 0, inv = 0;
        uint32_t c0 = 1, c1 = 1, c2 = 1;                                   // Order0Model::clear: the counts of A, C, T (G's and N's are never asked for)
        uint32_t t = 0;
        for (uint32_t a = 0; a < na_wave; a++) {
            const bool live = a < na;                                      // a lane of the last, partial piece stops early
            uint64_t w0 = 0, w1 = 0;
            if (live) { w0 = kmers[(a0 + a) * W]; if (W == 2) w1 = kmers[(a0 + a) * W + 1]; }
            for (uint32_t j = 0; j < k; j++, t++) {
                if ((t & 63u) == 0) inv = ~0ull / (uint64_t)(5u + t + lane);      // every lane, for the step t + lane
                const uint64_t b = dp_lane64(inv, t & 63u);
                const uint32_t tot = 5u + t;
                if (!live) continue;
                // symbol j of the anchor, first base in the highest bits (k_anchor_symbols)
                const uint32_t bit = 2u * (k - 1u - j);
                const uint32_t c = (uint32_t)((W == 2 && bit >= 64u ? w1 : w0) >> (bit & 63u)) & 3u;
                const uint32_t lo = (c > 0 ? c0 : 0u) + (c > 1 ? c1 : 0u) + (c > 2 ? c2 : 0u);
                const uint32_t fr = c == 0 ? c0 : c == 1 ? c1 : c == 2 ? c2 : tot - 1u - c0 - c1 - c2;      // (N keeps its count of 1)
                const uint64_t q = dp_quot(range, tot, b);
                low += q * lo;
                range = q * fr;
                c0 += c == 0; c1 += c == 1; c2 += c == 2;
                // RangeEncoder::encode's loop.  Usual case: low and low + range agree on their top 0..3 bytes and the shifted range stays
                // >= BOTTOM: those bytes leave at once with one 4-byte store at the cursor (what lies past it is overwritten later)
                const uint32_t lh = (uint32_t)(low >> 32);
                const uint32_t xh = lh ^ (uint32_t)((low + range) >> 32);
                const uint32_t sh = xh ? ((uint32_t)__builtin_clz(xh) & 24u) : 0u;
                if (xh != 0u && ((range << sh) >> 48) != 0) {
                    *(uint32_t*)(dst + (nout < cap4 ? nout : cap4)) = __builtin_bswap32(lh);
                    low <<= sh; range <<= sh; nout += sh >> 3;
                } else {
                    // rare: four bytes or more leave, or the range is below BOTTOM -- the loop as it is written
                    while ((low ^ (low + range)) < DP_TOP || (range < RC_BOTTOM && ((range = (0 - low) & (RC_BOTTOM - 1)), true))) {
                        if (nout < cap) dst[nout] = (uint8_t)(low >> 56);
                        nout++;
                        range <<= 8;
                        low <<= 8;
                    }
                }
            }
        }
        if (mine) {
            for (uint32_t i = 0; i < 8; i++) {                             // RangeEncoder::flush
                if (nout < cap) dst[nout] = (uint8_t)(low >> 56);
                nout++;
                low <<= 8;
            }
            sizes[p] = nout;
            if (nout > cap4) *err = 1;
        }
    }
}

// the slots back to back: piece p's bytes to dst[off[p] .. off[p + 1]) (off = the exclusive sums of sizes)
__global__ void __launch_bounds__(256) k_dict_gather_pieces(const uint8_t* __restrict__ scratch, uint64_t stride, const uint64_t* __restrict__ off,
                                                            uint64_t n_pieces, uint8_t* __restrict__ dst) {
    for (uint64_t p = blockIdx.y; p < n_pieces; p += gridDim.y) {
        const uint8_t* src = scratch + p * stride;
        uint8_t* d = dst + off[p];
        uint64_t n = off[p + 1] - off[p];
        if (n > stride) n = stride;                                        // (never: the caller gathers only when no piece overflowed)
        for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) d[i] = src[i];
    }
}

// The inverse: decode_anchor_dict's plain step (host_rc.h) per lane.  Piece p's bytes are payload[off[p] .. off[p + 1]): byte i of the
// piece is loaded only when i < its size, zeros stand in from there on as on the host, and a piece that asks for more than 16 bytes
// past its end is refused -- so is r == 0 and a fifth symbol.  A refused piece sets bad[p] and its lane does nothing more.
template <uint32_t W>
__global__ void __launch_bounds__(64) k_dict_decode_pieces(const uint8_t* __restrict__ payload, const uint64_t* __restrict__ off, uint64_t n_pieces,
                                                           uint64_t n_anchors, uint32_t k, uint32_t P, uint64_t* __restrict__ out,
                                                           uint32_t* __restrict__ bad) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t base = blockIdx.x * 64ull; base < n_pieces; base += gridDim.x * 64ull) {
        const uint64_t p = base + lane;
        const bool mine = p < n_pieces;
        const uint64_t a0 = mine ? p * P : 0;
        const uint32_t na = mine ? (uint32_t)(n_anchors - a0 < P ? n_anchors - a0 : P) : 0u;
        const uint32_t na_wave = (uint32_t)(n_anchors - base * P < P ? n_anchors - base * P : P);
        const uint64_t begin = mine ? off[p] : 0, n = mine ? off[p + 1] - begin : 0;
        const uint8_t* const src = payload + begin;
        uint64_t low = 0, range = ~0ull, code = 0, i = 0, inv = 0;
        for (; i < 8; i++) code = (code << 8) | (i < n ? src[i] : 0u);
        uint64_t m1 = 1, m2 = 2, m3 = 3, m4 = 4;                          // the model's cumulative counts below C, T, G, N
        uint32_t t = 0;
        bool failed = false;
        for (uint32_t a = 0; a < na_wave; a++) {
            uint64_t km0 = 0, km1 = 0;
            for (uint32_t j = 0; j < k; j++, t++) {
                if ((t & 63u) == 0) inv = ~0ull / (uint64_t)(5u + t + lane);
                const uint64_t b = dp_lane64(inv, t & 63u);
                const uint32_t tot = 5u + t;
                if (a >= na || failed) continue;
                const uint64_t r = dp_quot(range, tot, b);
                if (r == 0) { failed = true; continue; }
                const uint64_t d = code - low;
                const uint64_t p1 = r * m1, p2 = r * m2, p3 = r * m3, p4 = r * m4;
                const bool g1 = d >= p1, g2 = d >= p2, g3 = d >= p3;
                if (d >= p4) { failed = true; continue; }                   // an N inside an anchor
                const uint32_t c = (uint32_t)g1 + (uint32_t)g2 + (uint32_t)g3;
                low += g3 ? p3 : g2 ? p2 : g1 ? p1 : 0;
                range = g3 ? p4 - p3 : g2 ? p3 - p2 : g1 ? p2 - p1 : p1;
                while ((low ^ (low + range)) < DP_TOP || (range < RC_BOTTOM && ((range = (0 - low) & (RC_BOTTOM - 1)), true))) {
                    code = (code << 8) | (i < n ? src[i] : 0u);
                    i++;
                    range <<= 8;
                    low <<= 8;
                    if (i > n + 16) { failed = true; break; }              // far past the end (a range of 0 would spin here)
                }
                if (failed) continue;
                m1 += c < 1; m2 += c < 2; m3 += c < 3; m4 += 1;
                if (W == 2) km1 = (km1 << 2) | (km0 >> 62);
                km0 = (km0 << 2) | c;
                if (j == k - 1u) {
                    out[(a0 + a) * W] = km0;
                    if (W == 2) out[(a0 + a) * W + 1] = km1;
                }
            }
        }
        if (mine && failed) bad[p] = 1;
    }
}

inline uint32_t dp_groups(uint64_t n_pieces) {
    const uint64_t waves = (n_pieces + 63) / 64;
    return (uint32_t)(waves < DICT_PIECES_MAX_GROUPS ? waves : DICT_PIECES_MAX_GROUPS);
}

// piece p = anchors [p * P, min((p + 1) * P, n_anchors)) of kmers, coded into scratch[p * stride .. + stride) (stride >= 64), sizes[p] its
// bytes; *err (zeroed by the caller) is set when a piece came within 4 bytes of its stride: code again with a wider one
void launch_dict_encode_pieces(hipStream_t s, const uint64_t* kmers, uint64_t n_anchors, uint32_t k, uint32_t P, uint64_t n_pieces, uint8_t* scratch,
                               uint64_t stride, uint64_t* sizes, int* err) {
    if (!n_pieces || stride < 64) return;
    if (k >= 32) hipLaunchKernelGGL(k_dict_encode_pieces<2>, dim3(dp_groups(n_pieces)), dim3(64), 0, s, kmers, n_anchors, k, P, n_pieces, scratch, stride, sizes, err);
    else hipLaunchKernelGGL(k_dict_encode_pieces<1>, dim3(dp_groups(n_pieces)), dim3(64), 0, s, kmers, n_anchors, k, P, n_pieces, scratch, stride, sizes, err);
}

// the slots back to back: off[n_pieces + 1] = the exclusive sums of sizes
void launch_dict_gather_pieces(hipStream_t s, const uint8_t* scratch, uint64_t stride, const uint64_t* off, uint64_t n_pieces, uint8_t* dst) {
    if (!n_pieces) return;
    const uint32_t gy = n_pieces > 65535 ? 65535u : (uint32_t)n_pieces;
    hipLaunchKernelGGL(k_dict_gather_pieces, dim3(4, gy), dim3(256), 0, s, scratch, stride, off, n_pieces, dst);
}

// piece p = payload[off[p] .. off[p + 1]) -> its anchors' k-mer words in out; bad[p] (zeroed by the caller) is set for a piece that does not decode
void launch_dict_decode_pieces(hipStream_t s, const uint8_t* payload, const uint64_t* off, uint64_t n_pieces, uint64_t n_anchors, uint32_t k, uint32_t P,
                               uint64_t* out, uint32_t* bad) {
    if (!n_pieces) return;
    if (k >= 32) hipLaunchKernelGGL(k_dict_decode_pieces<2>, dim3(dp_groups(n_pieces)), dim3(64), 0, s, payload, off, n_pieces, n_anchors, k, P, out, bad);
    else hipLaunchKernelGGL(k_dict_decode_pieces<1>, dim3(dp_groups(n_pieces)), dim3(64), 0, s, payload, off, n_pieces, n_anchors, k, P, out, bad);
}

}  // namespace

// The pieces of d_kmers coded on stream s: piece_off (host, n_pieces + 1 entries) and the stream's bytes, back to back, in d_dst.
// A piece's slot is first P * k / 2 + 64 bytes, twice what a genomic dictionary needs (2 bits a base); a list that does not fit --
// nothing but adversarial k-mers -- is coded again with 8 bytes per symbol, the most a step can shift out (k_dict_encode_pieces).
// LEON_OK, or the code with `why`: leon_dna_finish (capi.hip) keeps it with its context, the stateless call below with the thread.
int dict_pieces_code(hipStream_t s, const uint64_t* d_kmers, uint64_t n_anchors, uint32_t k, uint32_t P, uint64_t* piece_off, OwnBuf& d_dst, std::string& why) {
#define PIECES_CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { why = hip_failure(#call, e_); return LEON_E_HIP; } } while (0)
    const uint64_t n_pieces = dict_piece_count(n_anchors, P);
    piece_off[0] = 0;
    if (!n_pieces) return LEON_OK;
    const uint64_t piece_syms = (uint64_t)std::min<uint64_t>(P, n_anchors) * k;
    OwnBuf d_scratch, d_sizes, d_off, d_err, d_tmp;
    PIECES_CHK(d_sizes.ensure((n_pieces + 1) * 8)); PIECES_CHK(d_off.ensure((n_pieces + 1) * 8)); PIECES_CHK(d_err.ensure(4));
    PIECES_CHK(hipMemsetAsync((uint64_t*)d_sizes.p + n_pieces, 0, 8, s));
    uint64_t stride = 0;
    for (int wide = 0;; wide++) {
        stride = ((wide ? 8 * piece_syms + 12 : piece_syms / 2 + 64) + 7) & ~7ull;
        PIECES_CHK(d_scratch.ensure(n_pieces * stride));
        PIECES_CHK(hipMemsetAsync(d_err.p, 0, 4, s));
        launch_dict_encode_pieces(s, d_kmers, n_anchors, k, P, n_pieces, d_scratch.as<uint8_t>(), stride, d_sizes.as<uint64_t>(), d_err.as<int>());
        PIECES_CHK(hipGetLastError());
        int err = 0;
        PIECES_CHK(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, s));
        PIECES_CHK(hipStreamSynchronize(s));
        if (!err) break;
        if (wide) { why = "anchor dictionary pieces: a piece outgrew 8 bytes per symbol (internal error)"; return LEON_E_OVERFLOW; }
    }
    size_t tmp_bytes = 0;
    PIECES_CHK(prim::ExclusiveSum(nullptr, tmp_bytes, d_sizes.as<uint64_t>(), d_off.as<uint64_t>(), n_pieces + 1, s));
    PIECES_CHK(d_tmp.ensure(tmp_bytes + 16));
    PIECES_CHK(prim::ExclusiveSum(d_tmp.p, tmp_bytes, d_sizes.as<uint64_t>(), d_off.as<uint64_t>(), n_pieces + 1, s));
    PIECES_CHK(hipMemcpyAsync(piece_off, d_off.p, (n_pieces + 1) * 8, hipMemcpyDeviceToHost, s));
    PIECES_CHK(hipStreamSynchronize(s));
    PIECES_CHK(d_dst.ensure(piece_off[n_pieces] + 16));
    launch_dict_gather_pieces(s, d_scratch.as<uint8_t>(), stride, d_off.as<uint64_t>(), n_pieces, d_dst.as<uint8_t>());
    PIECES_CHK(hipGetLastError());
    PIECES_CHK(hipStreamSynchronize(s));
    return LEON_OK;
#undef PIECES_CHK
}

}  // namespace leon

using namespace leon;

extern "C" int leon_anchor_dict_encode_pieces_device(int device_id, const uint64_t* d_kmers, uint64_t n_anchors, uint32_t k, uint32_t piece_anchors, uint8_t* out,
                                          uint64_t out_cap, uint64_t* piece_off, uint64_t* size) {
    if (const char* why = dict_pieces_encode_refusal(d_kmers, n_anchors, k, piece_anchors, out, out_cap, piece_off, size)) return dev_fail(LEON_E_INVALID, why);
    const uint32_t P = dict_piece_anchors(piece_anchors);
    *size = 0; piece_off[0] = 0;
    if (!n_anchors) return LEON_OK;                               // no piece: no device is asked
    CallStream st;
    if (const int rc = dev_open("leon_anchor_dict_encode_pieces_device", device_id, st)) return rc;
    OwnBuf d_dst;
    std::string why;
    if (const int rc = dict_pieces_code(st.s, d_kmers, n_anchors, k, P, piece_off, d_dst, why)) return dev_fail(rc, why);
    *size = piece_off[dict_piece_count(n_anchors, P)];
    if (*size > out_cap) return dev_fail(LEON_E_OVERFLOW, "anchor dictionary pieces: out_cap too small");
    DEVCHK(hipMemcpyAsync(out, d_dst.p, *size, hipMemcpyDeviceToHost, st.s));
    DEVCHK(hipStreamSynchronize(st.s));
    return LEON_OK;
}

extern "C" int leon_anchor_dict_decode_pieces_device(int device_id, const uint8_t* payload, const uint64_t* piece_off, uint64_t n_pieces, uint64_t n_anchors, uint32_t k,
                                          uint32_t piece_anchors, uint64_t* out_kmers) {
    if (const char* why = dict_pieces_decode_refusal(payload, piece_off, n_pieces, n_anchors, k, piece_anchors, out_kmers)) return dev_fail(LEON_E_INVALID, why);
    if (!n_pieces) return LEON_OK;                                // no piece: no device is asked
    const uint32_t P = dict_piece_anchors(piece_anchors), W = kmer_words(k);
    CallStream st;
    if (const int rc = dev_open("leon_anchor_dict_decode_pieces_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    // the pieces' bytes alone travel: [piece_off[0], piece_off[n_pieces]), the offsets rebased to them
    const uint64_t first = piece_off[0], bytes = piece_off[n_pieces] - first;
    std::vector<uint64_t> rel(n_pieces + 1);
    for (uint64_t p = 0; p <= n_pieces; p++) rel[p] = piece_off[p] - first;
    OwnBuf d_pay, d_off, d_out, d_bad;
    DEVCHK(d_pay.ensure(bytes + 16)); DEVCHK(d_off.ensure((n_pieces + 1) * 8));
    DEVCHK(d_out.ensure(n_anchors * W * 8)); DEVCHK(d_bad.ensure(n_pieces * 4));
    if (bytes && staged_h2d(device_id, d_pay.p, payload + first, bytes) != hipSuccess) { (void)hipGetLastError(); return dev_fail(LEON_E_HIP, "leon_anchor_dict_decode_pieces_device: the pieces' copy to the device failed"); }
    DEVCHK(hipMemcpyAsync(d_off.p, rel.data(), (n_pieces + 1) * 8, hipMemcpyHostToDevice, s));
    DEVCHK(hipMemsetAsync(d_bad.p, 0, n_pieces * 4, s));
    launch_dict_decode_pieces(s, d_pay.as<uint8_t>(), d_off.as<uint64_t>(), n_pieces, n_anchors, k, P, d_out.as<uint64_t>(), d_bad.as<uint32_t>());
    DEVCHK(hipGetLastError());
    std::vector<uint32_t> bad(n_pieces);
    DEVCHK(hipMemcpyAsync(bad.data(), d_bad.p, n_pieces * 4, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    for (uint64_t p = 0; p < n_pieces; p++) if (bad[p]) return dev_fail(LEON_E_INVALID, dict_piece_refusal(p));
    DEVCHK(hipMemcpyAsync(out_kmers, d_out.p, n_anchors * W * 8, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}

// host-only: the dictionary stream of a list of anchors (what the worker thread produces); no GPU involved
extern "C" int leon_host_anchor_dict_encode(const uint64_t* kmers, uint64_t n, uint32_t k, uint8_t* out, uint64_t out_cap, uint64_t* size) {
    if ((!kmers && n) || !size || k < 1 || k > 63) return LEON_E_INVALID;
    // the same worker (chain thread + reciprocal helper thread) the contexts use, fed in a few batches
    AnchorDictWorker worker(k);
    const uint32_t W = kmer_words(k);
    const uint64_t step = std::max<uint64_t>(1, n / 3);
    for (uint64_t i = 0; i < n; i += step) {
        const uint64_t m = std::min(step, n - i);
        worker.push(std::vector<uint64_t>(kmers + i * W, kmers + (i + m) * W));
    }
    worker.drain();
    AnchorDictCoder& coder = worker.coder();
    coder.flush();
    *size = coder.size();
    if (coder.size() > out_cap) return LEON_E_OVERFLOW;
    if (out) memcpy(out, coder.data(), coder.size());
    return LEON_OK;
}

extern "C" int leon_host_anchor_dict_decode(const uint8_t* payload, uint64_t size, uint64_t n_anchors, uint32_t k, uint64_t* out) {
    if ((!payload && size) || (!out && n_anchors)) return dev_fail(LEON_E_INVALID, "null argument");
    if (k < 3 || k > 63) return dev_fail(LEON_E_INVALID, "kmer_size must be in 3..63");
    if (!decode_anchor_dict(payload, size, n_anchors, k, out)) return dev_fail(LEON_E_INVALID, "anchor dictionary stream does not decode");
    return LEON_OK;
}

extern "C" int leon_host_anchor_dict_encode_pieces(const uint64_t* kmers, uint64_t n_anchors, uint32_t k, uint32_t piece_anchors, uint8_t* out, uint64_t out_cap,
                                        uint64_t* piece_off, uint64_t* size, uint32_t n_threads) {
    std::string why;
    const int rc = host_dict_encode_pieces(kmers, n_anchors, k, piece_anchors, out, out_cap, piece_off, size, n_threads, why);
    return rc ? dev_fail(rc, why) : LEON_OK;
}
extern "C" int leon_host_anchor_dict_decode_pieces(const uint8_t* payload, const uint64_t* piece_off, uint64_t n_pieces, uint64_t n_anchors, uint32_t k,
                                        uint32_t piece_anchors, uint64_t* out_kmers, uint32_t n_threads) {
    std::string why;
    const int rc = host_dict_decode_pieces(payload, piece_off, n_pieces, n_anchors, k, piece_anchors, out_kmers, n_threads, why);
    return rc ? dev_fail(rc, why) : LEON_OK;
}
