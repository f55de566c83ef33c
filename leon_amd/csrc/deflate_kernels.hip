// deflate_kernels.hip -- the quality stream's zlib blocks on the device (upstream deflates the block's
// buffered quality lines, Leon::writeBlockLena [RECALLED]).  One zlib stream per read block, as leon_host_qual_encode_blocks
// writes them, any inflate reads them; what differs is the encoder.  zlib's default strategy spends its time in hash chains
// looking for matches that quality strings rarely pay for (a three-byte match costs more bits than three literals of a 3-bit
// alphabet); what does pay is the run -- a quality value repeated -- and the entropy code.  So this is deflate with the RLE
// strategy (zlib's own Z_RLE: matches at distance 1 only) and dynamic Huffman codes per 32 KB of text, which needs no search
// and no serial parse: where a run starts and how long it is follows from comparing neighbours, every position knows from
// (run start, run length) alone which token starts at it, and the bit offsets are a prefix sum.
//   text -> chunks of DF_CHUNK bytes, one workgroup each, one deflate block each (dynamic codes, or stored when that is smaller),
//   closed on a byte boundary by an empty stored block (Z_SYNC_FLUSH's marker), so the chunks of a read block are concatenated
//   bytes; the read block's stream = 78 01, its chunks, a final empty stored block, Adler-32 (combined on the host from the
//   chunks' own).
#include "kernels.h"
#include "prim.h"
#include "staging.h"
#include "device_call.h"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

namespace leon {
// host_streams.cpp: what leon_text_bgzf_records_device and leon_host_bgzf_record_cuts both refuse, in the same words; nullptr = in order
const char* bgzf_records_refusal(bool have_off, uint64_t n_records, uint64_t n_head, uint64_t n_body, int last);
const char* bgzf_offsets_refusal(uint32_t flags);

namespace {

constexpr uint32_t DF_CHUNK = 32768;                         // text bytes per deflate block
constexpr uint32_t DF_T = 256;
constexpr uint32_t DF_PER = DF_CHUNK / DF_T;                  // consecutive positions per thread
constexpr uint32_t DF_OUT_STRIDE = DF_CHUNK + 64;             // bytes a chunk may write (stored form: text + 5)
constexpr uint32_t DF_NLIT = 286, DF_NCL = 19;
constexpr uint32_t DF_MAXSYM = 288;

// the quality lines of reads [r0, r1) each followed by '\n', as one text
__global__ void k_qual_text(const uint8_t* quals, const uint64_t* off, uint64_t n_reads, uint64_t q0, uint8_t* text) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n_reads; r += nwaves) {
        const uint64_t a = off[r] - q0, b = off[r + 1] - q0;
        uint8_t* d = text + a + r;
        for (uint64_t i = lane; i < b - a; i += 64) d[i] = quals[a + i];
        if (lane == 0) d[b - a] = '\n';
    }
}

__device__ const uint16_t df_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t df_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint8_t df_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ inline uint32_t df_len_code(uint32_t len) {        // 3..258 -> 0..28
    if (len == 258) return 28;
    const uint32_t l = len - 3;
    if (l < 8) return l;
    const uint32_t e = 29 - (uint32_t)__builtin_clz(l);       // extra bits: l in [2^(e+2), 2^(e+3))
    return 4 * e + 4 + ((l >> e) & 3u);
}
__device__ inline uint32_t df_rev(uint32_t code, uint32_t len) { return __builtin_bitreverse32(code) >> (32 - len); }

// Huffman code lengths of `n` symbols from their frequencies, none above `limit`, by the whole workgroup: the used symbols are
// ranked by (frequency, symbol) -- every thread counts the symbols before its own, broadcast reads, no sort -- then one lane runs
// Moffat & Katajainen's in-place algorithm over the ranked frequencies; when the depth exceeds the limit the frequencies are
// halved (rounded up) and it runs again (zlib moves the overflowing leaves instead; either gives a complete code).
// Scratch in LDS: A[n], order[n], fr2[n], ctl[2].
__device__ void df_code_lengths(const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* len, uint32_t* A, uint16_t* order, uint32_t* fr2, uint32_t* ctl) {
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < n; i += DF_T) { fr2[i] = freq[i]; len[i] = 0; }
    __syncthreads();
    for (;;) {
        if (t == 0) ctl[0] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += DF_T) {
            const uint32_t f = fr2[i];
            if (!f) continue;
            uint32_t r = 0;
            for (uint32_t j = 0; j < n; j++) { const uint32_t g = fr2[j]; r += (g && (g < f || (g == f && j < i))) ? 1u : 0u; }
            order[r] = (uint16_t)i; A[r] = f;
            atomicAdd(&ctl[0], 1u);
        }
        __syncthreads();
        if (t == 0) {
            const uint32_t m = ctl[0];
            uint32_t done = 1;
            if (m == 1) { const uint32_t i = order[0]; len[i] = 1; len[i ? i - 1 : 1] = 1; }   // one symbol: it and a neighbour get one bit each (inflate wants a complete code)
            else if (m >= 2) {
                A[0] += A[1];
                uint32_t root = 0, leaf = 2;
                for (uint32_t next = 1; next + 1 < m; next++) {
                    if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
                    if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
                }
                A[m - 2] = 0;
                for (int next = (int)m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
                int avbl = 1, usedn = 0, dpth = 0, rt = (int)m - 2, nx = (int)m - 1;
                while (avbl > 0) {
                    while (rt >= 0 && (int)A[rt] == dpth) { usedn++; rt--; }
                    while (avbl > usedn) { A[nx--] = (uint32_t)dpth; avbl--; }
                    avbl = 2 * usedn; dpth++; usedn = 0;
                }
                done = A[0] <= limit ? 1u : 0u;               // A[0]: the rarest symbol's length, the longest
            }
            ctl[1] = done | (m << 1);
        }
        __syncthreads();
        const uint32_t m = ctl[1] >> 1;
        if (ctl[1] & 1u) {
            if (m >= 2) for (uint32_t i = t; i < m; i += DF_T) len[order[i]] = (uint8_t)A[i];
            __syncthreads();
            return;
        }
        for (uint32_t i = t; i < n; i += DF_T) if (fr2[i]) fr2[i] = (fr2[i] + 1) >> 1;
        __syncthreads();
    }
}
// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream; cnt[16], nxt[16] in LDS
__device__ void df_codes(const uint8_t* len, uint32_t n, uint16_t* code, uint32_t* cnt, uint32_t* nxt) {
    const uint32_t t = threadIdx.x;
    if (t < 16) cnt[t] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n; i += DF_T) if (len[i]) atomicAdd(&cnt[len[i]], 1u);
    __syncthreads();
    if (t == 0) { uint32_t c = 0; nxt[0] = 0; for (uint32_t b = 1; b < 16; b++) { c = (c + cnt[b - 1]) << 1; nxt[b] = c; } }
    __syncthreads();
    for (uint32_t i = t; i < n; i += DF_T) {
        const uint32_t l = len[i];
        uint32_t r = 0;
        if (l) for (uint32_t j = 0; j < i; j++) r += len[j] == l ? 1u : 0u;
        code[i] = l ? (uint16_t)df_rev(nxt[l] + r, l) : (uint16_t)0;
    }
    __syncthreads();
}

struct BitW {                                                  // one lane's writer into a zeroed word buffer
    uint32_t* w; uint64_t pos;
    __device__ void put(uint32_t v, uint32_t nbits) {
        if (!nbits) return;
        const uint32_t i = (uint32_t)(pos >> 5), s = (uint32_t)(pos & 31);
        w[i] |= v << s;
        if (s + nbits > 32) w[i + 1] |= v >> (32 - s);
        pos += nbits;
    }
};

// The tokens of the positions [a, b] of one maximal run of equal bytes clipped to a thread's range: the run is [S, S + L) in the
// chunk.  RLE parse: the run's first byte is a literal; the R = L - 1 bytes after it are matches of 258 at distance 1, then one
// match of the remainder when it is 3 or more, else literals.  f(kind, length): kind 0 literal (length = count), 1 match.
template <typename F> __device__ inline void df_run_tokens(uint32_t S, uint32_t L, uint32_t a, uint32_t b, F f) {
    if (a == S) { f(0u, 1u); if (a == b) return; }
    const uint32_t R = L - 1, full = R / 258, rem = R - full * 258;
    const uint32_t ja = (a == S ? a + 1 : a) - (S + 1), jb = b - (S + 1);     // offsets into the R region, inclusive
    if (full) {                                                              // full matches start at j = 0, 258, ...: those with ja <= j <= jb
        const uint32_t first = (ja + 257) / 258, last = jb / 258;
        const uint32_t lastc = last < full - 1 ? last : full - 1;
        for (uint32_t i = first; i <= lastc && first <= lastc; i++) f(1u, 258u);
    }
    const uint32_t j0 = full * 258;                                          // the remainder region [j0, R)
    if (rem && jb >= j0) {
        if (rem >= 3) { if (ja <= j0) f(1u, rem); }
        else f(0u, (jb - (ja > j0 ? ja : j0)) + 1);
    }
}

// One chunk = one deflate block.  sizes[c] = bytes written at out + c * DF_OUT_STRIDE; adler[c] = Adler-32 of the chunk's text.
__global__ void __launch_bounds__(DF_T) k_deflate_chunks(const uint8_t* text, const uint64_t* chunk_begin, const uint32_t* chunk_len, uint64_t n_chunks,
                                                          uint8_t* out, uint32_t* sizes, uint32_t* adler) {
    __shared__ uint32_t textw[DF_CHUNK / 4 + 2];
    __shared__ uint32_t outw[DF_OUT_STRIDE / 4 + 4];
    __shared__ uint32_t freq[DF_MAXSYM], A[DF_MAXSYM], fr2[DF_MAXSYM], scan_sh[DF_T + 1], clfreq[DF_NCL];
    __shared__ uint16_t code[DF_MAXSYM], order[DF_MAXSYM], clcode[DF_NCL], hdr_sym[DF_MAXSYM + 8];
    __shared__ uint8_t len[DF_MAXSYM], cllen[DF_NCL], hdr_extra[DF_MAXSYM + 8];
    __shared__ uint8_t tfirst[DF_T], tlast[DF_T];
    __shared__ uint16_t tlead[DF_T], ttrail[DF_T], tn[DF_T];
    __shared__ uint32_t sh_misc[8], ctl[2], cnt16[16], nxt16[16];                               // 0 header bits, 1 total bits, 2 n header symbols, 3 hlit, 4 hclen
    uint8_t* const tb = (uint8_t*)textw;
    const uint32_t t = threadIdx.x;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t n = chunk_len[c];
        const uint8_t* src = text + chunk_begin[c];
        __syncthreads();
        for (uint32_t i = t; i < n; i += DF_T) tb[i] = src[i];
        for (uint32_t i = t; i < DF_OUT_STRIDE / 4 + 4; i += DF_T) outw[i] = 0;
        for (uint32_t i = t; i < DF_MAXSYM; i += DF_T) freq[i] = 0;
        if (t < DF_NCL) clfreq[t] = 0;
        __syncthreads();
        // ---- this thread's positions [p0, p1), their first / last byte, leading and trailing runs; Adler-32 partials ----
        const uint32_t p0 = t * DF_PER < n ? t * DF_PER : n, p1 = (t + 1) * DF_PER < n ? (t + 1) * DF_PER : n, cnt = p1 - p0;
        uint32_t lead = 0, trail = 0, sa = 0, sb = 0;
        if (cnt) {
            const uint8_t f0 = tb[p0], l0 = tb[p1 - 1];
            while (lead < cnt && tb[p0 + lead] == f0) lead++;
            while (trail < cnt && tb[p1 - 1 - trail] == l0) trail++;
            for (uint32_t i = 0; i < cnt; i++) { sa += tb[p0 + i]; sb += sa; }       // (128 * 255 and 128 * 129 / 2 * 255: no overflow)
            tfirst[t] = f0; tlast[t] = l0;
        }
        tlead[t] = (uint16_t)lead; ttrail[t] = (uint16_t)trail; tn[t] = (uint16_t)cnt;
        // Adler-32 over the chunk: A = 1 + sum of bytes, B = n + sum over bytes of (n - i) * byte = n + sum_t (sb_t + (n - p1_t) * sa_t)
        {
            uint64_t va = sa, vb = (uint64_t)sb + (uint64_t)(n - p1) * sa;
            for (uint32_t d = 32; d; d >>= 1) { va += __shfl_down((unsigned long long)va, d); vb += __shfl_down((unsigned long long)vb, d); }
            __syncthreads();
            if ((t & 63) == 0) { scan_sh[2 * (t >> 6)] = (uint32_t)(va % 65521u); scan_sh[2 * (t >> 6) + 1] = (uint32_t)(vb % 65521u); }
            __syncthreads();
            if (t == 0) {
                const uint32_t a32 = (1u + scan_sh[0] + scan_sh[2] + scan_sh[4] + scan_sh[6]) % 65521u;
                const uint32_t b32 = (uint32_t)(((uint64_t)n + scan_sh[1] + scan_sh[3] + scan_sh[5] + scan_sh[7]) % 65521u);
                adler[c] = (b32 << 16) | a32;
            }
        }
        __syncthreads();
        // how far the run at this thread's first position reaches back, how far the run at its last position reaches forward
        uint32_t back = 0, fwd = 0;
        if (cnt) {
            for (int q = (int)t - 1; q >= 0 && tn[q] && tlast[q] == tfirst[t]; q--) { back += ttrail[q]; if (ttrail[q] < tn[q]) break; }
            for (uint32_t q = t + 1; q < DF_T && tn[q] && tfirst[q] == tlast[t]; q++) { fwd += tlead[q]; if (tlead[q] < tn[q]) break; }
        }
        // every maximal local run [a, b] of this thread with its global start S and length L
        auto each_run = [&](auto g) {
            uint32_t a = p0;
            while (a < p1) {
                const uint8_t v = tb[a];
                uint32_t b = a;
                while (b + 1 < p1 && tb[b + 1] == v) b++;
                const uint32_t S = a == p0 ? a - back : a;
                const uint32_t E = b == p1 - 1 ? b + fwd : b;
                g(v, S, E - S + 1, a, b);
                a = b + 1;
            }
        };
        // ---- pass 1: symbol frequencies ----
        each_run([&](uint8_t v, uint32_t S, uint32_t L, uint32_t a, uint32_t b) {
            df_run_tokens(S, L, a, b, [&](uint32_t kind, uint32_t x) {
                if (kind == 0) atomicAdd(&freq[v], x);
                else atomicAdd(&freq[257 + df_len_code(x)], 1u);
            });
        });
        if (t == 0) atomicAdd(&freq[256], 1u);
        __syncthreads();
        // ---- the codes (the whole workgroup) and the block header (one lane) ----
        df_code_lengths(freq, DF_NLIT, 15, len, A, order, fr2, ctl);
        df_codes(len, DF_NLIT, code, cnt16, nxt16);
        if (t == 0) {
            uint32_t hlit = DF_NLIT;
            while (hlit > 257 && len[hlit - 1] == 0) hlit--;
            // lengths of the hlit literal/length codes, then two distance codes of one bit each (only code 0, distance 1, is ever used;
            // two make the distance code complete), run-length coded with the code-length alphabet (16: repeat, 17 / 18: zeros)
            uint32_t nh = 0;
            auto lens_at = [&](uint32_t i) -> uint32_t { return i < hlit ? len[i] : 1u; };
            const uint32_t total = hlit + 2;
            for (uint32_t i = 0; i < total;) {
                const uint32_t v = lens_at(i);
                uint32_t r = 1;
                while (i + r < total && lens_at(i + r) == v) r++;
                if (v == 0 && r >= 3) {
                    uint32_t left = r;
                    while (left >= 3) {
                        const uint32_t k = left > 138 ? 138 : left;
                        if (k >= 11) { hdr_sym[nh] = 18; hdr_extra[nh++] = (uint8_t)(k - 11); } else { hdr_sym[nh] = 17; hdr_extra[nh++] = (uint8_t)(k - 3); }
                        left -= k;
                    }
                    for (; left; left--) { hdr_sym[nh] = 0; hdr_extra[nh++] = 0; }
                } else if (v != 0 && r >= 4) {
                    hdr_sym[nh] = (uint16_t)v; hdr_extra[nh++] = 0;
                    uint32_t left = r - 1;
                    while (left >= 3) { const uint32_t k = left > 6 ? 6 : left; hdr_sym[nh] = 16; hdr_extra[nh++] = (uint8_t)(k - 3); left -= k; }
                    for (; left; left--) { hdr_sym[nh] = (uint16_t)v; hdr_extra[nh++] = 0; }
                } else {
                    for (uint32_t k = 0; k < r; k++) { hdr_sym[nh] = (uint16_t)v; hdr_extra[nh++] = 0; }
                }
                i += r;
            }
            for (uint32_t i = 0; i < nh; i++) clfreq[hdr_sym[i]]++;
            sh_misc[2] = nh; sh_misc[3] = hlit;
        }
        __syncthreads();
        df_code_lengths(clfreq, DF_NCL, 7, cllen, A, order, fr2, ctl);
        df_codes(cllen, DF_NCL, clcode, cnt16, nxt16);
        if (t == 0) {
            const uint32_t nh = sh_misc[2], hlit = sh_misc[3];
            uint32_t hclen = DF_NCL;
            while (hclen > 4 && cllen[df_cl_order[hclen - 1]] == 0) hclen--;
            BitW bw{outw, 0};
            bw.put(0u, 1); bw.put(2u, 2);                         // BFINAL 0, BTYPE 10
            bw.put(hlit - 257, 5); bw.put(2 - 1, 5); bw.put(hclen - 4, 4);
            for (uint32_t i = 0; i < hclen; i++) bw.put(cllen[df_cl_order[i]], 3);
            for (uint32_t i = 0; i < nh; i++) {
                const uint32_t s = hdr_sym[i];
                bw.put(clcode[s], cllen[s]);
                if (s == 16) bw.put(hdr_extra[i], 2); else if (s == 17) bw.put(hdr_extra[i], 3); else if (s == 18) bw.put(hdr_extra[i], 7);
            }
            sh_misc[0] = (uint32_t)bw.pos;
        }
        __syncthreads();
        // ---- pass 2: bits per thread, prefix sum ----
        uint32_t mybits = 0;
        each_run([&](uint8_t v, uint32_t S, uint32_t L, uint32_t a, uint32_t b) {
            df_run_tokens(S, L, a, b, [&](uint32_t kind, uint32_t x) {
                if (kind == 0) mybits += x * len[v];
                else { const uint32_t lc = df_len_code(x); mybits += len[257 + lc] + df_len_extra[lc] + 1u; }
            });
        });
        {
            uint32_t inc = mybits;
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d); if ((t & 63) >= d) inc += o; }
            if ((t & 63) == 63) scan_sh[t >> 6] = inc;
            __syncthreads();
            uint32_t base = sh_misc[0];
            for (uint32_t w = 0; w < (t >> 6); w++) base += scan_sh[w];
            if (t == DF_T - 1) sh_misc[1] = base + inc + len[256];              // body and end-of-block
            mybits = base + inc - mybits;                                      // this thread's first bit
        }
        __syncthreads();
        const uint32_t total_bits = sh_misc[1];
        // the block in its dynamic form + the empty stored block that closes it on a byte boundary: 3 bits, padding, 00 00 FF FF
        const uint32_t dyn_bytes = (total_bits + 3 + 7) / 8 + 4;
        const bool stored = dyn_bytes >= n + 5;
        uint8_t* dst = out + c * (uint64_t)DF_OUT_STRIDE;
        if (!stored) {
            // ---- pass 3: the tokens' bits ----
            uint64_t pos = mybits;
            auto put = [&](uint32_t v, uint32_t nbits) {                         // other lanes write the same words: atomic OR
                const uint32_t i = (uint32_t)(pos >> 5), s = (uint32_t)(pos & 31);
                atomicOr(&outw[i], v << s);
                if (s + nbits > 32) atomicOr(&outw[i + 1], v >> (32 - s));
                pos += nbits;
            };
            each_run([&](uint8_t v, uint32_t S, uint32_t L, uint32_t a, uint32_t b) {
                df_run_tokens(S, L, a, b, [&](uint32_t kind, uint32_t x) {
                    if (kind == 0) { for (uint32_t i = 0; i < x; i++) put(code[v], len[v]); }
                    else {
                        const uint32_t lc = df_len_code(x);
                        put(code[257 + lc], len[257 + lc]);
                        if (df_len_extra[lc]) put(x - df_len_base[lc], df_len_extra[lc]);
                        put(0u, 1);                                              // distance code 0 (distance 1): the one-bit code 0
                    }
                });
            });
            __syncthreads();
            if (t == 0) {
                BitW bw{outw, (uint64_t)total_bits - len[256]};
                bw.put(code[256], len[256]);
                bw.put(0u, 3);                                                   // BFINAL 0, BTYPE 00: the empty stored block
                bw.pos = (bw.pos + 7) & ~7ull;
                bw.put(0xFFFF0000u, 32);
                sizes[c] = (uint32_t)(bw.pos >> 3);
            }
            __syncthreads();
            const uint32_t nbytes = dyn_bytes;
            for (uint32_t i = t; i < (nbytes + 3) / 4; i += DF_T) ((uint32_t*)dst)[i] = outw[i];
        } else {
            if (t == 0) {
                dst[0] = 0; dst[1] = (uint8_t)n; dst[2] = (uint8_t)(n >> 8); dst[3] = (uint8_t)~n; dst[4] = (uint8_t)(~n >> 8);
                sizes[c] = n + 5;
            }
            for (uint32_t i = t; i < n; i += DF_T) dst[5 + i] = tb[i];
        }
    }
}

// ---- the same block with LZ77 matches, for record text (leon_text_bgzf_device_ex with LEON_BGZF_F_MATCHES) ----
// A header line repeats most of the one a record back, sequence fragments repeat too: text pays for a match search that qualities do
// not.  The parse of a chunk is a function of its bytes alone (tests/deflate_lz.py restates it):
//   candidates  in steps of DF_LZ_STEP positions, one per thread: every position with four bytes left reads table[hash of them] -- the
//               largest position of the steps before with that hash --, and after a barrier enters itself by atomicMax (so the order
//               does not matter).  A source inside the same step is not found; the run covers the common case of it.  The candidate
//               is compared with the text, at most 258 bytes and not past the chunk: another 4-gram of the same hash gives 0;
//   runs        as k_deflate_chunks: the bytes from p on equal to t[p - 1], at most 258, valid from 3, distance 1;
//   choice      the hash candidate when it has DF_LZ_MIN bytes and two more than the run, else the run, else a literal;
//   selection   greedy from position 0.  Every thread owns DF_PER positions and finds, backwards, for each of them the last token of
//               its range that a parse entering there takes (7 bits beside the 9 of the length); one lane chains the 256 ranges (a
//               token of 258 can skip two of them); every thread then walks forward from where the parse enters its range.
// The hash table lies in the words the block is written to later (zeroed in between); the distances, 64 KiB a chunk, do not fit in
// LDS beside text, lengths and output and lie in global memory, DF_CHUNK entries per workgroup of a grid of at most DF_LZ_MAX_GROUPS.
constexpr uint32_t DF_LZ_STEP = DF_T;
constexpr uint32_t DF_LZ_HASH_BITS = 13;
constexpr uint32_t DF_LZ_MIN = 5;                               // (4: 158 374, 5: 158 081, 6: 158 489 bytes on the suite's FASTQ)
constexpr uint32_t DF_LZ_MAX_GROUPS = 256;                      // one workgroup a CU; 16 MiB of distances
constexpr uint32_t DF_NDIST = 30;
constexpr uint32_t DF_LZ_NONE = 0xFFFFu;
static_assert(DF_PER == 128 && DF_CHUNK <= 32768, "a token's length (9 bits) and the last token of a range (7 bits) share 16 bits");
static_assert((1u << DF_LZ_HASH_BITS) <= DF_OUT_STRIDE / 4 + 4, "the hash table lies in the output words");

__device__ const uint16_t df_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
                                              12289, 16385, 24577};
__device__ inline uint32_t df_dist_code(uint32_t dist) {        // 1..32768 -> 0..29; code c has (c >> 1) - 1 extra bits from 4 on
    const uint32_t d = dist - 1;
    if (d < 4) return d;
    const uint32_t b = 31 - (uint32_t)__builtin_clz(d);
    return 2 * b + ((d >> (b - 1)) & 1u);
}
__device__ inline uint32_t df_dist_extra(uint32_t code) { return code < 4 ? 0u : (code >> 1) - 1; }

// how many bytes from a and from b on are equal, at most cap (a < b, b + cap within the text; tb is readable 3 bytes past its end)
__device__ inline uint32_t df_common(const uint8_t* tb, uint32_t a, uint32_t b, uint32_t cap) {
    uint32_t k = 0;
    while (k < cap) {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) x |= (uint32_t)(tb[a + k + u] ^ tb[b + k + u]) << (8 * u);
        if (x) { k += (uint32_t)__builtin_ctz(x) >> 3; break; }
        k += 4;
    }
    return k < cap ? k : cap;
}

// the code lengths lens_at(0 .. total) as items of the code-length alphabet (16: repeat, 17 / 18: zeros); returns their number
template <typename F> __device__ inline uint32_t df_header_items(F lens_at, uint32_t total, uint16_t* hdr_sym, uint8_t* hdr_extra) {
    uint32_t nh = 0;
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = lens_at(i);
        uint32_t r = 1;
        while (i + r < total && lens_at(i + r) == v) r++;
        if (v == 0 && r >= 3) {
            uint32_t left = r;
            while (left >= 3) {
                const uint32_t k = left > 138 ? 138 : left;
                if (k >= 11) { hdr_sym[nh] = 18; hdr_extra[nh++] = (uint8_t)(k - 11); } else { hdr_sym[nh] = 17; hdr_extra[nh++] = (uint8_t)(k - 3); }
                left -= k;
            }
            for (; left; left--) { hdr_sym[nh] = 0; hdr_extra[nh++] = 0; }
        } else if (v != 0 && r >= 4) {
            hdr_sym[nh] = (uint16_t)v; hdr_extra[nh++] = 0;
            uint32_t left = r - 1;
            while (left >= 3) { const uint32_t k = left > 6 ? 6 : left; hdr_sym[nh] = 16; hdr_extra[nh++] = (uint8_t)(k - 3); left -= k; }
            for (; left; left--) { hdr_sym[nh] = (uint16_t)v; hdr_extra[nh++] = 0; }
        } else {
            for (uint32_t k = 0; k < r; k++) { hdr_sym[nh] = (uint16_t)v; hdr_extra[nh++] = 0; }
        }
        i += r;
    }
    return nh;
}

// One chunk = one deflate block, as k_deflate_chunks.  dist: DF_CHUNK entries per workgroup, gridDim.x <= DF_LZ_MAX_GROUPS of them.
// Bounds: tb is read below n + 3 (df_common), mlen / md at [0, n), table at a 13-bit hash, outw like k_deflate_chunks (the dynamic form
// is written only when it is smaller than n + 5 bytes; the header alone, at most 17 + 19 * 3 + 316 * 14 bits, always fits).
__global__ void __launch_bounds__(DF_T) k_deflate_lz_chunks(const uint8_t* text, const uint64_t* chunk_begin, const uint32_t* chunk_len, uint64_t n_chunks,
                                                             uint8_t* out, uint32_t* sizes, uint32_t* adler, uint16_t* dist) {
    __shared__ uint32_t textw[DF_CHUNK / 4 + 2];
    __shared__ uint32_t outw[DF_OUT_STRIDE / 4 + 4];
    __shared__ uint16_t mlen[DF_CHUNK];                          // bits 0..8 the token's length at p (1: a literal), 9..15 see above
    __shared__ uint32_t freq[DF_MAXSYM], dfreq[32], A[DF_MAXSYM], fr2[DF_MAXSYM], scan_sh[DF_T + 1], clfreq[DF_NCL];
    __shared__ uint16_t code[DF_MAXSYM], dcode[32], order[DF_MAXSYM], clcode[DF_NCL], hdr_sym[DF_MAXSYM + DF_NDIST + 8], entry[DF_T];
    __shared__ uint8_t len[DF_MAXSYM], dlen[32], cllen[DF_NCL], hdr_extra[DF_MAXSYM + DF_NDIST + 8];
    __shared__ uint32_t sh_misc[8], ctl[2], cnt16[16], nxt16[16];                               // 0 header bits, 1 total bits, 2 n header symbols, 3 hlit, 4 hdist
    if (blockIdx.x >= DF_LZ_MAX_GROUPS) return;
    uint8_t* const tb = (uint8_t*)textw;
    uint32_t* const table = outw;
    uint16_t* const md = dist + blockIdx.x * (uint64_t)DF_CHUNK;
    const uint32_t t = threadIdx.x;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t n = chunk_len[c];
        const uint8_t* src = text + chunk_begin[c];
        __syncthreads();
        for (uint32_t i = t; i < n; i += DF_T) tb[i] = src[i];
        for (uint32_t i = t; i < (1u << DF_LZ_HASH_BITS); i += DF_T) table[i] = 0;                // an entry: position + 1, 0 none
        for (uint32_t i = t; i < DF_MAXSYM; i += DF_T) freq[i] = 0;
        if (t < 32) dfreq[t] = 0;
        if (t < DF_NCL) clfreq[t] = 0;
        __syncthreads();
        const uint32_t p0 = t * DF_PER < n ? t * DF_PER : n, p1 = (t + 1) * DF_PER < n ? (t + 1) * DF_PER : n;
        // ---- Adler-32 over the chunk, as k_deflate_chunks ----
        {
            uint32_t sa = 0, sb = 0;
            for (uint32_t i = p0; i < p1; i++) { sa += tb[i]; sb += sa; }
            uint64_t va = sa, vb = (uint64_t)sb + (uint64_t)(n - p1) * sa;
            for (uint32_t d = 32; d; d >>= 1) { va += __shfl_down((unsigned long long)va, d); vb += __shfl_down((unsigned long long)vb, d); }
            if ((t & 63) == 0) { scan_sh[2 * (t >> 6)] = (uint32_t)(va % 65521u); scan_sh[2 * (t >> 6) + 1] = (uint32_t)(vb % 65521u); }
            __syncthreads();
            if (t == 0) {
                const uint32_t a32 = (1u + scan_sh[0] + scan_sh[2] + scan_sh[4] + scan_sh[6]) % 65521u;
                const uint32_t b32 = (uint32_t)(((uint64_t)n + scan_sh[1] + scan_sh[3] + scan_sh[5] + scan_sh[7]) % 65521u);
                adler[c] = (b32 << 16) | a32;
            }
        }
        // ---- the candidate and the choice at every position, a step at a time ----
        for (uint32_t s0 = 0; s0 < n; s0 += DF_LZ_STEP) {
            const uint32_t p = s0 + t;
            const bool hashed = p + 4 <= n;
            uint32_t h = 0, q1 = 0;
            if (hashed) {
                const uint32_t v = (uint32_t)tb[p] | (uint32_t)tb[p + 1] << 8 | (uint32_t)tb[p + 2] << 16 | (uint32_t)tb[p + 3] << 24;
                h = (v * 2654435761u) >> (32 - DF_LZ_HASH_BITS);
                q1 = table[h];
            }
            __syncthreads();                                    // every look-up of the step comes before its entries
            if (hashed) atomicMax(&table[h], p + 1);
            if (p < n) {
                const uint32_t cap = n - p < 258 ? n - p : 258;
                uint32_t run = p ? df_common(tb, p - 1, p, cap) : 0;
                if (run < 3) run = 0;
                const uint32_t hit = q1 ? df_common(tb, q1 - 1, p, cap) : 0;
                uint32_t L = 1, D = 0;
                if (hit >= DF_LZ_MIN && hit >= run + 2) { L = hit; D = p - (q1 - 1); }
                else if (run) { L = run; D = 1; }
                mlen[p] = (uint16_t)L; md[p] = (uint16_t)D;
            }
            __syncthreads();
        }
        for (uint32_t i = t; i < DF_OUT_STRIDE / 4 + 4; i += DF_T) outw[i] = 0;                   // (the table's words)
        // ---- selection: per position the last token of this thread's range on a parse entering there; the chain; the entries ----
        for (uint32_t p = p1; p-- > p0;) {
            const uint32_t L = mlen[p], nxt = p + L;
            const uint32_t last = nxt >= p1 ? p - p0 : (uint32_t)(mlen[nxt] >> 9);
            mlen[p] = (uint16_t)(L | (last << 9));
        }
        __syncthreads();
        if (t == 0) {
            uint32_t pos = 0;
            for (uint32_t g = 0; g < DF_T; g++) {
                const uint32_t a = g * DF_PER, b = (g + 1) * DF_PER < n ? (g + 1) * DF_PER : n;
                if (pos < b) {                                   // (pos >= a: it passed the range before)
                    entry[g] = (uint16_t)pos;
                    const uint32_t lt = a + (mlen[pos] >> 9);
                    pos = lt + (mlen[lt] & 511u);
                } else entry[g] = (uint16_t)DF_LZ_NONE;
            }
        }
        __syncthreads();
        const uint32_t e0 = entry[t];
        // every token of this thread's range: g(position, length, distance), distance 0 a literal
        auto each_token = [&](auto g) {
            if (e0 == DF_LZ_NONE) return;
            for (uint32_t p = e0; p < p1;) {
                const uint32_t L = mlen[p] & 511u;
                g(p, L, L > 1 ? (uint32_t)md[p] : 0u);
                p += L;
            }
        };
        // ---- pass 1: symbol frequencies ----
        each_token([&](uint32_t p, uint32_t L, uint32_t D) {
            if (!D) atomicAdd(&freq[tb[p]], 1u);
            else { atomicAdd(&freq[257 + df_len_code(L)], 1u); atomicAdd(&dfreq[df_dist_code(D)], 1u); }
        });
        if (t == 0) atomicAdd(&freq[256], 1u);
        __syncthreads();
        // ---- the codes (the whole workgroup) and the block header (one lane) ----
        df_code_lengths(freq, DF_NLIT, 15, len, A, order, fr2, ctl);
        df_codes(len, DF_NLIT, code, cnt16, nxt16);
        df_code_lengths(dfreq, DF_NDIST, 15, dlen, A, order, fr2, ctl);
        if (t == 0 && (ctl[1] >> 1) == 0) dlen[0] = dlen[1] = 1;    // no match in the chunk: two codes of one bit make the distance code complete
        __syncthreads();
        df_codes(dlen, DF_NDIST, dcode, cnt16, nxt16);
        if (t == 0) {
            uint32_t hlit = DF_NLIT, hdist = DF_NDIST;
            while (hlit > 257 && len[hlit - 1] == 0) hlit--;
            while (hdist > 1 && dlen[hdist - 1] == 0) hdist--;
            const uint32_t nh = df_header_items([&](uint32_t i) -> uint32_t { return i < hlit ? len[i] : dlen[i - hlit]; }, hlit + hdist, hdr_sym, hdr_extra);
            for (uint32_t i = 0; i < nh; i++) clfreq[hdr_sym[i]]++;
            sh_misc[2] = nh; sh_misc[3] = hlit; sh_misc[4] = hdist;
        }
        __syncthreads();
        df_code_lengths(clfreq, DF_NCL, 7, cllen, A, order, fr2, ctl);
        df_codes(cllen, DF_NCL, clcode, cnt16, nxt16);
        if (t == 0) {
            const uint32_t nh = sh_misc[2], hlit = sh_misc[3], hdist = sh_misc[4];
            uint32_t hclen = DF_NCL;
            while (hclen > 4 && cllen[df_cl_order[hclen - 1]] == 0) hclen--;
            BitW bw{outw, 0};
            bw.put(0u, 1); bw.put(2u, 2);                         // BFINAL 0, BTYPE 10
            bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4);
            for (uint32_t i = 0; i < hclen; i++) bw.put(cllen[df_cl_order[i]], 3);
            for (uint32_t i = 0; i < nh; i++) {
                const uint32_t s = hdr_sym[i];
                bw.put(clcode[s], cllen[s]);
                if (s == 16) bw.put(hdr_extra[i], 2); else if (s == 17) bw.put(hdr_extra[i], 3); else if (s == 18) bw.put(hdr_extra[i], 7);
            }
            sh_misc[0] = (uint32_t)bw.pos;
        }
        __syncthreads();
        // ---- pass 2: bits per thread, prefix sum ----
        uint32_t mybits = 0;
        each_token([&](uint32_t p, uint32_t L, uint32_t D) {
            if (!D) mybits += len[tb[p]];
            else {
                const uint32_t lc = df_len_code(L), dc = df_dist_code(D);
                mybits += len[257 + lc] + df_len_extra[lc] + dlen[dc] + df_dist_extra(dc);
            }
        });
        {
            uint32_t inc = mybits;
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d); if ((t & 63) >= d) inc += o; }
            if ((t & 63) == 63) scan_sh[t >> 6] = inc;
            __syncthreads();
            uint32_t base = sh_misc[0];
            for (uint32_t w = 0; w < (t >> 6); w++) base += scan_sh[w];
            if (t == DF_T - 1) sh_misc[1] = base + inc + len[256];              // body and end-of-block
            mybits = base + inc - mybits;                                      // this thread's first bit
        }
        __syncthreads();
        const uint32_t total_bits = sh_misc[1];
        const uint32_t dyn_bytes = (total_bits + 3 + 7) / 8 + 4;                // with the empty stored block: 3 bits, padding, 00 00 FF FF
        const bool stored = dyn_bytes >= n + 5;
        uint8_t* dst = out + c * (uint64_t)DF_OUT_STRIDE;
        if (!stored) {
            // ---- pass 3: the tokens' bits ----
            uint64_t pos = mybits;
            auto put = [&](uint32_t v, uint32_t nbits) {                         // other lanes write the same words: atomic OR
                const uint32_t i = (uint32_t)(pos >> 5), s = (uint32_t)(pos & 31);
                atomicOr(&outw[i], v << s);
                if (s + nbits > 32) atomicOr(&outw[i + 1], v >> (32 - s));
                pos += nbits;
            };
            each_token([&](uint32_t p, uint32_t L, uint32_t D) {
                if (!D) { const uint32_t v = tb[p]; put(code[v], len[v]); return; }
                const uint32_t lc = df_len_code(L), dc = df_dist_code(D), de = df_dist_extra(dc);
                put(code[257 + lc], len[257 + lc]);
                if (df_len_extra[lc]) put(L - df_len_base[lc], df_len_extra[lc]);
                put(dcode[dc], dlen[dc]);
                if (de) put(D - df_dist_base[dc], de);
            });
            __syncthreads();
            if (t == 0) {
                BitW bw{outw, (uint64_t)total_bits - len[256]};
                bw.put(code[256], len[256]);
                bw.put(0u, 3);                                                   // BFINAL 0, BTYPE 00: the empty stored block
                bw.pos = (bw.pos + 7) & ~7ull;
                bw.put(0xFFFF0000u, 32);
                sizes[c] = (uint32_t)(bw.pos >> 3);
            }
            __syncthreads();
            for (uint32_t i = t; i < (dyn_bytes + 3) / 4; i += DF_T) ((uint32_t*)dst)[i] = outw[i];
        } else {
            if (t == 0) {
                dst[0] = 0; dst[1] = (uint8_t)n; dst[2] = (uint8_t)(n >> 8); dst[3] = (uint8_t)~n; dst[4] = (uint8_t)(~n >> 8);
                sizes[c] = n + 5;
            }
            for (uint32_t i = t; i < n; i += DF_T) dst[5 + i] = tb[i];
        }
    }
}

// the read blocks' streams, contiguous: 78 01, the chunks, the final empty stored block; the Adler-32 is added on the host
__global__ void k_deflate_gather(const uint8_t* chunks, const uint32_t* sizes, const uint64_t* chunk_dst, uint64_t n_chunks, uint8_t* dst) {
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint8_t* s = chunks + c * (uint64_t)DF_OUT_STRIDE;
        uint8_t* d = dst + chunk_dst[c];
        const uint32_t n = sizes[c];
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
    }
}

// ---- BGZF: any text as a series of independent gzip members (leon_text_bgzf_device) ----
// One member = one chunk of k_deflate_chunks (LEON_BGZF_MEMBER_TEXT == DF_CHUNK bytes of text, the last one what is left):
//   18 bytes of header (1f 8b 08 04, no time, XFL 0, OS ff, XLEN 6, the extra field 'B' 'C' 2 0 BSIZE = member bytes - 1),
//   the sizes[c] bytes the chunk kernel wrote (its block and the empty stored block behind it, or the stored form: BFINAL 0 both),
//   03 00 (the empty fixed block, BFINAL 1), CRC-32 and ISIZE of the chunk's text: sizes[c] + 28 bytes, at most 32 801.
static_assert(DF_CHUNK == LEON_BGZF_MEMBER_TEXT, "a BGZF member is one chunk of k_deflate_chunks");
constexpr uint32_t BGZF_FRAME = 28;                            // header 18 + 03 00 + CRC-32 + ISIZE
constexpr uint32_t BGZF_MEMBER_MAX = DF_CHUNK + 5 + BGZF_FRAME;   // the stored form
constexpr uint64_t BGZF_MAX_GROUPS = 4096;                     // k_bgzf_members' grid cap: a workgroup frames members c, c + cap, ...
static_assert(BGZF_MEMBER_MAX <= 65536, "BSIZE is 16 bits");
const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
__device__ const uint8_t bgzf_head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};

// the chunk table of a slice of n_text bytes: begin[c] = c * DF_CHUNK for c <= n (the last entry = n_text: the CRC's segment bounds too)
__global__ void k_bgzf_table(uint64_t n_text, uint64_t n, uint64_t* begin, uint32_t* len) {
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c > n) return;
    const uint64_t a = c * DF_CHUNK < n_text ? c * DF_CHUNK : n_text;
    begin[c] = a;
    if (c < n) len[c] = (uint32_t)(n_text - a < DF_CHUNK ? n_text - a : DF_CHUNK);
}
// member sizes as 64-bit words for the scan; msize[n] = 0, so that the exclusive sum's entry n is the slice's size
__global__ void k_bgzf_sizes(const uint32_t* sizes, uint64_t n, uint64_t* msize) {
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c <= n) msize[c] = c < n ? (uint64_t)sizes[c] + BGZF_FRAME : 0;
}
// Member-driven, one workgroup per member, like k_deflate_gather.  Bounds: chunks is read at [c * DF_OUT_STRIDE, + sizes[c]) with
// sizes[c] <= len[c] + 5 (k_deflate_chunks keeps the stored form when the dynamic one is not smaller); dst is written at
// [moff[c], moff[c + 1]) = sizes[c] + 28 bytes, moff[n] <= n * BGZF_MEMBER_MAX = what the caller allocated.  No atomics, nothing waits.
__global__ void __launch_bounds__(256) k_bgzf_members(const uint8_t* chunks, const uint32_t* sizes, const uint32_t* len, const uint32_t* crc, const uint64_t* moff,
                                                      uint64_t n, uint8_t* dst) {
    const uint32_t t = threadIdx.x;
    for (uint64_t c = blockIdx.x; c < n; c += gridDim.x) {
        const uint8_t* s = chunks + c * (uint64_t)DF_OUT_STRIDE;
        uint8_t* d = dst + moff[c];
        const uint32_t m = sizes[c], bsize = m + BGZF_FRAME - 1;
        if (t < 16) d[t] = bgzf_head[t];
        else if (t < 18) d[t] = (uint8_t)(bsize >> (8 * (t - 16)));
        for (uint32_t i = t; i < m; i += 256) d[18 + i] = s[i];
        if (t >= 32 && t < 42) {                                  // (another wave than the header's)
            const uint32_t j = t - 32;
            const uint32_t v = j == 0 ? 3u : j == 1 ? 0u : j < 6 ? crc[c] >> (8 * (j - 2)) : len[c] >> (8 * (j - 6));
            d[18 + m + j] = (uint8_t)v;
        }
    }
}

// per member (its offset in the call's output, its offset in the call's text), then the slice's size: what the host fetches in one copy
__global__ void k_bgzf_index(const uint64_t* moff, const uint64_t* begin, uint64_t n, uint64_t out_base, uint64_t text_base, uint64_t* idx) {
    const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (c < n) { idx[2 * c] = out_base + moff[c]; idx[2 * c + 1] = text_base + begin[c]; }
    else if (c == n) idx[2 * n] = moff[n];
}

// ---- members cut at record starts (leon_text_bgzf_records_device) ----
// The record starts of the call's text, S(0 .. n_starts): 0 when there is a head (one record as far as the rule goes), then
// n_head + rec_off[0 .. n_records]; n_starts = (n_head != 0) + n_records + 1.
__device__ __forceinline__ uint64_t bgzf_start(const uint64_t* rec_off, uint64_t n_head, uint64_t k) {
    const uint64_t hs = n_head ? 1 : 0;
    return k < hs ? 0 : n_head + (rec_off ? rec_off[k - hs] : 0);
}
// flags (zeroed by the caller): 1 the offsets run backwards or stand still somewhere, 2 the first is not 0, 4 the last is not n_body.
// Runs before anything is indexed with them; every lane stores the same word, no atomics (k_fmt_sizes' discipline).
__global__ void __launch_bounds__(256) k_bgzf_check_recs(const uint64_t* __restrict__ rec_off, uint64_t n_records, uint64_t n_body, uint32_t* __restrict__ flags) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r > n_records) return;
    if (r == n_records) {
        if (rec_off[0] != 0) flags[1] = 1;
        if (rec_off[n_records] != n_body) flags[2] = 1;
        return;
    }
    if (rec_off[r + 1] <= rec_off[r]) flags[0] = 1;
}

// The cut table of a slice.  The greedy chain is serial (cut c + 1 follows from cut c), so ONE workgroup walks it, in phases separated
// by barriers: all threads load the starts S(k .. k + cnt) into LDS as 32-bit offsets from S(k) (clamped: an offset the walk may take
// as a cut is below 2^31, see below), then wave 0 walks the chain inside the tile -- per member one look at 64 starts around where
// the member before would put the cut, a binary search in LDS when the cut is not among them -- until a step's
// range p + W reaches past the tile's last start; the next phase begins at the current cut.  A tile holds 16 000 starts, so records of
// two bytes and more advance by at least one member per phase; a step whose W bytes hold more starts than a tile (records of one
// byte) does that one search in global memory.  An oversized record is walked with its two 64-bit starts from global memory.
//   state in : k0 the start the slice's first cut is at, skip0 the bytes of record k0 already taken (a multiple of W, an oversized
//              record cut by a slice's end); budget_end: a member that ends behind it is left to the next slice unless it is the
//              first; cap: members begin / len have room for (begin: cap + 1).
//   state out: [0] members, [1] k, [2] skip, [3] S(k) + skip = where the text taken ends (also begin[members]: the CRC's last bound),
//              [4] 1 when the budget or cap stopped the walk (more may follow), 0 when the rule did.
// begin == NULL: members are counted only.  32-bit range: after an oversized record the phase ends when the next start is at 2^31 or
// more from S(k); an ordinary step adds at most W, and a phase has at most 16 000 of them: p + W < 2^31 + 2^29 + W, which does not
// wrap, and a clamped entry (2^32 - 1) is above every p + W, so it is never taken for a cut.
// Bounds: rec_off is read at [0, n_records], tile at [0, cnt), begin at [0, cap], len at [0, cap).  No atomics, nothing spins.
constexpr uint32_t BGZF_CUT_TILE = 16000;
constexpr uint32_t BGZF_CUT_T = 1024;
// which of tile[w0 .. w0 + 64) are at most target and not behind hi, a bit per lane of the wave (the tile ascends: ones, then zeros);
// at_cut = the last of them, read from the lane that holds it (no second trip to LDS on the chain)
__device__ __forceinline__ uint64_t bgzf_window(const uint32_t* tile, uint32_t w0, uint32_t hi, uint32_t target, uint32_t lane, uint32_t& at_cut) {
    const uint32_t j = w0 + lane;
    const uint32_t v = j <= hi ? tile[j] : 0xFFFFFFFFu;           // (above every target)
    const uint64_t in = __ballot(v <= target);
    at_cut = in ? (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_popcountll(in) - 1) : 0u;
    return in;
}
__global__ void __launch_bounds__(BGZF_CUT_T) k_bgzf_cuts(const uint64_t* __restrict__ rec_off, uint64_t n_starts, uint64_t n_head, uint64_t k0, uint64_t skip0,
                                                          uint64_t budget_end, uint64_t n_text, uint32_t last, uint64_t cap, uint64_t* __restrict__ begin,
                                                          uint32_t* __restrict__ len, uint64_t* __restrict__ state) {
    __shared__ uint32_t tile[BGZF_CUT_TILE];
    __shared__ uint64_t sh_k;
    __shared__ uint32_t sh_done;
    constexpr uint32_t W = DF_CHUNK;
    const uint32_t t = threadIdx.x;
    uint64_t n = 0, skip = skip0;                                 // (wave 0's, the same in every lane)
    uint32_t more = 0, guess = 64;
    if (t == 0) { sh_k = k0; sh_done = 0; }
    for (;;) {
        __syncthreads();
        const uint64_t k = sh_k;
        if (sh_done) break;                                       // (uniform)
        const uint64_t base = bgzf_start(rec_off, n_head, k), left = n_starts - k;
        const uint32_t cnt = left < BGZF_CUT_TILE ? (uint32_t)left : BGZF_CUT_TILE;
        for (uint32_t i0 = t; i0 < cnt; i0 += 4 * BGZF_CUT_T) {    // four loads in flight per thread: one workgroup has only latency to hide
            uint64_t v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) { const uint32_t i = i0 + u * BGZF_CUT_T; v[u] = i < cnt ? bgzf_start(rec_off, n_head, k + i) - base : 0; }
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) { const uint32_t i = i0 + u * BGZF_CUT_T; if (i < cnt) tile[i] = v[u] < 0xFFFFFFFFull ? (uint32_t)v[u] : 0xFFFFFFFFu; }
        }
        __syncthreads();
        if (t >= 64) continue;                                    // wave 0 walks, its lanes in step: the state is uniform, lane 0 stores
        uint32_t i = 0, done = 0, p = 0;                          // p = tile[i], carried in a register (tile[0] = 0)
        const uint32_t tail = tile[cnt - 1];
        uint64_t next_k = 0;                                      // (a step that searched global memory: the next phase's first start)
        for (;;) {
            if (n >= cap) { more = 1; done = 1; break; }
            if (k + i + 1 >= n_starts) { done = 1; break; }       // the whole text is taken
            const uint64_t p_abs = base + p;
            if (!skip && !last && n_text - p_abs <= W) { done = 1; break; }
            if (i + 1 >= cnt) break;                              // (i != 0: a tile has two starts when the text goes on)
            if (skip || tile[i + 1] - p > W) {                    // an oversized record: members of its own
                const uint64_t a = bgzf_start(rec_off, n_head, k + i), L = bgzf_start(rec_off, n_head, k + i + 1) - a;
                while (skip < L) {
                    const uint64_t m = L - skip < W ? L - skip : W;
                    if (n >= cap || (n && a + skip + m > budget_end)) { more = 1; done = 1; break; }
                    if (begin && t == 0) { begin[n] = a + skip; len[n] = (uint32_t)m; }
                    n++; skip += m;
                }
                if (done) break;
                skip = 0; i++;
                p = tile[i];
                if (p >= 0x80000000u) break;                // the next phase counts from this cut
                continue;
            }
            const uint32_t target = p + W;
            uint64_t m;
            if (tail <= target && k + cnt < n_starts) {  // the range reaches past the tile
                if (i) break;
                uint64_t lo = k + cnt - 1, hi = n_starts - 1 < k + W ? n_starts - 1 : k + W;     // (records have at least one byte)
                while (lo < hi) {
                    const uint64_t mid = lo + (hi - lo + 1) / 2;
                    if (bgzf_start(rec_off, n_head, mid) <= p_abs + W) lo = mid; else hi = mid - 1;
                }
                m = bgzf_start(rec_off, n_head, lo) - p_abs;
                if (n && p_abs + m > budget_end) { more = 1; done = 1; break; }
                next_k = lo;
            } else {
                // the largest j in [lo, hi] with tile[j] <= target (tile[lo] is).  The 64 lanes look at 64 starts around where a member
                // of as many records as the one before would end -- one LDS read whose address does not wait for p -- and the ballot
                // is the answer when it changes inside the window; a binary search over what is left otherwise
                uint32_t lo = i + 1, hi = cnt - 1;
                uint32_t w0 = i + guess > lo + 32 ? i + guess - 32 : lo;
                if (w0 + 63 > hi) w0 = hi >= lo + 63 ? hi - 63 : lo;
                uint32_t q;
                const uint64_t in = bgzf_window(tile, w0, hi, target, t, q);
                if (in && (~in != 0 || w0 + 63 >= hi)) lo = w0 + (uint32_t)__builtin_popcountll(in) - 1;
                else {
                    if (!in) hi = w0 - 1; else lo = w0 + 63;      // (w0 != i + 1 when none is in: tile[i + 1] is)
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi + 1) >> 1;
                        if (tile[mid] <= target) lo = mid; else hi = mid - 1;
                    }
                    q = tile[lo];
                }
                m = q - p;
                if (n && p_abs + m > budget_end) { more = 1; done = 1; break; }
                guess = lo - i;
                i = lo; p = q;
            }
            if (begin && t == 0) { begin[n] = p_abs; len[n] = (uint32_t)m; }
            n++;
            if (next_k) break;
        }
        const uint64_t kk = next_k ? next_k : k + i;
        if (t == 0) {
            if (done) {
                const uint64_t end = bgzf_start(rec_off, n_head, kk) + skip;
                state[0] = n; state[1] = kk; state[2] = skip; state[3] = end; state[4] = more;
                if (begin) begin[n] = end;
            }
            sh_k = kk; sh_done = done;
        }
    }
}

// Device buffers kept from call to call (one set per process, taken under a lock): a call per batch of a file would otherwise
// allocate and free ~1.5 GB each time, and memory this process has freed comes back from hipMalloc at the driver's wiping
// rate (~43 GB/s), for this call and for whoever allocates next.  Large calls go through in slices, so the set stays small.
// (a quarter of slack, not DevBuf's eighth: it decides how often a file's batches reallocate)
struct Grow : DevBuf { Grow() { slack = 4; } };
// One set PER DEVICE (it was one for the process, dropped and rebuilt whenever the device changed: callers on several GPUs serialised
// behind one mutex and thrashed 1.5 GB each way -- ADVICE r3).  A device's set is used by one call at a time.
struct DeflateScratch {
    std::mutex mu;
    int device = -1;
    Grow off, text, cb, cl, out, sizes, adler, cdst, fin;
    std::vector<uint8_t> h;
    void drop() { for (Grow* g : {&off, &text, &cb, &cl, &out, &sizes, &adler, &cdst, &fin}) g->release(); }
};
constexpr int DF_MAX_DEVICES = 64;
DeflateScratch* scratch_table() { static DeflateScratch* t = new DeflateScratch[DF_MAX_DEVICES]; return t; }     // (never destroyed: the HIP runtime may be gone by then)
DeflateScratch& scratch(int device_id) { return scratch_table()[device_id]; }

constexpr uint64_t DF_SLICE_TEXT = 512ull << 20;                // text bytes per slice of a large call

// blocks [b0, b1) of the call: reads [r0, r1), whose qualities start at d_quals + (offsets[r0] - offsets[0])
int deflate_slice(DeflateScratch& S, int device_id, const uint8_t* d_quals, const uint64_t* offsets, uint64_t r0, uint64_t r1, uint32_t reads_per_block,
                  leon_block_sink sink, void* user, uint64_t first_block_id) {
    hipStream_t s = nullptr;
    static const bool trace = getenv("LEON_TRACE_DEFLATE") != nullptr;           // measurement aid: a slice's stages on stderr
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    double ms_tables = 0, ms_kernels = 0, ms_d2h = 0;
    const uint64_t n_reads = r1 - r0, n_blocks = (n_reads + reads_per_block - 1) / reads_per_block;
    const uint64_t* off = offsets + r0;
    const uint64_t q0 = off[0], n_q = off[n_reads] - q0, n_text = n_q + n_reads;
    const uint8_t* dq = d_quals + (q0 - offsets[0]);
    // chunk table: block b's text is [blk_text[b], blk_text[b + 1]) of the slice's text, cut in DF_CHUNK pieces
    std::vector<uint64_t> blk_text(n_blocks + 1), chunk_begin, blk_chunk0(n_blocks + 1);
    std::vector<uint32_t> chunk_len;
    for (uint64_t b = 0; b <= n_blocks; b++) {
        const uint64_t r = std::min<uint64_t>(n_reads, b * reads_per_block);
        blk_text[b] = off[r] - q0 + r;
    }
    for (uint64_t b = 0; b < n_blocks; b++) {
        blk_chunk0[b] = chunk_begin.size();
        for (uint64_t p = blk_text[b]; p < blk_text[b + 1]; p += DF_CHUNK) {
            chunk_begin.push_back(p);
            chunk_len.push_back((uint32_t)std::min<uint64_t>(DF_CHUNK, blk_text[b + 1] - p));
        }
    }
    blk_chunk0[n_blocks] = chunk_begin.size();
    const uint64_t n_chunks = chunk_begin.size();
    ms_tables = ms_since(t_start);
    const auto t_k = std::chrono::steady_clock::now();
    DEVCHK(S.off.ensure((n_reads + 1) * 8)); DEVCHK(S.text.ensure(n_text + 64));
    DEVCHK(staged_h2d(device_id, S.off.p, off, (n_reads + 1) * 8));
    hipLaunchKernelGGL(k_qual_text, dim3((uint32_t)std::min<uint64_t>((n_reads + 3) / 4, 1u << 16)), dim3(256), 0, s, dq, S.off.as<uint64_t>(), n_reads, q0,
                       S.text.as<uint8_t>());
    std::vector<uint32_t> sizes(n_chunks), adl(n_chunks);
    if (n_chunks) {
        DEVCHK(S.cb.ensure(n_chunks * 8)); DEVCHK(S.cl.ensure(n_chunks * 4)); DEVCHK(S.out.ensure(n_chunks * (uint64_t)DF_OUT_STRIDE));
        DEVCHK(S.sizes.ensure(n_chunks * 4)); DEVCHK(S.adler.ensure(n_chunks * 4)); DEVCHK(S.cdst.ensure(n_chunks * 8));
        DEVCHK(hipMemcpyAsync(S.cb.p, chunk_begin.data(), n_chunks * 8, hipMemcpyHostToDevice, s));
        DEVCHK(hipMemcpyAsync(S.cl.p, chunk_len.data(), n_chunks * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_deflate_chunks, dim3((uint32_t)std::min<uint64_t>(n_chunks, 1u << 20)), dim3(DF_T), 0, s, S.text.as<uint8_t>(), S.cb.as<uint64_t>(),
                           S.cl.as<uint32_t>(), n_chunks, S.out.as<uint8_t>(), S.sizes.as<uint32_t>(), S.adler.as<uint32_t>());
        DEVCHK(hipGetLastError());
        DEVCHK(hipMemcpy(sizes.data(), S.sizes.p, n_chunks * 4, hipMemcpyDeviceToHost));
        DEVCHK(hipMemcpy(adl.data(), S.adler.p, n_chunks * 4, hipMemcpyDeviceToHost));
    }
    // layout of the final streams: per block 2 bytes of zlib header, its chunks, 5 bytes of final stored block, 4 of Adler-32
    std::vector<uint64_t> blk_dst(n_blocks + 1, 0), chunk_dst(n_chunks);
    for (uint64_t b = 0; b < n_blocks; b++) {
        uint64_t at = blk_dst[b] + 2;
        for (uint64_t c = blk_chunk0[b]; c < blk_chunk0[b + 1]; c++) { chunk_dst[c] = at; at += sizes[c]; }
        blk_dst[b + 1] = at + 5 + 4;
    }
    const uint64_t total = blk_dst[n_blocks];
    if (S.h.size() < total) S.h.resize(total + total / 4);
    uint8_t* h = S.h.data();
    if (n_chunks) {
        DEVCHK(S.fin.ensure(total + 16));
        DEVCHK(hipMemcpyAsync(S.cdst.p, chunk_dst.data(), n_chunks * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_deflate_gather, dim3((uint32_t)std::min<uint64_t>(n_chunks, 1u << 20)), dim3(256), 0, s, S.out.as<uint8_t>(), S.sizes.as<uint32_t>(),
                           S.cdst.as<uint64_t>(), n_chunks, S.fin.as<uint8_t>());
        DEVCHK(hipGetLastError());
        DEVCHK(hipStreamSynchronize(s));
        ms_kernels = ms_since(t_k);
        const auto t_d = std::chrono::steady_clock::now();
        DEVCHK(staged_d2h(device_id, h, S.fin.p, total));
        ms_d2h = ms_since(t_d);
    }
    const auto t_sink = std::chrono::steady_clock::now();
    for (uint64_t b = 0; b < n_blocks; b++) {
        uint8_t* p = h + blk_dst[b];
        p[0] = 0x78; p[1] = 0x01;
        uLong ad = adler32(0L, Z_NULL, 0);
        for (uint64_t c = blk_chunk0[b]; c < blk_chunk0[b + 1]; c++) ad = adler32_combine(ad, adl[c], (z_off_t)chunk_len[c]);
        uint8_t* e = h + blk_dst[b + 1] - 9;
        e[0] = 1; e[1] = 0; e[2] = 0; e[3] = 0xFF; e[4] = 0xFF;                  // BFINAL 1, stored, empty
        e[5] = (uint8_t)(ad >> 24); e[6] = (uint8_t)(ad >> 16); e[7] = (uint8_t)(ad >> 8); e[8] = (uint8_t)ad;
        const uint32_t nr = (uint32_t)std::min<uint64_t>(reads_per_block, n_reads - b * reads_per_block);
        if (sink(user, first_block_id + b, p, blk_dst[b + 1] - blk_dst[b], nr)) return dev_fail(LEON_E_SINK, "qual_deflate: block sink returned non-zero");
    }
    if (trace) fprintf(stderr, "[leon deflate] %llu blocks, %.1f MB of text -> %.1f MB: tables %.1f ms, offsets + kernels %.1f, D2H %.1f, sink %.1f\n",
                       (unsigned long long)n_blocks, n_text / 1e6, total / 1e6, ms_tables, ms_kernels, ms_d2h, ms_since(t_sink));
    return LEON_OK;
}

// ---- leon_text_bgzf_device: the buffers it keeps (one set per device, like DeflateScratch) and a slice of its text ----
struct BgzfScratch {
    std::mutex mu;
    int device = -1;
    Grow begin, len, out, sizes, adler, crc, msize, moff, tmp, framed, idx, state, lzdist;     // lzdist: k_deflate_lz_chunks' distances
    std::vector<uint64_t> h_idx;
    void drop() { for (Grow* g : {&begin, &len, &out, &sizes, &adler, &crc, &msize, &moff, &tmp, &framed, &idx, &state, &lzdist}) g->release(); }
};
// the member tables of a call (host memory), filled slice by slice; out == NULL: none asked for
struct BgzfIndex { uint64_t* out = nullptr; uint64_t* text = nullptr; uint64_t at = 0; };
BgzfScratch* bgzf_table() { static BgzfScratch* t = new BgzfScratch[DF_MAX_DEVICES]; return t; }
constexpr uint64_t BGZF_SLICE_TEXT = 512ull << 20;

// text bytes per slice: LEON_BGZF_SLICE (tests), rounded down to whole members, at least one
uint64_t bgzf_slice_text() {
    uint64_t v = BGZF_SLICE_TEXT;
    if (const char* e = getenv("LEON_BGZF_SLICE")) { const long long x = atoll(e); if (x > 0) v = (uint64_t)x; }
    return std::max<uint64_t>(v / DF_CHUNK, 1) * DF_CHUNK;
}

// The n members of S.begin / S.len -- offsets into d_text, member c = [begin[c], begin[c + 1]), [lo, hi) in all, as k_bgzf_table or
// k_bgzf_cuts left them on stream s -- compressed, framed and delivered at `base` of the call's output; *out_size = their bytes.
// ix (may be NULL): the call's member tables, which receive base + the members' offsets and text_base + begin[c].
// flags: LEON_BGZF_F_MATCHES has k_deflate_lz_chunks write the members' blocks instead of k_deflate_chunks.
int bgzf_members_out(BgzfScratch& S, int device_id, hipStream_t s, const uint8_t* d_text, uint64_t n, uint64_t lo, uint64_t hi, uint64_t base, uint64_t text_base,
                     leon_piece_sink sink, void* user, BgzfIndex* ix, const std::string& who, uint32_t flags, uint64_t* out_size) {
    DEVCHK(S.sizes.ensure(n * 4)); DEVCHK(S.adler.ensure(n * 4)); DEVCHK(S.crc.ensure(n * 4));
    DEVCHK(S.msize.ensure((n + 1) * 8)); DEVCHK(S.moff.ensure((n + 1) * 8));
    DEVCHK(S.out.ensure(n * (uint64_t)DF_OUT_STRIDE)); DEVCHK(S.framed.ensure(n * (uint64_t)BGZF_MEMBER_MAX));
    size_t tmp_bytes = 0;
    DEVCHK(prim::ExclusiveSum(nullptr, tmp_bytes, S.msize.as<uint64_t>(), S.moff.as<uint64_t>(), n + 1, s));
    DEVCHK(S.tmp.ensure(tmp_bytes));
    const uint32_t tgrid = (uint32_t)((n + 1 + 255) / 256);
    if (flags & LEON_BGZF_F_MATCHES) {
        DEVCHK(S.lzdist.ensure((uint64_t)DF_LZ_MAX_GROUPS * DF_CHUNK * sizeof(uint16_t)));
        hipLaunchKernelGGL(k_deflate_lz_chunks, dim3((uint32_t)std::min<uint64_t>(n, DF_LZ_MAX_GROUPS)), dim3(DF_T), 0, s, d_text, S.begin.as<uint64_t>(),
                           S.len.as<uint32_t>(), n, S.out.as<uint8_t>(), S.sizes.as<uint32_t>(), S.adler.as<uint32_t>(), S.lzdist.as<uint16_t>());
    } else
        hipLaunchKernelGGL(k_deflate_chunks, dim3((uint32_t)std::min<uint64_t>(n, 1u << 20)), dim3(DF_T), 0, s, d_text, S.begin.as<uint64_t>(), S.len.as<uint32_t>(), n,
                           S.out.as<uint8_t>(), S.sizes.as<uint32_t>(), S.adler.as<uint32_t>());
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemsetAsync(S.crc.p, 0, n * 4, s));
    launch_crc32_segments(s, d_text, S.begin.as<uint64_t>(), n, crc32_tile_count(d_text, lo, hi), S.crc.as<uint32_t>());
    DEVCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bgzf_sizes, dim3(tgrid), dim3(256), 0, s, S.sizes.as<uint32_t>(), n, S.msize.as<uint64_t>());
    DEVCHK(prim::ExclusiveSum(S.tmp.p, tmp_bytes, S.msize.as<uint64_t>(), S.moff.as<uint64_t>(), n + 1, s));
    hipLaunchKernelGGL(k_bgzf_members, dim3((uint32_t)std::min<uint64_t>(n, BGZF_MAX_GROUPS)), dim3(256), 0, s, S.out.as<uint8_t>(), S.sizes.as<uint32_t>(), S.len.as<uint32_t>(),
                       S.crc.as<uint32_t>(), S.moff.as<uint64_t>(), n, S.framed.as<uint8_t>());
    DEVCHK(hipGetLastError());
    uint64_t total = 0;
    if (ix && ix->out) {                                          // the members' places come with the total, in the one small copy
        DEVCHK(S.idx.ensure((2 * n + 1) * 8));
        S.h_idx.resize(2 * n + 1);
        hipLaunchKernelGGL(k_bgzf_index, dim3(tgrid), dim3(256), 0, s, S.moff.as<uint64_t>(), S.begin.as<uint64_t>(), n, base, text_base, S.idx.as<uint64_t>());
        DEVCHK(hipGetLastError());
        DEVCHK(hipMemcpyAsync(S.h_idx.data(), S.idx.p, (2 * n + 1) * 8, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
        total = S.h_idx[2 * n];
        for (uint64_t c = 0; c < n; c++) { ix->out[ix->at + c] = S.h_idx[2 * c]; ix->text[ix->at + c] = S.h_idx[2 * c + 1]; }
        ix->at += n;
    } else {
        DEVCHK(hipMemcpyAsync(&total, S.moff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
    }
    if (total > n * (uint64_t)BGZF_MEMBER_MAX || total < n * (uint64_t)BGZF_FRAME) return dev_fail(LEON_E_OVERFLOW, who + ": the members' sizes do not add up");
    const int rc = staged_d2h_pieces(device_id, S.framed.p, total, [&](uint64_t offset, const void* p, uint64_t size) { return sink(user, base + offset, p, size); });
    if (rc == 2) return dev_fail(LEON_E_SINK, who + ": the sink returned non-zero");
    if (rc) return dev_fail(LEON_E_HIP, who + ": copy to the host failed");
    *out_size = total;
    return LEON_OK;
}

// the n_text bytes at d_text as ceil(n_text / DF_CHUNK) members, delivered at `base` of the call's output; *out_size = their bytes
int bgzf_slice(BgzfScratch& S, int device_id, hipStream_t s, const uint8_t* d_text, uint64_t n_text, uint64_t base, uint64_t text_base, leon_piece_sink sink, void* user,
               BgzfIndex* ix, const std::string& who, uint32_t flags, uint64_t* out_size) {
    const uint64_t n = (n_text + DF_CHUNK - 1) / DF_CHUNK;
    DEVCHK(S.begin.ensure((n + 1) * 8)); DEVCHK(S.len.ensure(n * 4));
    hipLaunchKernelGGL(k_bgzf_table, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, s, n_text, n, S.begin.as<uint64_t>(), S.len.as<uint32_t>());
    return bgzf_members_out(S, device_id, s, d_text, n, 0, n_text, base, text_base, sink, user, ix, who, flags, out_size);
}

// the fixed cuts of leon_text_bgzf_device and of leon_text_bgzf_records_device without records: `taken` bytes of d_text in slices
int bgzf_fixed(int device_id, const uint8_t* d_text, uint64_t taken, leon_piece_sink sink, void* user, BgzfIndex* ix, const std::string& who, uint32_t flags, uint64_t* at,
               uint64_t* members) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) { (void)hipGetLastError(); return dev_fail(LEON_E_NO_DEVICE, who + ": no such HIP device"); }
    if (device_id >= DF_MAX_DEVICES) return dev_fail(LEON_E_INVALID, who + ": device ordinal beyond the scratch table");
    DEVCHK(hipSetDevice(device_id));
    BgzfScratch& S = bgzf_table()[device_id];
    std::lock_guard<std::mutex> lock(S.mu);
    S.device = device_id;
    CallStream st;
    if (const int rc = dev_stream(st)) return rc;
    const uint64_t slice = bgzf_slice_text();
    for (uint64_t a = 0; a < taken; a += slice) {                 // sequential: a slice's base is the sum of the sizes before it
        const uint64_t m = std::min(slice, taken - a);
        uint64_t size = 0;
        const int rc = bgzf_slice(S, device_id, st.s, d_text + a, m, *at, a, sink, user, ix, who, flags, &size);
        if (rc) return rc;
        *at += size; *members += (m + DF_CHUNK - 1) / DF_CHUNK;
    }
    return LEON_OK;
}

}  // namespace
}  // namespace leon

using namespace leon;

extern "C" int leon_qual_deflate_blocks_device(int device_id, const uint8_t* d_quals, const uint64_t* offsets, uint64_t n_reads,
                                               uint32_t reads_per_block, leon_block_sink sink, void* user, uint64_t first_block_id) {
    if ((n_reads && (!d_quals || !offsets)) || !sink || !reads_per_block) return dev_fail(LEON_E_INVALID, "qual_deflate: null argument");
    if (!n_reads) return LEON_OK;
    for (uint64_t i = 0; i < n_reads; i++)
        if (offsets[i + 1] < offsets[i]) return dev_fail(LEON_E_INVALID, "qual_deflate: offsets are not monotonic");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return dev_fail(LEON_E_NO_DEVICE, "qual_deflate: no such HIP device");
    if (device_id >= DF_MAX_DEVICES) return dev_fail(LEON_E_INVALID, "qual_deflate: device ordinal beyond the scratch table");
    DEVCHK(hipSetDevice(device_id));
    DeflateScratch& S = scratch(device_id);
    std::lock_guard<std::mutex> lock(S.mu);
    S.device = device_id;
    const uint64_t n_blocks = (n_reads + reads_per_block - 1) / reads_per_block;
    for (uint64_t b0 = 0; b0 < n_blocks;) {                      // slices of whole blocks, ~DF_SLICE_TEXT of text each
        uint64_t b1 = b0 + 1;
        const uint64_t r0 = b0 * reads_per_block;
        while (b1 < n_blocks && offsets[std::min<uint64_t>(n_reads, (b1 + 1) * reads_per_block)] - offsets[r0] <= DF_SLICE_TEXT) b1++;
        const uint64_t r1 = std::min<uint64_t>(n_reads, b1 * reads_per_block);
        const int rc = deflate_slice(S, device_id, d_quals, offsets, r0, r1, reads_per_block, sink, user, first_block_id + b0);
        if (rc) return rc;
        b0 = b1;
    }
    return LEON_OK;
}

/* any text in device memory as BGZF: the whole members of it, or with `last` all of it and the EOF marker */
extern "C" int leon_text_bgzf_device(int device_id, const uint8_t* d_text, uint64_t n_text, int last, leon_piece_sink sink, void* user,
                                     uint64_t* n_taken, uint64_t* out_bytes, uint64_t* n_members) {
    auto refuse = [](const char* why) { return dev_fail(LEON_E_INVALID, std::string("leon_text_bgzf_device: ") + why); };
    if (!d_text && n_text) return refuse("d_text is NULL with n_text != 0");
    if (!sink) return refuse("sink is NULL");
    if (!n_taken) return refuse("n_taken is NULL");
    if (!out_bytes) return refuse("out_bytes is NULL");
    if (last != 0 && last != 1) return refuse("last is neither 0 nor 1");
    const uint64_t taken = last ? n_text : n_text - n_text % DF_CHUNK;
    *n_taken = taken; *out_bytes = 0;
    if (n_members) *n_members = 0;
    uint64_t at = 0, members = 0;
    if (taken) {
        const int rc = bgzf_fixed(device_id, d_text, taken, sink, user, nullptr, "leon_text_bgzf_device", 0, &at, &members);
        if (rc) return rc;
    }
    if (last) {
        if (sink(user, at, kBgzfEof, sizeof kBgzfEof)) return dev_fail(LEON_E_SINK, "leon_text_bgzf_device: the sink returned non-zero");
        at += sizeof kBgzfEof;
    }
    *out_bytes = at;
    if (n_members) *n_members = members;
    return LEON_OK;
}

/* the same with members cut at record starts and the members' places; flags: which encoder */
static int bgzf_records_call(const std::string& who, int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body, const uint64_t* d_rec_off, uint64_t n_records,
                             int last, leon_piece_sink sink, void* user, uint64_t* n_taken, uint64_t* out_bytes, uint64_t* member_out_off, uint64_t* member_text_off,
                             uint64_t members_cap, uint64_t* n_members, uint32_t flags) {
    auto fail = [&](int code, const std::string& why) { return dev_fail(code, who + ": " + why); };
    constexpr uint64_t W = DF_CHUNK;
    if (!d_text && (n_head || n_body)) return fail(LEON_E_INVALID, "d_text is NULL with text given");
    if (!sink) return fail(LEON_E_INVALID, "sink is NULL");
    if (!n_taken) return fail(LEON_E_INVALID, "n_taken is NULL");
    if (!out_bytes) return fail(LEON_E_INVALID, "out_bytes is NULL");
    if (!n_members) return fail(LEON_E_INVALID, "n_members is NULL");
    if (flags & ~(uint32_t)LEON_BGZF_F_MATCHES) return fail(LEON_E_INVALID, "unknown bits in flags");
    if ((member_out_off == nullptr) != (member_text_off == nullptr) || (!member_out_off && members_cap)) return fail(LEON_E_INVALID, "bgzf records: a half-given member table");
    if (const char* why = bgzf_records_refusal(d_rec_off != nullptr, n_records, n_head, n_body, last)) return fail(LEON_E_INVALID, why);
    *n_taken = 0; *out_bytes = 0; *n_members = 0;
    const bool fixed = !d_rec_off && !n_head;                     // (and no records: refused above otherwise)
    const uint64_t n_text = n_head + n_body;
    BgzfIndex ix;
    ix.out = member_out_off; ix.text = member_text_off;
    uint64_t at = 0, members = 0, taken = 0;
    if (fixed) {
        taken = last ? n_text : n_text - n_text % W;
        const uint64_t need = (taken + W - 1) / W;
        if (ix.out && need > members_cap) { *n_members = need; return fail(LEON_E_OVERFLOW, "the member table needs " + std::to_string(need) + " entries"); }
        if (taken) {
            const int rc = bgzf_fixed(device_id, d_text, taken, sink, user, &ix, who, flags, &at, &members);
            if (rc) return rc;
        }
    } else if (d_rec_off || n_text) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) { (void)hipGetLastError(); return fail(LEON_E_NO_DEVICE, "no such HIP device"); }
        if (device_id >= DF_MAX_DEVICES) return fail(LEON_E_INVALID, "device ordinal beyond the scratch table");
        DEVCHK(hipSetDevice(device_id));
        BgzfScratch& S = bgzf_table()[device_id];
        std::lock_guard<std::mutex> lock(S.mu);
        S.device = device_id;
        CallStream st;
        if (const int rc = dev_stream(st)) return rc;
        hipStream_t s = st.s;
        DEVCHK(S.state.ensure(8 * 8));
        uint64_t h_state[5] = {0, 0, 0, 0, 0};
        if (d_rec_off) {                                          // the offsets are checked before anything is indexed with them
            uint32_t flags[3] = {0, 0, 0};
            DEVCHK(hipMemsetAsync(S.state.p, 0, sizeof flags, s));
            hipLaunchKernelGGL(k_bgzf_check_recs, dim3((uint32_t)((n_records + 1 + 255) / 256)), dim3(256), 0, s, d_rec_off, n_records, n_body, S.state.as<uint32_t>());
            DEVCHK(hipGetLastError());
            DEVCHK(hipMemcpyAsync(flags, S.state.p, sizeof flags, hipMemcpyDeviceToHost, s));
            DEVCHK(hipStreamSynchronize(s));
            if (const char* why = bgzf_offsets_refusal((flags[0] ? 1u : 0u) | (flags[1] ? 2u : 0u) | (flags[2] ? 4u : 0u))) return fail(LEON_E_INVALID, why);
        }
        const uint64_t n_starts = (n_head ? 1 : 0) + n_records + 1, bound = 3 * (n_text / W) + 2;
        auto cuts = [&](uint64_t k, uint64_t skip, uint64_t budget_end, uint64_t cap, uint64_t* begin, uint32_t* len) -> int {
            hipLaunchKernelGGL(k_bgzf_cuts, dim3(1), dim3(BGZF_CUT_T), 0, s, d_rec_off, n_starts, n_head, k, skip, budget_end, n_text, (uint32_t)last, cap, begin, len,
                               S.state.as<uint64_t>());
            DEVCHK(hipGetLastError());
            DEVCHK(hipMemcpyAsync(h_state, S.state.p, sizeof h_state, hipMemcpyDeviceToHost, s));
            DEVCHK(hipStreamSynchronize(s));
            return LEON_OK;
        };
        if (ix.out && members_cap < bound) {                      // a table that may be too small: found out before a byte is delivered, by one counting walk
            if (const int rc = cuts(0, 0, ~0ull, ~0ull, nullptr, nullptr)) return rc;
            if (h_state[0] > members_cap) { *n_members = h_state[0]; return fail(LEON_E_OVERFLOW, "the member table needs " + std::to_string(h_state[0]) + " entries"); }
        }
        const uint64_t slice = bgzf_slice_text();
        uint64_t k = 0, skip = 0;
        for (;;) {                                                // sequential: a slice ends at a cut, the next one begins there
            const uint64_t cap = 3 * (std::min(slice, n_text - taken) / W) + 4;
            DEVCHK(S.begin.ensure((cap + 1) * 8)); DEVCHK(S.len.ensure(cap * 4));
            if (const int rc = cuts(k, skip, taken + slice, cap, S.begin.as<uint64_t>(), S.len.as<uint32_t>())) return rc;
            const uint64_t n = h_state[0], end = h_state[3];
            if (n > cap || end < taken + n || end > n_text || h_state[1] >= n_starts || members + n > bound || (ix.out && members + n > members_cap))
                return fail(LEON_E_OVERFLOW, "the cut table does not add up");
            if (n) {
                uint64_t size = 0;
                const int rc = bgzf_members_out(S, device_id, s, d_text, n, taken, end, at, 0, sink, user, &ix, who, flags, &size);
                if (rc) return rc;
                at += size; members += n;
            }
            k = h_state[1]; skip = h_state[2]; taken = end;
            if (!n || !h_state[4]) break;
        }
        if (members > bound) return fail(LEON_E_OVERFLOW, "more members than 3 * (n_text / W) + 2");
        if (last && taken != n_text) return fail(LEON_E_OVERFLOW, "the cut table does not add up");
    }
    if (last) {
        if (sink(user, at, kBgzfEof, sizeof kBgzfEof)) return fail(LEON_E_SINK, "the sink returned non-zero");
        at += sizeof kBgzfEof;
    }
    *n_taken = taken; *out_bytes = at; *n_members = members;
    return LEON_OK;
}

extern "C" int leon_text_bgzf_records_device(int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body, const uint64_t* d_rec_off, uint64_t n_records, int last,
                                             leon_piece_sink sink, void* user, uint64_t* n_taken, uint64_t* out_bytes, uint64_t* member_out_off,
                                             uint64_t* member_text_off, uint64_t members_cap, uint64_t* n_members) {
    return bgzf_records_call("leon_text_bgzf_records_device", device_id, d_text, n_head, n_body, d_rec_off, n_records, last, sink, user, n_taken, out_bytes, member_out_off,
                             member_text_off, members_cap, n_members, 0);
}
extern "C" int leon_text_bgzf_device_ex(int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body, const uint64_t* d_rec_off, uint64_t n_records, int last,
                                        leon_piece_sink sink, void* user, uint64_t* n_taken, uint64_t* out_bytes, uint64_t* member_out_off, uint64_t* member_text_off,
                                        uint64_t members_cap, uint64_t* n_members, uint32_t flags) {
    return bgzf_records_call("leon_text_bgzf_device_ex", device_id, d_text, n_head, n_body, d_rec_off, n_records, last, sink, user, n_taken, out_bytes, member_out_off,
                             member_text_off, members_cap, n_members, flags);
}

/* the device buffers leon_qual_deflate_blocks_device keeps from call to call (about 1.5 GB after a large call) */
extern "C" void leon_qual_deflate_release(void) {
    int before = -1;
    const bool had_device = hipGetDevice(&before) == hipSuccess;
    for (int d = 0; d < DF_MAX_DEVICES; d++) {
        DeflateScratch& S = scratch(d);
        std::lock_guard<std::mutex> lock(S.mu);
        if (S.device >= 0 && hipSetDevice(S.device) == hipSuccess) S.drop();
        S.device = -1;
        std::vector<uint8_t>().swap(S.h);
        BgzfScratch& B = bgzf_table()[d];                        // (leon_text_bgzf_device's set goes with it)
        std::lock_guard<std::mutex> lock_b(B.mu);
        if (B.device >= 0 && hipSetDevice(B.device) == hipSuccess) B.drop();
        B.device = -1;
    }
    if (had_device) (void)hipSetDevice(before);
}
