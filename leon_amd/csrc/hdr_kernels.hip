// hdr_kernels.hip -- the header stream's symbols (gatb HeaderCoder.cpp HeaderEncoder [RECALLED lo]).
// Upstream codes headers per read block through the same RangeCoder, field by field against the previous header (the
// file's FIRST header at the start of every block, AbstractHeaderCoder::startBlock).  What a header contributes to the
// stream depends on the previous header's TEXT only, never on coder state, so the records of all headers of a batch
// are produced in parallel -- one lane per header, count pass / scan / emit pass like k_symbols -- and the per-block
// serial part is left to k_rc_encode (rc_kernels.hip) with this stream's model set.  The record layout is the one
// DESIGN.md section 1.3 states; the tests compare payload bytes with the CPU restatement of the same rules.
#include "ctx.h"
#include "prim.h"
#include "staging.h"
#include <cstring>

namespace leon {

namespace {

struct HField { uint32_t len, tok; uint32_t sep; bool has_sep; uint32_t kind, zeros; uint64_t value; };
enum : uint32_t { HK_ASCII = 0, HK_NUM = 1, HK_ZERO_ONLY = 2, HK_ZERO_NUM = 3 };

__device__ inline bool h_isalnum(uint32_t c) { return (c - '0') < 10u || ((c | 32u) - 'a') < 26u; }

// the field starting at h[pos] (pos < len): an alphanumeric run plus the one separator byte after it, classified in the same pass
__device__ inline HField h_field(const uint8_t* h, uint32_t len, uint32_t pos) {
    HField f; f.sep = 0; f.has_sep = false; f.kind = HK_ASCII; f.zeros = 0; f.value = 0;
    uint32_t e = pos, z = 0, sig = 0;
    bool digits = true, lead = true;
    uint64_t v = 0;
    while (e < len) {
        const uint32_t c = h[e];
        if (!h_isalnum(c)) { f.has_sep = true; f.sep = c; break; }
        const uint32_t d = c - '0';
        if (d < 10u) {
            if (lead && d == 0) z++; else { lead = false; if (sig < 18) v = v * 10 + d; sig++; }
        } else digits = false;
        e++;
    }
    f.tok = e - pos;
    f.len = f.tok + (f.has_sep ? 1u : 0u);
    if (digits && f.tok > 0 && !(f.has_sep && f.sep == 0)) {
        if (f.tok == 1 || z == 0) { if (f.tok <= 18) { f.kind = HK_NUM; f.value = f.tok == 1 ? (uint64_t)(h[pos] - '0') : v; } }
        else if (z == f.tok) { f.kind = HK_ZERO_ONLY; f.zeros = z; }
        else if (sig <= 18) { f.kind = HK_ZERO_NUM; f.zeros = z; f.value = v; }
    }
    return f;
}

struct HSink {
    uint16_t* p;          // nullptr: count only
    uint64_t n;
    __device__ inline void put(uint32_t model, uint32_t sym) { if (p) p[n] = (uint16_t)(model | (sym << 8)); n++; }
    __device__ inline void numeric(uint64_t v) {                    // CompressionUtils::encodeNumeric on _numericModels
        uint32_t bc = 1;
        while (bc < 8 && (v >> (8 * bc)) != 0) bc++;
        put(HM_NUMERIC0, bc);
        for (uint32_t b = 0; b < bc; b++) put(HM_NUMERIC0 + 1 + b, (uint32_t)(v >> (8 * b)) & 0xff);
    }
    __device__ inline void count(uint32_t model, uint64_t x) {
        if (x < 255) put(model, (uint32_t)x); else { put(model, 255); numeric(x - 255); }
    }
};

}  // namespace

// EMIT = false: sym_off[i] = number of symbols of header i; EMIT = true: the symbols at syms + 2 * sym_off[i].
template <bool EMIT>
__global__ void __launch_bounds__(256) k_hdr_symbols(const uint8_t* hdr, const uint64_t* off, uint64_t n, uint32_t rpb,
                                                    const uint8_t* first, uint32_t first_len, uint64_t* sym_off, uint8_t* syms) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* cur = hdr + off[i];
    const uint32_t lc = (uint32_t)(off[i + 1] - off[i]);
    const bool block_start = i % rpb == 0;                          // AbstractHeaderCoder::startBlock: previous = the file's first header
    const uint8_t* prev = block_start ? first : hdr + off[i - 1];
    const uint32_t lp = block_start ? first_len : (uint32_t)(off[i] - off[i - 1]);
    HSink S;
    S.p = EMIT ? (uint16_t*)syms + sym_off[i] : nullptr;
    S.n = 0;
    uint32_t pc = 0, pp = 0, fi = 0, fprev = 0;
    while (pc < lc) {
        const HField c = h_field(cur, lc, pc);
        const bool have_p = pp < lp;
        HField p; p.len = 0; p.kind = HK_ASCII; p.sep = 0; p.has_sep = false; p.value = 0; p.tok = 0; p.zeros = 0;
        uint32_t col = 0;
        bool same = false;
        if (have_p) {
            p = h_field(prev, lp, pp);
            const uint32_t m = c.len < p.len ? c.len : p.len;
            while (col < m && cur[pc + col] == prev[pp + col]) col++;
            same = col == c.len && c.len == p.len;
            fprev++;
        }
        if (!same) {
            if (c.kind == HK_NUM) {
                if (have_p && p.kind == HK_NUM && p.has_sep == c.has_sep && p.sep == c.sep && p.value != c.value) {
                    const bool up = c.value > p.value;
                    S.put(HM_TYPE, up ? H_FIELD_DELTA : H_FIELD_DELTA_2);
                    S.count(HM_FIELD_INDEX, fi);
                    S.numeric(up ? c.value - p.value : p.value - c.value);
                } else {
                    S.put(HM_TYPE, H_FIELD_NUMERIC);
                    S.count(HM_FIELD_INDEX, fi);
                    S.numeric(c.value);
                    S.put(HM_ASCII, c.has_sep ? c.sep : 0u);
                }
            } else if (c.kind != HK_ASCII) {
                S.put(HM_TYPE, c.kind == HK_ZERO_ONLY ? H_FIELD_ZERO_ONLY : H_FIELD_ZERO_AND_NUMERIC);
                S.count(HM_FIELD_INDEX, fi);
                S.count(HM_ZERO, c.zeros);
                if (c.kind == HK_ZERO_NUM) S.numeric(c.value);
                S.put(HM_ASCII, c.has_sep ? c.sep : 0u);
            } else {
                S.put(HM_TYPE, H_FIELD_ASCII);
                S.count(HM_FIELD_INDEX, fi);
                S.count(HM_FIELD_COLUMN, col);
                S.count(HM_MIS_SIZE, c.len - col);
                if (EMIT) { for (uint32_t j = col; j < c.len; j++) S.put(HM_ASCII, cur[pc + j]); }
                else S.n += c.len - col;
            }
        }
        pc += c.len; pp += p.len; fi++;
    }
    while (pp < lp) { pp += h_field(prev, lp, pp).len; fprev++; }
    if (fi >= fprev) S.put(HM_TYPE, H_END_MATCH);
    else { S.put(HM_TYPE, H_END); S.count(HM_FIELD_INDEX, fi); }
    if (!EMIT) sym_off[i] = S.n;
}

void launch_hdr_symbols(hipStream_t s, const uint8_t* hdr, const uint64_t* off, uint64_t n, uint32_t rpb, const uint8_t* first,
                        uint32_t first_len, uint64_t* sym_off, uint8_t* syms) {
    if (!n) return;
    const uint32_t g = (uint32_t)((n + 255) / 256);
    if (syms) hipLaunchKernelGGL(k_hdr_symbols<true>, dim3(g), dim3(256), 0, s, hdr, off, n, rpb, first, first_len, sym_off, syms);
    else hipLaunchKernelGGL(k_hdr_symbols<false>, dim3(g), dim3(256), 0, s, hdr, off, n, rpb, first, first_len, sym_off, syms);
}

}  // namespace leon

// ================================================================================================
// quality stream, lossy form (the default without -lossless): DnaEncoder::storeSolidCoverageInfo + smoothQuals
// [RECALLED med].  cover[i] = number of the read's k-mers that are in the bloom (canonical, N read as 'A') and span
// position i; a quality becomes '@' where cover[i] >= 2 (_smoothing_threshold) or where it is above '@' (truncation);
// reads shorter than k are left as they are.  One wave per read, lane = k-mer position (64 per step): the solid flags
// of a step are one ballot, and a position's coverage is a popcount over the k flags that span it.
// ================================================================================================
namespace leon {

// ---- the smoothing's bloom probes, shared between the reads of a locus ----
// In file order every k-mer of every read costs its random sectors (100 M reads: 1.1 s at the chip's rate; taking the reads in a
// better ORDER alone gives 7 %: a read's sectors are gone from L2 long before its neighbour is looked at).
// The walk shares probes because the reads of an anchor sit in neighbouring lanes and step through the same genome k-mers in the
// same instruction.  The same here, without the dictionary: every read is anchored on its MINIMIZER (its canonical k-mer of
// smallest hash); reads are sorted by it, one lane per read, and every lane goes through its k-mers outwards from the minimizer,
// one step to either side per iteration, the side towards the canonical k-mer's "right" first whatever the read's strand -- so at
// iteration g all reads that share a minimizer ask for the SAME genome k-mer, and identical addresses coalesce in the wave's own
// memory instruction.  The flags (k-mer solid or not, one bit per position) go to an array laid out like the N mask; a second,
// streaming kernel turns them into coverages and rewrites the qualities.  Measured at 100 M x 150 bp: 1 106 -> 580 ms, FETCH_SIZE
// 1.76 TB = 2.3 sectors per k-mer position; what is left is mostly the reads whose minimizer a sequencing error destroyed (a
// quarter of them at 1 % errors, k = 31): they land in clusters of their own, and the k-mers over errors, which no read shares.
template <typename K>
__global__ void __launch_bounds__(256) k_read_minimizer(ReadsDev R, uint32_t* key, uint32_t* mpos) {
    const uint32_t lane = lane_id(), k = R.k;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < R.n; i += nwaves) {
        const uint32_t len = R.len[i];
        if (len < k) { if (lane == 0) { key[i] = 0xFFFFFFFFu; mpos[i] = 0; } continue; }     // reads shorter than k: last, untouched
        const uint32_t nk = len - k + 1;
        const uint32_t* pk = R.packed + 2 * R.slot_off[i];
        uint64_t best = ~0ull;                                   // (hash << 32) | position: the smallest hash, its first position
        for (uint32_t base = 0; base < nk; base += 64) {
            const uint32_t p = base + lane;
            const K cn = canon_from_words<K>(pass_words(pk, base, lane), base, p < nk ? p : nk - 1, k);
            const uint64_t cand = ((uint64_t)(key_hash(cn) >> 33) << 32) | p;
            if (p < nk && cand < best) best = cand;
        }
        for (int d = 32; d; d >>= 1) {
            const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)best, d);
            best = o < best ? o : best;
        }
        if (lane == 0) {
            const uint32_t m = (uint32_t)best;
            const K km = kmer_at<K>(pk, m, k);
            const uint32_t fwd = km <= revcomp(km, k) ? 1u : 0u;   // the read carries the minimizer in its canonical orientation
            key[i] = (uint32_t)(best >> 32);
            mpos[i] = (m << 1) | fwd;
        }
    }
}

__global__ void k_mpos_from_anchors(ReadsDev R, const int32_t* anchor_pos, const uint32_t* anchor_addr, const uint8_t* flags, uint32_t* key, uint32_t* mpos) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < R.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t len = R.len[i], k = R.k;
        const int32_t a = anchor_pos[i];
        if (len < k) { key[i] = 0xFFFFFFFFu; mpos[i] = 0; }
        else if (a < 0 || (uint32_t)a > len - k) { key[i] = 0xFFFFFFFEu; mpos[i] = 1; }          // no (usable) anchor: on its own, from its first k-mer
        else { key[i] = anchor_addr[i]; mpos[i] = ((uint32_t)a << 1) | ((flags[i] & 1u) ? 0u : 1u); }   // flags bit 0: the anchor is reverse-complemented in the read
    }
}
void launch_mpos_from_anchors(hipStream_t s, ReadsDev R, const int32_t* anchor_pos, const uint32_t* anchor_addr, const uint8_t* flags, uint32_t* key, uint32_t* mpos) {
    if (!R.n) return;
    hipLaunchKernelGGL(k_mpos_from_anchors, dim3((uint32_t)std::min<uint64_t>((R.n + 255) / 256, 8192)), dim3(256), 0, s, R, anchor_pos, anchor_addr, flags, key, mpos);
}

template <typename K, uint32_t NH>       // NH: the bloom's number of hash functions when built for it (7), 0 = at run time (leon_device.h bloom_keys)
__global__ void __launch_bounds__(256) k_solid_flags(ReadsDev R, BloomDev B, const uint16_t* rv16g, const uint32_t* perm, const uint32_t* mpos,
                                                    uint32_t* flags) {
    __shared__ uint16_t rv16[256];
    load_rv16(rv16, rv16g, NH ? B.block_mask : 0xFFFFu);
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= R.n) return;
    const uint32_t i = perm[t], k = R.k, len = R.len[i];
    if (len < k) return;
    const uint32_t nk = len - k + 1, m = mpos[i] >> 1;
    const bool fwd = (mpos[i] & 1u) != 0;
    const uint32_t* pk = R.packed + 2 * R.slot_off[i];
    uint32_t* fl = flags + R.slot_off[i];
    const K mask = kmask<K>(k);
    const uint32_t top = 2 * (k - 1);
    // side P goes to higher positions, side M to lower ones; each keeps its k-mer, the reverse complement and a word of the read
    K xP = kmer_at<K>(pk, m, k), rP = revcomp(xP, k), xM = xP, rM = rP;
    uint32_t wP = 0, wP_idx = 0xFFFFFFFFu, wM = 0, wM_idx = 0xFFFFFFFFu;
    // flags collected per 32-position word and side, handed over when the side moves on to another word
    uint32_t aP = 0, aP_idx = m >> 5, aM = 0, aM_idx = m >> 5;
    if (bloom_contains_xr<K, NH>(B, rv16, xP, rP)) aP |= 1u << (m & 31);
    const uint32_t nP = nk - 1 - m, nM = m, nmax = nP > nM ? nP : nM;
    for (uint32_t g = 1; g <= nmax; g++) {
        // "A" = the side towards the canonical minimizer's right (P for a read that carries it forwards, M otherwise), "B" = the other
        const bool onP = g <= nP, onM = g <= nM;
        if (onP) {                                               // position m + g: the new last base is m + g + k - 1
            const uint32_t q = m + g + k - 1;
            if ((q >> 4) != wP_idx) { wP_idx = q >> 4; wP = pk[wP_idx]; }
            const uint32_t b = (wP >> (30 - 2 * (q & 15))) & 3u;
            xP = ((xP << 2) | (K)b) & mask;
            rP = (rP >> 2) | ((K)(b ^ 2u) << top);
        }
        if (onM) {                                               // position m - g: the new first base is m - g
            const uint32_t q = m - g;
            if ((q >> 4) != wM_idx) { wM_idx = q >> 4; wM = pk[wM_idx]; }
            const uint32_t b = (wM >> (30 - 2 * (q & 15))) & 3u;
            xM = (xM >> 2) | ((K)b << top);
            rM = ((rM << 2) | (K)(b ^ 2u)) & mask;
        }
        const bool onA = fwd ? onP : onM, onB = fwd ? onM : onP;
        // (both sides' first hashes in flight together, then the rest of both: measured, no different -- 487 against 471 ms; the
        // kernel is bound by its sectors, 1.76 TB at 100 M reads, not by their latency)
        const bool sA = onA && bloom_contains_xr<K, NH>(B, rv16, fwd ? xP : xM, fwd ? rP : rM);
        const bool sB = onB && bloom_contains_xr<K, NH>(B, rv16, fwd ? xM : xP, fwd ? rM : rP);
        const bool sP = fwd ? sA : sB, sM = fwd ? sB : sA;
        if (onP) {
            const uint32_t p = m + g;
            if ((p >> 5) != aP_idx) { if (aP) atomicOr(fl + aP_idx, aP); aP = 0; aP_idx = p >> 5; }
            if (sP) aP |= 1u << (p & 31);
        }
        if (onM) {
            const uint32_t p = m - g;
            if ((p >> 5) != aM_idx) { if (aM) atomicOr(fl + aM_idx, aM); aM = 0; aM_idx = p >> 5; }
            if (sM) aM |= 1u << (p & 31);
        }
    }
    if (aP) atomicOr(fl + aP_idx, aP);
    if (aM) atomicOr(fl + aM_idx, aM);
}

// coverages from the flags, qualities rewritten: one wave per read, lane = position (DnaEncoder::smoothQuals as restated in DESIGN 1.4)
__global__ void __launch_bounds__(256) k_qual_rewrite(ReadsDev R, const uint32_t* flags, uint8_t* quals) {
    const uint32_t lane = lane_id(), k = R.k;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < R.n; i += nwaves) {
        const uint32_t len = R.len[i];
        if (len < k) continue;
        const uint32_t* fl = flags + R.slot_off[i];
        uint8_t* q = quals + (R.base_off[i] - R.base_off[0]);
        unsigned long long prev = 0;                              // solid flags of k-mer positions [base - 64, base)
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t p = base + lane;
            // positions [base, base + 64): two words of the read's flag array (it has a word per 32-base slot; bits past the
            // last k-mer are zero)
            const uint32_t nw = (len + 31) >> 5, w0 = base >> 5;
            const unsigned long long cur = (unsigned long long)(w0 < nw ? fl[w0] : 0u) | ((unsigned long long)(w0 + 1 < nw ? fl[w0 + 1] : 0u) << 32);
            if (p < len) {
                const unsigned __int128 both = ((unsigned __int128)cur << 64) | prev;
                const uint32_t lo = lane + 65 - k;                // k <= 63: lo >= 2
                const unsigned __int128 win = (both >> lo) & ((((unsigned __int128)1) << k) - 1);
                const uint32_t cover = (uint32_t)__popcll((unsigned long long)win) + (uint32_t)__popcll((unsigned long long)(win >> 64));
                const uint8_t c = q[p];
                if (cover >= 2u || c > (uint8_t)'@') q[p] = (uint8_t)'@';
            }
            prev = cur;
        }
    }
}

// the smoothing in file order, every read probing for itself: small batches, and the measurement reference (LEON_QUAL_ORDER=0)
template <typename K>
__global__ void __launch_bounds__(256) k_qual_smooth(ReadsDev R, BloomDev B, const uint16_t* rv16g, uint8_t* quals) {
    __shared__ uint16_t rv16[256];
    load_rv16(rv16, rv16g);
    const uint32_t lane = lane_id(), k = R.k;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < R.n; i += nwaves) {
        const uint32_t len = R.len[i];
        if (len < k) continue;
        const uint32_t nk = len - k + 1;
        const uint32_t* pk = R.packed + 2 * R.slot_off[i];
        uint8_t* q = quals + (R.base_off[i] - R.base_off[0]);
        unsigned long long prev = 0;                              // solid flags of k-mer positions [base - 64, base)
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t p = base + lane;
            bool solid = false;
            const uint32_t kb = base < nk ? base : ((nk - 1) & ~63u);    // past the last k-mer only the coverage counts go on
            const K cn = canon_from_words<K>(pass_words(pk, kb, lane), kb, p < nk ? p : nk - 1, k);
            if (p < nk) solid = bloom_contains<K>(B, rv16, cn);
            const unsigned long long cur = __ballot(solid);
            if (p < len) {
                // k-mer positions spanning p: [p - k + 1, p] = bits [lane + 65 - k, lane + 64] of the 128 flags prev:cur
                const unsigned __int128 both = ((unsigned __int128)cur << 64) | prev;
                const uint32_t lo = lane + 65 - k;                // k <= 63: lo >= 2
                const unsigned __int128 win = (both >> lo) & ((((unsigned __int128)1) << k) - 1);
                const uint32_t cover = (uint32_t)__popcll((unsigned long long)win) + (uint32_t)__popcll((unsigned long long)(win >> 64));
                const uint8_t c = q[p];
                if (cover >= 2u || c > (uint8_t)'@') q[p] = (uint8_t)'@';
            }
            prev = cur;
        }
    }
}
static uint32_t wave_grid(uint64_t n) { uint64_t g = (n + 3) / 4; return (uint32_t)(g > 256 * 16 ? 256 * 16 : g); }
void launch_read_minimizer(hipStream_t s, ReadsDev R, uint32_t* key, uint32_t* mpos) {
    if (!R.n) return;
    if (R.k >= 32) hipLaunchKernelGGL(k_read_minimizer<u128>, dim3(wave_grid(R.n)), dim3(256), 0, s, R, key, mpos);
    else hipLaunchKernelGGL(k_read_minimizer<uint64_t>, dim3(wave_grid(R.n)), dim3(256), 0, s, R, key, mpos);
}
void launch_solid_flags(hipStream_t s, ReadsDev R, BloomDev B, const uint16_t* rv16, const uint32_t* perm, const uint32_t* mpos, uint32_t* flags) {
    if (!R.n) return;
    const uint32_t g = (uint32_t)((R.n + 255) / 256);
#define SF_LAUNCH(KT, NHV) hipLaunchKernelGGL((k_solid_flags<KT, NHV>), dim3(g), dim3(256), 0, s, R, B, rv16, perm, mpos, flags)
    if (R.k >= 32) { if (B.n_hash == 7) SF_LAUNCH(u128, 7); else SF_LAUNCH(u128, 0); }
    else { if (B.n_hash == 7) SF_LAUNCH(uint64_t, 7); else SF_LAUNCH(uint64_t, 0); }
#undef SF_LAUNCH
}
void launch_qual_rewrite(hipStream_t s, ReadsDev R, const uint32_t* flags, uint8_t* quals) {
    if (!R.n) return;
    hipLaunchKernelGGL(k_qual_rewrite, dim3(wave_grid(R.n)), dim3(256), 0, s, R, flags, quals);
}
void launch_qual_smooth(hipStream_t s, ReadsDev R, BloomDev B, const uint16_t* rv16, uint8_t* quals) {
    if (!R.n) return;
    if (R.k >= 32) hipLaunchKernelGGL(k_qual_smooth<u128>, dim3(wave_grid(R.n)), dim3(256), 0, s, R, B, rv16, quals);
    else hipLaunchKernelGGL(k_qual_smooth<uint64_t>, dim3(wave_grid(R.n)), dim3(256), 0, s, R, B, rv16, quals);
}

}  // namespace leon

// ---- the context's calls that end in this file's kernels, and the header decoders (ctx.h) ----
using namespace leon;

// A host batch to the device, for the entry points that take host memory: the offsets, rebased to begin at 0, in c->in_off and the
// bytes they span in c->in_bases.  nb: how many bytes that is.  (leon_dna_encode_batch has an upload of its own, staged and threaded.)
static int upload_host_batch(leon_dna_ctx* c, const uint8_t* bytes, const uint64_t* off, uint64_t n, uint64_t& nb) {
    if (off[n] < off[0]) return fail(c, LEON_E_INVALID, "offsets are not monotonic");
    HIPCHK(c, hipSetDevice(c->device));
    nb = off[n] - off[0];
    HIPCHK(c, c->in_bases.ensure(nb + 64)); HIPCHK(c, c->in_off.ensure((n + 1) * 8));
    HIPCHK(c, hipMemcpy(c->in_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice));
    if (off[0]) {
        launch_rebase_offsets(c->stream, c->in_off.as<uint64_t>(), n + 1, off[0]);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (nb) HIPCHK(c, hipMemcpy(c->in_bases.p, bytes + off[0], nb, hipMemcpyHostToDevice));
    return LEON_OK;
}

extern "C" {
// ------------------------------------------------------------------------------------------------ header stream
// Leon::startHeaderCompression: Dispatcher::iterate(bank, HeaderEncoder(this)) [RECALLED].  Records of every header
// against the previous one in parallel (hdr_kernels.hip), then the per-block chains on k_rc_encode with the header
// stream's model set; blocks leave through the sink in increasing id, like the DNA stream's.
static int header_batch_impl(leon_dna_ctx* c, const uint8_t* d_hdr, const uint64_t* d_off, uint64_t n, uint64_t first_read_index,
                             const uint8_t* first_header, uint64_t first_len, leon_block_sink sink, void* user) {
    if (!c) return LEON_E_INVALID;
    if (int rc = c->hdr.follows(c, first_read_index, n, "header stream")) return rc;
    if (n == 0) return LEON_OK;
    if (!d_hdr || !d_off || !sink || (!first_header && first_len)) return fail(c, LEON_E_INVALID, "null argument");
    if (n > 0xFFFFFFF0ull) return fail(c, LEON_E_INVALID, "more than 2^32 reads in one batch");
    if (first_len >= (1ull << 31)) return fail(c, LEON_E_INVALID, "first header longer than 2^31 bytes");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint32_t rpb = c->cfg.reads_per_block;
    // offsets must be an offsets array before anything indexes with them (headers below 2^31 bytes each)
    if (int rc = check_offsets(c, d_off, n, "a header is longer than 2^31 bytes", nullptr, false)) return rc;
    const Share sh = share_of(c, n);                            // this rank's share: the same contiguous block range as the DNA stream's
    if (sh.nl) {
        HIPCHK(c, c->hdr_first.ensure(first_len + 16));
        if (first_len) HIPCHK(c, hipMemcpyAsync(c->hdr_first.p, first_header, first_len, hipMemcpyHostToDevice, s));
        auto symbols = [&](uint8_t* syms) { launch_hdr_symbols(s, d_hdr, d_off + sh.r0, sh.nl, rpb, c->hdr_first.as<uint8_t>(), (uint32_t)first_len,
                                                                c->sym_off.as<uint64_t>(), syms); };
        CodedBlocks out;
        if (int rc = code_blocks(c, sh, symbols, SMALL_SIZES_HEADER, false, "header", out)) return rc;
        if (int rc = deliver_blocks(c, out, sh, n, c->hdr.next_block, sink, user)) return rc;
    }
    c->hdr.advance(n, rpb);
    return LEON_OK;
}

int leon_header_encode_batch_device(leon_dna_ctx* c, const uint8_t* d_headers, const uint64_t* d_off, uint64_t n, uint64_t first_read_index,
                                    const uint8_t* first_header, uint64_t first_header_len, leon_block_sink sink, void* user) {
    if (!c) return LEON_E_INVALID;
    if (c->poisoned) return refuse_poisoned(c);
    return note_poisoned(c, header_batch_impl(c, d_headers, d_off, n, first_read_index, first_header, first_header_len, sink, user));   // (a sink that refused a block)
}

int leon_header_encode_batch(leon_dna_ctx* c, const uint8_t* headers, const uint64_t* off, uint64_t n, uint64_t first_read_index,
                             const uint8_t* first_header, uint64_t first_header_len, leon_block_sink sink, void* user) {
    if (!c) return LEON_E_INVALID;
    if (n == 0) return leon_header_encode_batch_device(c, nullptr, nullptr, 0, first_read_index, first_header, first_header_len, sink, user);
    if (!headers || !off) return fail(c, LEON_E_INVALID, "null argument");
    uint64_t nb = 0;
    if (int rc = upload_host_batch(c, headers, off, n, nb)) return rc;
    return leon_header_encode_batch_device(c, c->in_bases.as<uint8_t>(), c->in_off.as<uint64_t>(), n, first_read_index, first_header,
                                           first_header_len, sink, user);
}

// ------------------------------------------------------------------------------------------------ quality stream (lossy)
// DnaEncoder::smoothQuals over a batch: the reads are packed as for the encode path, then one wave per read rewrites the
// qualities in place (hdr_kernels.hip k_qual_smooth).  Needs the file's bloom in the context.
int leon_qual_smooth_batch_device(leon_dna_ctx* c, const uint8_t* d_bases, const uint64_t* d_off, uint64_t n, uint8_t* d_quals) {
    if (!c) return LEON_E_INVALID;
    if (n == 0) return LEON_OK;
    if (!d_bases || !d_off || !d_quals) return fail(c, LEON_E_INVALID, "null argument");
    if (n > 0xFFFFFFF0ull) return fail(c, LEON_E_INVALID, "more than 2^32 reads in one batch");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    uint64_t n_slots = 0;
    if (int rc = check_offsets(c, d_off, n, "a read is longer than 2^31 bases", &n_slots, false)) return rc;
    if (int rc = ensure_pack_bufs(c, n, n_slots)) return rc;
    HIPCHK(c, hipMemsetAsync(c->packed.as<uint32_t>() + n_slots * 2, 0, 64, s));
    launch_pack(s, d_bases, d_off, c->slot_off.as<uint64_t>(), n, c->packed.as<uint32_t>(), c->nmask.as<uint32_t>(), c->rlen.as<uint32_t>(),
                c->ncount.as<uint32_t>());
    // large batches: the probes shared between the reads of a locus (hdr_kernels.hip) -- a minimizer per read, one sort, one lane per
    // read in that order, then the rewrite; small ones (and LEON_QUAL_ORDER=0, the measurement reference): every read for itself
    const char* qo = getenv("LEON_QUAL_ORDER");
    const bool in_file_order = qo && atoi(qo) == 0;
    const ReadsDev R = reads_view(c, d_off, n);
    if (!in_file_order && n >= 256) {
        HIPCHK(c, c->sort_key.ensure(n * 4)); HIPCHK(c, c->sort_key2.ensure(n * 4));
        HIPCHK(c, c->perm.ensure(n * 4)); HIPCHK(c, c->perm2.ensure(n * 4));
        HIPCHK(c, c->hit_pos.ensure(n * 4));                    // (the minimizers' positions; the encode's per-read arrays are free between batches)
        HIPCHK(c, c->events.ensure((n_slots + 4) * 4));         // (the flags)
        HIPCHK(c, hipMemsetAsync(c->events.p, 0, (n_slots + 4) * 4, s));
        // the reads of the batch this context encoded last (the CLI smooths a file right after its DNA stream): their ANCHORS are
        // at hand and serve better than minimizers -- a read with a sequencing error in its minimizer lands in a cluster of its
        // own, one with an error in an anchor k-mer simply has another anchor.  (Which k-mer a read is aligned on only decides
        // who shares probes with whom, never a flag: stale anchors would cost time, not bytes; positions are range-checked.)
        const bool anchors = n == c->last_n && d_bases == c->last_d_bases && d_off == c->last_d_off && c->shard_world == 1 && !c->poisoned;
        if (anchors) launch_mpos_from_anchors(s, R, c->anchor_pos.as<int32_t>(), c->anchor_addr.as<uint32_t>(), c->flags.as<uint8_t>(),
                                              c->sort_key.as<uint32_t>(), c->hit_pos.as<uint32_t>());
        else launch_read_minimizer(s, R, c->sort_key.as<uint32_t>(), c->hit_pos.as<uint32_t>());
        launch_iota(s, c->perm.as<uint32_t>(), n);
        auto sort = [&](void* t, size_t& b) { return prim::SortPairs(t, b, c->sort_key.as<uint32_t>(), c->sort_key2.as<uint32_t>(), c->perm.as<uint32_t>(), c->perm2.as<uint32_t>(), n, 0, 32, s); };
        if (int rc = run_prim(c, sort)) return rc;
        launch_solid_flags(s, R, c->B, c->rv16(), c->perm2.as<uint32_t>(), c->hit_pos.as<uint32_t>(), c->events.as<uint32_t>());
        launch_qual_rewrite(s, R, c->events.as<uint32_t>(), d_quals);
    } else launch_qual_smooth(s, R, c->B, c->rv16(), d_quals);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    return LEON_OK;
}

int leon_qual_smooth_batch(leon_dna_ctx* c, const uint8_t* bases, const uint64_t* off, uint64_t n, uint8_t* quals) {
    if (!c) return LEON_E_INVALID;
    if (n == 0) return LEON_OK;
    if (!bases || !off || !quals) return fail(c, LEON_E_INVALID, "null argument");
    uint64_t nb = 0;
    if (int rc = upload_host_batch(c, bases, off, n, nb)) return rc;
    OwnBuf dq;
    HIPCHK(c, dq.ensure(nb + 64));
    if (nb) HIPCHK(c, hipMemcpy(dq.p, quals + off[0], nb, hipMemcpyHostToDevice));
    if (int rc = leon_qual_smooth_batch_device(c, c->in_bases.as<uint8_t>(), c->in_off.as<uint64_t>(), n, dq.as<uint8_t>())) return rc;
    if (nb) HIPCHK(c, hipMemcpy(quals + off[0], dq.p, nb, hipMemcpyDeviceToHost));
    return LEON_OK;
}

// Header blocks: the symbols on the device (one wave per block, all blocks at once), the text on host threads
extern "C++" { namespace leon {                                // (host_streams.cpp)
int header_blocks_from_symbols(const uint8_t* syms, const uint64_t* sym_begin, const uint64_t* sym_count, const uint32_t* block_n_reads, uint64_t n_blocks,
                               const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                               uint64_t* out_size, uint32_t n_threads);
} }
struct leon_header_symbols {
    std::unique_ptr<uint8_t[]> syms;                             // every block's symbols, one byte each, block after block
    std::vector<uint64_t> begin, count;                          // block b: syms[begin[b] .. + count[b])
    bool overflowed = false;                                     // some block had more symbols than its share of the device buffer: decode the payloads on the host
};

// The front that the header decoders share: the payloads to the device, every block's share of the symbol buffer, the symbol
// kernel on the context's stream (not waited for), and -- hdr_symbols_wait -- its verdict.
struct HdrSymbolsDev {
    OwnBuf pay, begin, count, syms, err;
    BlockTableDev T;                                             // the payloads' places and reads per block
    std::vector<uint64_t> sym_begin;                             // block b's share: syms[sym_begin[b] .. sym_begin[b + 1])
};
static int hdr_symbols_launch(leon_dna_ctx* c, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads, uint64_t n_blocks, HdrSymbolsDev& D) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (int rc = block_table_to_device(c, payloads, payload_off, block_n_reads, n_blocks, D.pay, D.T)) return rc;
    // a block's share of the symbol buffer: enough for the headers sequencers write (a dozen symbols each); a block that
    // needs more (free text in every header) is left to the host decoder -- same result, its speed
    D.sym_begin.assign(n_blocks + 1, 0);
    for (uint64_t b = 0; b < n_blocks; b++)
        D.sym_begin[b + 1] = D.sym_begin[b] + 24ull * block_n_reads[b] + 6 * (payload_off[b + 1] - payload_off[b]) + 256;   // (SRA-style headers: 12-17 symbols, ~6 bytes each)
    const uint64_t sym_cap = D.sym_begin[n_blocks];
    HIPCHK(c, D.begin.ensure((n_blocks + 1) * 8)); HIPCHK(c, D.count.ensure(n_blocks * 8));
    HIPCHK(c, D.syms.ensure(sym_cap + 64)); HIPCHK(c, D.err.ensure(16));
    HIPCHK(c, hipMemcpyAsync(D.begin.p, D.sym_begin.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(D.err.p, 0, 16, s));
    launch_hdr_decode_symbols(s, D.pay.as<uint8_t>(), D.T.off.as<uint64_t>(), D.T.nreads.as<uint32_t>(), n_blocks, D.syms.as<uint8_t>(),
                              D.begin.as<uint64_t>(), (unsigned long long*)D.count.p, D.err.as<int>());
    HIPCHK(c, hipGetLastError());
    return LEON_OK;
}
// the kernel's err[0]: 0, 1 some block's symbols did not fit its share (`overflowed`), 2 block err[1] is not a header stream (refused here)
static int hdr_symbols_wait(leon_dna_ctx* c, HdrSymbolsDev& D, bool& overflowed) {
    int err[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(err, D.err.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err[0] == 2) return fail(c, LEON_E_INVALID, "header block " + std::to_string(err[1]) + " does not decode");
    overflowed = err[0] == 1;
    return LEON_OK;
}

int leon_header_decode_symbols(leon_dna_ctx* c, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads, uint64_t n_blocks,
                               leon_header_symbols** set) {
    if (!c) return LEON_E_INVALID;
    if (!set || (n_blocks && (!payloads || !payload_off || !block_n_reads))) return fail(c, LEON_E_INVALID, "null argument");
    *set = nullptr;
    std::unique_ptr<leon_header_symbols> H(new leon_header_symbols());
    H->begin.assign(n_blocks + 1, 0); H->count.assign(n_blocks, 0);
    if (!n_blocks) { *set = H.release(); return LEON_OK; }
    HdrSymbolsDev D;
    if (int rc = hdr_symbols_launch(c, payloads, payload_off, block_n_reads, n_blocks, D)) return rc;
    hipStream_t s = c->stream;
    if (int rc = hdr_symbols_wait(c, D, H->overflowed)) return rc;
    if (H->overflowed) { *set = H.release(); return LEON_OK; }
    HIPCHK(c, hipMemcpy(H->count.data(), D.count.p, n_blocks * 8, hipMemcpyDeviceToHost));
    // only the symbols that were written come back (a block's share is mostly empty)
    for (uint64_t b = 0; b < n_blocks; b++) H->begin[b + 1] = H->begin[b] + H->count[b];
    H->syms.reset(new uint8_t[H->begin[n_blocks] + 1]);
    for (uint64_t b = 0; b < n_blocks; b++)
        if (H->count[b]) HIPCHK(c, hipMemcpyAsync(H->syms.get() + H->begin[b], D.syms.as<uint8_t>() + D.sym_begin[b], H->count[b], hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *set = H.release();
    return LEON_OK;
}

int leon_header_text_from_symbols(const leon_header_symbols* H, uint64_t first_block, uint64_t n_blocks, const uint32_t* block_n_reads,
                                  const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                  uint64_t* out_size, uint32_t n_threads) {
    if (!H || !out_size || (n_blocks && (!block_n_reads || !out_off)) || (!first_header && first_header_len)) return dev_fail(LEON_E_INVALID, "null argument");
    *out_size = 0;
    if (first_block > H->count.size() || n_blocks > H->count.size() - first_block) return dev_fail(LEON_E_INVALID, "blocks beyond the symbol set");
    if (H->overflowed) return dev_fail(LEON_E_STATE, "the set's symbols did not fit the device buffer: decode the payloads with leon_host_header_decode_blocks");
    if (!n_blocks) return LEON_OK;
    return leon::header_blocks_from_symbols(H->syms.get(), H->begin.data() + first_block, H->count.data() + first_block, block_n_reads, n_blocks, first_header,
                                            first_header_len, out, out_cap, out_off, out_size, n_threads);
}

void leon_header_symbols_free(leon_header_symbols* H) { delete H; }

int leon_header_decode_blocks(leon_dna_ctx* c, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads, uint64_t n_blocks,
                              const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                              uint64_t* out_size, uint32_t n_threads) {
    if (!c) return LEON_E_INVALID;
    if (!out_size || (n_blocks && (!payloads || !payload_off || !block_n_reads || !out_off)) || (!first_header && first_header_len))
        return fail(c, LEON_E_INVALID, "null argument");
    *out_size = 0;
    if (!n_blocks) return LEON_OK;
    leon_header_symbols* H = nullptr;
    if (int rc = leon_header_decode_symbols(c, payloads, payload_off, block_n_reads, n_blocks, &H)) return rc;
    std::unique_ptr<leon_header_symbols> own(H);
    int rc;
    if (H->overflowed)                                           // more symbols than a block's share: the host decodes the payloads itself
        rc = leon_host_header_decode_blocks(payloads, payload_off, block_n_reads, n_blocks, first_header, first_header_len, out, out_cap, out_off, out_size, n_threads);
    else
        rc = leon_header_text_from_symbols(H, 0, n_blocks, block_n_reads, first_header, first_header_len, out, out_cap, out_off, out_size, n_threads);
    if (rc != LEON_OK) c->err = leon_last_error(nullptr);
    return rc;
}

// Header blocks, the text on the device too (k_hdr_text): what a set keeps, all of it in device memory
struct leon_header_text {
    int device = 0;
    OwnBuf text, off;                                            // every block's headers back to back; off[reads + 1], counted from text's first byte
    std::vector<uint64_t> text_begin, read0;                     // block b: text[text_begin[b] .. text_begin[b + 1]), off[read0[b] .. read0[b + 1]]
    std::vector<uint32_t> status;                                // HT_OK, or why the kernel declined the block (kernels.h)
    ~leon_header_text() { if (text.p || off.p) (void)hipSetDevice(device); }     // (for the members' release)
};

int leon_header_decode_text(leon_dna_ctx* c, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                            const uint64_t* block_text_bytes, uint64_t n_blocks, const uint8_t* first_header, uint64_t first_header_len,
                            leon_header_text** set) {
    if (!c) return LEON_E_INVALID;
    if (!set || (n_blocks && (!payloads || !payload_off || !block_n_reads)) || (!first_header && first_header_len)) return fail(c, LEON_E_INVALID, "null argument");
    *set = nullptr;
    std::unique_ptr<leon_header_text> T(new leon_header_text());
    T->device = c->device;
    T->text_begin.assign(n_blocks + 1, 0); T->read0.assign(n_blocks + 1, 0); T->status.assign(n_blocks, 0);
    if (!n_blocks) { *set = T.release(); return LEON_OK; }
    HdrSymbolsDev D;
    if (int rc = hdr_symbols_launch(c, payloads, payload_off, block_n_reads, n_blocks, D)) return rc;
    hipStream_t s = c->stream;
    for (uint64_t b = 0; b < n_blocks; b++) T->read0[b + 1] = T->read0[b] + block_n_reads[b];
    const uint64_t n_reads = T->read0[n_blocks];
    // a first header beyond the kernel's cap is not uploaded: every block is declined by its length alone
    const uint32_t first_len = (uint32_t)std::min<uint64_t>(first_header_len, (uint64_t)LEON_HT_HEADER_CAP + 1);
    OwnBuf d_first, d_read0, d_tbegin, d_status, d_tsize;
    HIPCHK(c, d_first.ensure(first_len + 64)); HIPCHK(c, d_read0.ensure((n_blocks + 1) * 8)); HIPCHK(c, d_tbegin.ensure((n_blocks + 1) * 8));
    HIPCHK(c, d_status.ensure(n_blocks * 4)); HIPCHK(c, d_tsize.ensure(n_blocks * 8));
    if (first_len) HIPCHK(c, hipMemcpyAsync(d_first.p, first_header, first_len, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_read0.p, T->read0.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice, s));
    auto text_kernel = [&](uint8_t* text, uint64_t* off) {
        launch_hdr_text(s, D.syms.as<uint8_t>(), D.begin.as<uint64_t>(), (const unsigned long long*)D.count.p, D.T.nreads.as<uint32_t>(), d_read0.as<uint64_t>(),
                        d_tbegin.as<uint64_t>(), n_blocks, d_first.as<uint8_t>(), first_len, text, off, d_status.as<uint32_t>(), d_tsize.as<uint64_t>());
    };
    std::vector<uint64_t> sizes;
    if (!block_text_bytes) {                                     // the sizing pass: the same chains, nothing written but the counts
        text_kernel(nullptr, nullptr);
        HIPCHK(c, hipGetLastError());
        sizes.resize(n_blocks);
        HIPCHK(c, hipMemcpyAsync(sizes.data(), d_tsize.p, n_blocks * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(T->status.data(), d_status.p, n_blocks * 4, hipMemcpyDeviceToHost, s));
        // what this pass refuses is refused here: in the pass that writes, a refused block has no share of the text, and a valid
        // header before its bad record would have it declined for that (HT_SHARE) before the record is reached
        bool overflowed = false;
        if (int rc = hdr_symbols_wait(c, D, overflowed)) return rc;
        for (uint64_t b = 0; b < n_blocks; b++)
            if (T->status[b] >= HT_INVALID) return fail(c, LEON_E_INVALID, "header block " + std::to_string(b) + " does not decode");
        block_text_bytes = sizes.data();
    }
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (block_text_bytes[b] > (1ull << 48)) return fail(c, LEON_E_INVALID, "header block " + std::to_string(b) + ": text size out of range");
        T->text_begin[b + 1] = T->text_begin[b] + block_text_bytes[b];
    }
    HIPCHK(c, T->text.ensure(T->text_begin[n_blocks] + 64)); HIPCHK(c, T->off.ensure((n_reads + 1) * 8));
    HIPCHK(c, hipMemcpyAsync(d_tbegin.p, T->text_begin.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(T->off.p, 0, 8, s));
    text_kernel(T->text.as<uint8_t>(), T->off.as<uint64_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(T->status.data(), d_status.p, n_blocks * 4, hipMemcpyDeviceToHost, s));
    bool overflowed = false;                                     // (such blocks carry their own status)
    if (int rc = hdr_symbols_wait(c, D, overflowed)) return rc;
    for (uint64_t b = 0; b < n_blocks; b++)
        if (T->status[b] >= HT_INVALID) return fail(c, LEON_E_INVALID, "header block " + std::to_string(b) + " does not decode");
    *set = T.release();
    return LEON_OK;
}

// blocks [b0, b0 + nb) of the set into out / out_off, the offsets counted from `at` (the run's first byte in the caller's text)
static int header_text_copy(const leon_header_text* T, uint64_t b0, uint64_t nb, uint8_t* out, uint64_t* out_off, uint64_t at) {
    const uint64_t t0 = T->text_begin[b0], size = T->text_begin[b0 + nb] - t0, r0 = T->read0[b0], nr = T->read0[b0 + nb] - r0;
    if (hipSetDevice(T->device) != hipSuccess) return dev_fail(LEON_E_HIP, "hipSetDevice");
    if (staged_d2h(T->device, out, T->text.as<uint8_t>() + t0, size) != hipSuccess) return dev_fail(LEON_E_HIP, "header text: copy to the host failed");
    if (staged_d2h(T->device, out_off, T->off.as<uint64_t>() + r0, (nr + 1) * 8) != hipSuccess) return dev_fail(LEON_E_HIP, "header offsets: copy to the host failed");
    if (at != t0) for (uint64_t i = 0; i <= nr; i++) out_off[i] = out_off[i] - t0 + at;
    return LEON_OK;
}
static int header_text_run(const leon_header_text* T, uint64_t first_block, uint64_t n_blocks) {
    if (first_block > T->status.size() || n_blocks > T->status.size() - first_block) return dev_fail(LEON_E_INVALID, "blocks beyond the text set");
    for (uint64_t b = first_block; b < first_block + n_blocks; b++)
        if (T->status[b]) return dev_fail(LEON_E_STATE, "header block " + std::to_string(b) + " was not built on the device (reason " + std::to_string(T->status[b]) +
                                      "): decode the payloads with leon_host_header_decode_blocks");
    return LEON_OK;
}

int leon_header_text_fetch(const leon_header_text* T, uint64_t first_block, uint64_t n_blocks, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint64_t* out_size) {
    if (!T || !out_size || (n_blocks && !out_off)) return dev_fail(LEON_E_INVALID, "null argument");
    *out_size = 0;
    if (int rc = header_text_run(T, first_block, n_blocks)) return rc;
    if (!n_blocks) return LEON_OK;
    const uint64_t size = T->text_begin[first_block + n_blocks] - T->text_begin[first_block];
    *out_size = size;
    if (size > out_cap || !out) return dev_fail(LEON_E_OVERFLOW, "header output needs " + std::to_string(size) + " bytes");
    return header_text_copy(T, first_block, n_blocks, out, out_off, 0);
}

int leon_header_text_device_ptr(const leon_header_text* T, uint64_t first_block, uint64_t n_blocks, const uint8_t** d_text, const uint64_t** d_off, uint64_t* size) {
    if (!T || !d_text || !d_off || !size) return dev_fail(LEON_E_INVALID, "null argument");
    *d_text = nullptr; *d_off = nullptr; *size = 0;
    if (int rc = header_text_run(T, first_block, n_blocks)) return rc;
    if (!T->text.p) return LEON_OK;                              // a set of no blocks
    *d_text = T->text.as<uint8_t>() + T->text_begin[first_block];
    *d_off = T->off.as<uint64_t>() + T->read0[first_block];
    *size = T->text_begin[first_block + n_blocks] - T->text_begin[first_block];
    return LEON_OK;
}

void leon_header_text_free(leon_header_text* T) { delete T; }

int leon_header_decode_blocks_device(leon_dna_ctx* c, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads, uint64_t n_blocks,
                                     const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                     uint64_t* out_size, uint32_t n_threads, uint64_t* n_blocks_on_host) {
    if (!c) return LEON_E_INVALID;
    if (!out_size || (n_blocks && (!payloads || !payload_off || !block_n_reads || !out_off)) || (!first_header && first_header_len))
        return fail(c, LEON_E_INVALID, "null argument");
    *out_size = 0;
    if (n_blocks_on_host) *n_blocks_on_host = 0;
    if (!n_blocks) return LEON_OK;
    leon_header_text* Tp = nullptr;
    if (int rc = leon_header_decode_text(c, payloads, payload_off, block_n_reads, nullptr, n_blocks, first_header, first_header_len, &Tp)) return rc;
    std::unique_ptr<leon_header_text> T(Tp);
    // the blocks the kernel declined, run by run, through the host decoder from their payloads
    struct HostRun { uint64_t b0, nb; std::vector<uint8_t> text; std::vector<uint64_t> off; uint64_t size; };
    std::vector<HostRun> runs;
    uint64_t on_host = 0;
    for (uint64_t b = 0; b < n_blocks;) {
        if (!T->status[b]) { b++; continue; }
        HostRun R; R.b0 = b;
        while (b < n_blocks && T->status[b]) b++;
        R.nb = b - R.b0; on_host += R.nb;
        R.off.assign(T->read0[R.b0 + R.nb] - T->read0[R.b0] + 1, 0);
        R.text.resize((payload_off[R.b0 + R.nb] - payload_off[R.b0]) * 8 + 4096);
        auto decode = [&](uint64_t b0, uint64_t nb) {
            return leon_host_header_decode_blocks(payloads, payload_off + b0, block_n_reads + b0, nb, first_header, first_header_len, R.text.data(), R.text.size(),
                                                  R.off.data(), &R.size, n_threads);
        };
        int rc = decode(R.b0, R.nb);
        if (rc == LEON_E_OVERFLOW) { R.text.resize(R.size + 1); rc = decode(R.b0, R.nb); }
        if (rc == LEON_E_INVALID && R.nb > 1) {                  // (the host decoder counts from the run's first block: name the block by its place in the call)
            for (uint64_t k = 0; k < R.nb; k++)
                if (decode(R.b0 + k, 1) == LEON_E_INVALID) return fail(c, LEON_E_INVALID, "header block " + std::to_string(R.b0 + k) + " does not decode");
        }
        if (rc == LEON_E_INVALID) return fail(c, LEON_E_INVALID, "header block " + std::to_string(R.b0) + " does not decode");
        if (rc != LEON_OK) { c->err = leon_last_error(nullptr); return rc; }
        runs.push_back(std::move(R));
    }
    if (n_blocks_on_host) *n_blocks_on_host = on_host;
    uint64_t total = T->text_begin[n_blocks];
    for (const HostRun& R : runs) total += R.size;
    *out_size = total;
    if (total > out_cap || !out) return fail(c, LEON_E_OVERFLOW, "header output needs " + std::to_string(total) + " bytes");
    uint64_t at = 0, b = 0;
    size_t next_run = 0;
    out_off[0] = 0;
    while (b < n_blocks) {
        uint64_t* o = out_off + T->read0[b];
        if (next_run < runs.size() && runs[next_run].b0 == b) {
            const HostRun& R = runs[next_run++];
            if (R.size) memcpy(out + at, R.text.data(), R.size);
            for (size_t i = 0; i < R.off.size(); i++) o[i] = at + R.off[i];
            at += R.size; b += R.nb;
        } else {
            const uint64_t e = next_run < runs.size() ? runs[next_run].b0 : n_blocks;
            if (int rc = header_text_copy(T.get(), b, e - b, out + at, o, at)) { c->err = leon_last_error(nullptr); return rc; }
            at += T->text_begin[e] - T->text_begin[b]; b = e;
        }
    }
    return LEON_OK;
}
}  // extern "C"
