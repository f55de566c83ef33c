// rc_kernels.hip -- block-parallel order-0 adaptive range coder (gatb RangeCoder.cpp: Order0Model,
// RangeEncoder::encode / flush [RECALLED]).  The models reset per read block, so blocks are the only
// independent streams the format has.  A workgroup takes a group of up to 8 blocks, software-pipelined over tiles of 64 symbols:
//   one modeler wave per block (lane = symbol): every symbol's (cumLow, freq, total) from the model state at the tile
//     start plus the earlier symbols of the tile, then Order0Model::update for the tile, then the reciprocal of total;
//   one coder wave per group (lane = block): the serial chains
//     range /= total; low += cumLow*range; range *= freq; renormalise
//     with one multiply-high by the precomputed reciprocal instead of a 64-bit division.
// Counts are exactly Order0Model's cumulative counts (its rescale cannot trigger: MAX_RANGE = 2^48 total).
#include "ctx.h"
#include "rc_model.h"
#include "prim.h"
#include <atomic>
#include <cstring>
#include <mutex>
#include <thread>

namespace leon {

size_t rc_model_scratch_bytes(uint64_t n_blocks) {
    return (size_t)n_blocks * (RC_NNUM - RC_NSLOT_SMALL) * RC_STRIDE * sizeof(uint32_t);
}

// Waves of a workgroup land on the CU's four SIMDs round-robin.  Wave 0 is the coder; the waves whose index is a multiple
// of 4 would share its SIMD and stay idle (they only keep the barriers), so the chain never waits for a modeler's
// vector instruction; the other waves are the modelers.
__host__ __device__ constexpr uint32_t rc_waves(uint32_t g) { return g + 1 + (g - 1) / 3; }

// The earlier symbols of a tile, lane = symbol: lo += #(same model, smaller symbol), hi += #(same model, symbol <= mine),
// tot += #(same model) over the lanes before this one -- 64 steps of a broadcast and three compare/add-with-carry pairs; the lane
// mask "after lane i" is exec itself, shifted once per step (one asm block, exec restored inside it).  key = model << 8 | symbol.
__device__ inline void rc_rank_loop(uint32_t key, uint32_t c, uint32_t& lo, uint32_t& hi, uint32_t& tot) {
    const uint32_t lowkey = key & ~0xFFu;
    uint32_t sk0, sk1, dd;
    uint64_t m1, m2, sav;
    asm volatile(
        "s_mov_b64 %[sav], exec\n\t"
        "v_readlane_b32 %[sk0], %[key], 0\n\t"
        "s_mov_b64 exec, -2\n\t"
        "s_nop 1\n\t"
        ".set rc_i, 0\n\t"
        ".rept 32\n\t"
        "v_sub_u32 %[dd], %[sk0], %[lowkey]\n\t"
        "v_readlane_b32 %[sk1], %[key], rc_i + 1\n\t"
        "v_cmp_lt_u32 vcc, %[dd], %[c]\n\t"
        "v_cmp_le_u32 %[m1], %[dd], %[c]\n\t"
        "v_cmp_gt_u32 %[m2], %[k256], %[dd]\n\t"
        "v_addc_co_u32 %[lo], vcc, 0, %[lo], vcc\n\t"
        "v_addc_co_u32 %[hi], %[m1], 0, %[hi], %[m1]\n\t"
        "v_addc_co_u32 %[tot], %[m2], 0, %[tot], %[m2]\n\t"
        "s_lshl_b64 exec, exec, 1\n\t"
        "v_sub_u32 %[dd], %[sk1], %[lowkey]\n\t"
        "v_readlane_b32 %[sk0], %[key], (rc_i + 2) & 63\n\t"
        "v_cmp_lt_u32 vcc, %[dd], %[c]\n\t"
        "v_cmp_le_u32 %[m1], %[dd], %[c]\n\t"
        "v_cmp_gt_u32 %[m2], %[k256], %[dd]\n\t"
        "v_addc_co_u32 %[lo], vcc, 0, %[lo], vcc\n\t"
        "v_addc_co_u32 %[hi], %[m1], 0, %[hi], %[m1]\n\t"
        "v_addc_co_u32 %[tot], %[m2], 0, %[tot], %[m2]\n\t"
        "s_lshl_b64 exec, exec, 1\n\t"
        ".set rc_i, rc_i + 2\n\t"
        ".endr\n\t"
        "s_mov_b64 exec, %[sav]\n\t"
        : [lo] "+v"(lo), [hi] "+v"(hi), [tot] "+v"(tot), [sk0] "=&s"(sk0), [sk1] "=&s"(sk1), [dd] "=&v"(dd),
          [m1] "=&s"(m1), [m2] "=&s"(m2), [sav] "=&s"(sav)
        : [key] "v"(key), [lowkey] "v"(lowkey), [c] "v"(c), [k256] "s"(256u)
        : "vcc");
}

// The modeler of ONE block, run by one wave (lane = symbol of the current tile of 64): the adaptive order-0 models of the block in
// LDS (two-level cumulative counts, rc_model.h; numeric models beyond the LDS slots in a global overflow area), and per tile every
// symbol's (cumLow, cumLow + freq, total) = the counts at the tile start + the earlier symbols of the tile, then
// Order0Model::update for the whole tile.  Used by the block coder below (records into an LDS ring for the coder wave) and by
// k_rc_records (records into global memory for host chains).
// CMP: a numeric group's byte-COUNT model (encodeNumeric's first symbol: 0..8 of its 256) keeps to the small layout in a place of its own
// -- Lw[x] = F(x) for x <= 16, total = F(16) + 240 -- so the slots, 280 words each, serve the byte models only: the nine or ten of them a
// read set uses all the time then fit the 12 a workgroup of 8 blocks has room for, and nothing hot is left to the global overflow area.
template <uint32_t RC_NSLOT, bool CMP>
struct RcModeler {
    static constexpr uint32_t SLOT_BASE = RC_SMALL_WORDS + (CMP ? RC_CMP_WORDS : 0);
    static constexpr uint32_t WORDS = SLOT_BASE + RC_NSLOT * RC_STRIDE;
    uint32_t* models; uint8_t* slotmap; uint32_t* gmodels; const uint16_t* sym16; int* err;
    uint64_t s0, s1;
    uint32_t nused, raw_next, small_sizes;
    // per-lane constants of the branch-free Order0Model::update of the overflow area: lanes 0..15 own Lw of the symbol's 16-block,
    // lanes 16..32 own H[0..16]
    bool is_lw; uint32_t upd_lane, upd_base, upd_blkmask;

    __device__ inline void init(uint32_t* models_, uint8_t* slotmap_, const uint16_t* sym16_, uint32_t small_sizes_, uint32_t lane, int* err_) {
        models = models_; slotmap = slotmap_; sym16 = sym16_; small_sizes = small_sizes_; err = err_;
        is_lw = lane < 16;
        upd_lane = is_lw ? lane : (lane < 33 ? lane - 16 : 0);
        upd_base = is_lw ? RC_LW + lane : upd_lane;
        upd_blkmask = is_lw ? ~0u : 0u;
        nused = 0; raw_next = 0xFFFFu; s0 = s1 = 0; gmodels = nullptr;
    }
    // AbstractDnaCoder::startBlock: the block's symbols are [s0_, s1_); the next tile's symbols are fetched one tile ahead
    // (a global load costs ~2000 cycles)
    __device__ inline void start_block(uint64_t s0_, uint64_t s1_, uint32_t* gmodels_, uint32_t lane) {
        s0 = s0_; s1 = s1_; gmodels = gmodels_; nused = 0;
        raw_next = lane < (uint32_t)((s1 - s0) < 64 ? (s1 - s0) : 64) ? sym16[s0 + lane] : 0xFFFFu;
        for (uint32_t m = 0; m < N_SMALL_MODELS + (CMP ? N_NUM_GROUPS : 0); m++) model_init(&models[m * RC_SSTRIDE], lane, true);
        for (uint32_t i = lane; i < RC_NNUM; i += 64) slotmap[i] = 255;
    }
    // tile t of the block: this lane's record (lanes past the block's end: cumLow 0, freq = total = 1, which leaves a chain as it is)
    __device__ inline void tile(uint32_t t, uint32_t lane, uint32_t& lo, uint32_t& hi, uint32_t& tot) {
        const uint64_t base = s0 + (uint64_t)t * 64;
        const uint32_t cnt = (uint32_t)((s1 - base) < 64 ? (s1 - base) : 64);
        const bool act = lane < cnt;
        const uint32_t raw = raw_next;
        {
            const uint64_t nb = base + 64;
            raw_next = (nb < s1 && lane < (uint32_t)((s1 - nb) < 64 ? (s1 - nb) : 64)) ? sym16[nb + lane] : 0xFFFFu;
        }
        const uint32_t m = raw & 0xff;
        const uint32_t grp = ((m - N_SMALL_MODELS) * 57u) >> 9;       // (m - 8) / 9 for the 72 numeric ids
        const bool cmodel = CMP && act && m >= N_SMALL_MODELS && (m - N_SMALL_MODELS) == grp * MODELS_PER_NUMERIC;
        uint32_t c = raw >> 8;
        if (CMP && __builtin_expect(__ballot(cmodel && c > 8u) != 0, 0)) {     // not from k_symbols (a value has at most 8 bytes): the launch fails, nothing is written out of place
            if (lane == 0) atomicExch(err, 3);
            if (cmodel && c > 8u) c = 8u;
        }
        const uint32_t key = (m << 8) | c;
        const bool numeric = act && m >= N_SMALL_MODELS && !cmodel;
        // slots for numeric models first seen in this tile
        uint32_t slot = numeric ? slotmap[m - N_SMALL_MODELS] : 0;
        unsigned long long need = __ballot(numeric && slot == 255);
        while (need) {
            const uint32_t l = (uint32_t)__builtin_ctzll(need);
            const uint32_t mm = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)l);
            const uint32_t ns = nused++;
            if (lane == 0) slotmap[mm - N_SMALL_MODELS] = (uint8_t)ns;
            if (ns < RC_NSLOT) model_init(&models[SLOT_BASE + ns * RC_STRIDE], lane, false);
            else { model_init(gmodels + (uint64_t)(ns - RC_NSLOT) * RC_STRIDE, lane, false); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
            if (numeric && m == mm) slot = ns;
            need &= ~__ballot(numeric && m == mm);
        }
        // word offset of this lane's model (RC_GLOBAL | offset for the overflow area)
        uint32_t mb = 0;
        if (act) mb = cmodel ? RC_SMALL_WORDS + grp * RC_SSTRIDE
                    : !numeric ? m * RC_SSTRIDE
                               : (slot < RC_NSLOT ? SLOT_BASE + slot * RC_STRIDE : (RC_GLOBAL | ((slot - RC_NSLOT) * RC_STRIDE)));
        const uint32_t tot_idx = numeric ? 16u : RC_LW + (cmodel ? 16u : small_size_of(small_sizes, m));
        __builtin_amdgcn_wave_barrier();
        // counts at the tile start
        lo = 0; hi = 1; tot = 1;
        if (act) {
            if (!(mb & RC_GLOBAL)) {
                const uint32_t* s = &models[mb];
                lo = s[c >> 4] + s[RC_LW + c]; hi = s[(c + 1) >> 4] + s[RC_LW + c + 1]; tot = s[tot_idx] + (cmodel ? 240u : 0u);
            } else {
                const uint32_t* s = gmodels + (mb & ~RC_GLOBAL);
                lo = s[c >> 4] + s[RC_LW + c]; hi = s[(c + 1) >> 4] + s[RC_LW + c + 1]; tot = s[tot_idx];
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // earlier symbols of the tile: lo += #(same model, smaller symbol), hi += #(same model, symbol <= mine),
        // tot += #(same model) over the lanes before this one -- 64 steps of a broadcast and three
        // compare/add-with-carry pairs; the lane mask "after lane i" is exec itself, shifted once per step
        // (one asm block, exec restored inside it)
        rc_rank_loop(key, c, lo, hi, tot);
        {
            if (!act) { lo = 0; hi = 1; tot = 1; }         // past the block's end: a record that leaves the chain as it is
        }
        // Order0Model::update for the whole tile, lane = symbol: F(x) += 1 for x > c, i.e. H[k] for k > c >> 4
        // and Lw[x] for the x after c inside c's 16-block (adds of 0 where it does not apply: no exec juggling)
        {
            // (only the lanes an add applies to take part: same-address adds serialise in the LDS, and with 8
            // modelers per CU its atomic unit is the busiest part of the kernel.  A small model's total is
            // read from Lw[size], so its H[] is never touched)
            const bool in_lds = act && !(mb & RC_GLOBAL);
            uint32_t* mp = &models[in_lds ? mb : 0];
            const uint32_t h4 = (in_lds && numeric) ? c >> 4 : 64u;
            const uint32_t l4 = in_lds ? c & 15u : 64u, ymax = numeric ? 15u : (cmodel ? 16u : small_size_of(small_sizes, m));
            uint32_t* lp = mp + RC_LW + (in_lds ? (c & ~15u) : 0u);
#pragma unroll
            for (uint32_t k = 1; k <= 16; k++)
                if (k > h4) (void)__hip_atomic_fetch_add(&mp[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#pragma unroll
            for (uint32_t y = 1; y <= (CMP ? 16u : 15u); y++)
                if (y > l4 && y <= ymax) (void)__hip_atomic_fetch_add(&lp[y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            // symbols of models that live in the global overflow area: one at a time, lanes 0..32 own the entries
            unsigned long long gl = __ballot(act && (mb & RC_GLOBAL));
            while (gl) {
                const uint32_t i = (uint32_t)__builtin_ctzll(gl);
                gl &= gl - 1;
                const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)i);
                const uint32_t mbi = (uint32_t)__builtin_amdgcn_readlane((int)mb, (int)i);
                const uint32_t thr = is_lw ? (ci & 15u) : (ci >> 4);
                const uint32_t idx = upd_base + ((ci & ~15u) & upd_blkmask);
                if (upd_lane > thr)
                    (void)__hip_atomic_fetch_add(gmodels + (mbi & ~RC_GLOBAL) + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
};

// The coder's 64 steps of one tile, lane = block: RangeEncoder::encode for every record of the tile.  EXACT: the quotient by a
// 64-bit division (totals of 2^30 and more); else a truncated multiply-high by the total's reciprocal with a 32-bit fix-up.
template <bool EXACT>
__device__ inline void rc_coder_tile(const uint4* ra, const uint2* rb, uint64_t& low, uint64_t& range, uint32_t& nout, uint8_t* dst, uint32_t cap) {
    // the record TWO steps on is fetched under this step (one step ahead the coder still waited for the LDS now and then: 122.6 -> 118.9 ms
    // at 100 M reads, 175 -> 167 at the k = 63 shape; three ahead is slower again; the row's 65th entry is a spare)
    uint4 pa = ra[0], pa1 = ra[1];
    uint2 pb = rb[0], pb1 = rb[1];
#pragma clang loop unroll_count(EXACT ? 1 : 4)
    for (uint32_t j = 0; j < 64; j++) {
        const uint32_t s_lo = pa.x, s_fr = pa.y, s_tot = pa.z, s_hc = pa.w, b0 = pb.x, b1 = pb.y;
        const uint32_t jn = j + 2 < 64 ? j + 2 : 64;
        pa = pa1; pb = pb1; pa1 = ra[jn]; pb1 = rb[jn];
        // low += cumLow * q; range = q * freq; top = low + range = low + q * (cumLow + freq), q = floor(range / total)
        // (a third product and not `low + range`: the add waits for both products; profiles/r4_minimizer_filter.txt)
        uint64_t top;
        if (EXACT) {
            const uint64_t q = range / (uint64_t)s_tot;
            const uint32_t q0 = (uint32_t)q, q1 = (uint32_t)(q >> 32);
            top = (uint64_t)q0 * s_hc + low;   top += (uint64_t)(q1 * s_hc) << 32;
            low = (uint64_t)q0 * s_lo + low;   low += (uint64_t)(q1 * s_lo) << 32;
            range = (uint64_t)q0 * s_fr;       range += (uint64_t)(q1 * s_fr) << 32;
        } else {
            // The step is as long as its DEPENDENT path (a lone wave issues in order; round 5: leaving instructions out of the step changed
            // nothing, an emitter wave's four and the modelers' updates alike -- DESIGN.md 4.3).  The quotient is a truncated multiply-high by the total's
            // reciprocal, at most 3 short (total < 2^30); the three products start from that estimate while the remainder is compared, and
            // the 0..3 it was short by goes into each with one multiply-add -- two levels fewer than fixing the quotient first.
            const uint32_t r0 = (uint32_t)range, r1 = (uint32_t)(range >> 32);
            uint64_t qe = (uint64_t)r1 * b1 + __umulhi(r1, b0);
            qe += __umulhi(r0, b1);
            const uint32_t q0 = (uint32_t)qe, q1 = (uint32_t)(qe >> 32);
            uint64_t T0 = (uint64_t)q0 * s_hc + low;   T0 += (uint64_t)(q1 * s_hc) << 32;
            uint64_t L0 = (uint64_t)q0 * s_lo + low;   L0 += (uint64_t)(q1 * s_lo) << 32;
            uint64_t R0 = (uint64_t)q0 * s_fr;         R0 += (uint64_t)(q1 * s_fr) << 32;
            asm volatile("" : "+v"(T0), "+v"(L0), "+v"(R0));        // (as written: the compiler would fold the fix-up back into the quotient)
            const uint32_t rem = r0 - q0 * s_tot;                   // true remainder < 4 * tot < 2^32
            const uint32_t t2 = s_tot << 1, t3 = t2 + s_tot;
            uint32_t e = (rem >= s_tot ? 1u : 0u) + (rem >= t2 ? 1u : 0u) + (rem >= t3 ? 1u : 0u);
            asm volatile("" : "+v"(e));
            top = (uint64_t)e * s_hc + T0;
            low = (uint64_t)e * s_lo + L0;
            range = (uint64_t)e * s_fr + R0;
        }
        // RangeEncoder::encode's while loop.  Usual case: low and low + range agree on their top 0..3
        // bytes and the shifted range stays >= BOTTOM: those bytes leave at once -- one unaligned 4-byte
        // store at the cursor (what lies past the cursor is overwritten by the stores that follow)
        const uint32_t lh = (uint32_t)(low >> 32);
        uint32_t xh = lh ^ (uint32_t)(top >> 32);
        uint32_t lead;                                              // v_ffbh_u32 answers -1 for 0: & 24 = 24 either way, without the `| 1` a level before it
        asm("v_ffbh_u32 %0, %1" : "=v"(lead), "+v"(xh));            // (xh in and out: the compiler would widen `xh == 0` below to a 64-bit compare of low ^ top)
        const uint32_t sh = lead & 24u;
        const uint64_t range_s = range << sh;
        // rare: four bytes or more leave, or the shifted range is below BOTTOM (one compare: the branch waits for it)
        uint32_t rare_below = xh == 0u ? 0xFFFFFFFFu : 0xFFFFu;
        asm volatile("" : "+v"(rare_below));
        const bool rare = (uint32_t)(range_s >> 32) <= rare_below;
        {
            const uint32_t cap4 = cap - 4;                          // (stores clamp to the block's room; the block reports overflow at its end)
            *(uint32_t*)(dst + (nout < cap4 ? nout : cap4)) = __builtin_bswap32(lh);
        }
        uint64_t low_n = low << sh, range_n = range_s;
        uint32_t nout_n = nout + (sh >> 3);
        // (the rare case is ONE scalar branch on "any lane", not an exec mask saved and restored around the lanes' own test)
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0, 0) && rare) {
            // RangeEncoder::encode's loop as it is written
            low_n = low; range_n = range; nout_n = nout;
            while ((low_n ^ (low_n + range_n)) < (1ull << 56) ||
                   (range_n < RC_BOTTOM && ((range_n = (0 - low_n) & (RC_BOTTOM - 1)), true))) {
                if (nout_n < cap) dst[nout_n] = (uint8_t)(low_n >> 56);
                nout_n++;
                range_n <<= 8;
                low_n <<= 8;
            }
        }
        low = low_n; range = range_n; nout = nout_n;
    }
}

// One workgroup codes G blocks: G modeler waves, and one coder wave that runs the G serial chains
// in its lanes 0..G-1 (lane = block).  A chain step costs the same issue slots whether one lane or eight are active, so
// a CU that holds 8 blocks runs ONE chain instruction stream instead of eight; the step itself is branch-free in the
// usual cases (0..2 bytes leave, no range < BOTTOM reset) and falls back to RangeEncoder::encode's loop per lane otherwise.
// BIGOK: some block of the launch is long enough for a model's total to reach 2^30 (the host knows the blocks' symbol counts):
// that instantiation also carries the exact-division steps, tile by tile; the other one is the plain fast chain.
template <uint32_t G, uint32_t RC_NSLOT, bool BIGOK, bool CMP>
__global__ void __launch_bounds__(64 * rc_waves(G)) k_rc_encode(const uint8_t* syms, const uint64_t* blk_begin, uint64_t n_blocks,
                                                            uint8_t* out, const uint64_t* out_off, uint64_t* out_size,
                                                            uint32_t* scratch, int* err, uint32_t small_sizes, uint32_t fast_total) {
    constexpr uint32_t MW = RcModeler<RC_NSLOT, CMP>::WORDS;
    __shared__ uint32_t models_all[G * MW];
    // a step's record: {cumLow, freq, total, cumLow + freq} and the total's 64-bit reciprocal -- two LDS reads for the coder (its
    // step is paid in issue slots); one spare entry per row: the coder prefetches record j + 1
    __shared__ uint4 ring_a[G][2][RC_RING];
    __shared__ uint2 ring_b[G][2][RC_RING];
    __shared__ uint8_t slotmap_all[G][RC_NNUM];
    __shared__ uint32_t ntiles_s[G];
    __shared__ uint32_t tile_big[BIGOK ? G : 1][2];              // a total of fast_total or more in the tile: the coder divides exactly
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool is_coder = wave == 0, is_idle = wave != 0 && (wave & 3u) == 0;
    const uint32_t mi = is_coder || is_idle ? 0 : wave - 1 - (wave >> 2);     // the modeler's block inside the group
    RcModeler<RC_NSLOT, CMP> M;
    M.init(models_all + mi * MW, slotmap_all[mi], (const uint16_t*)syms, small_sizes, lane, err);

    const uint64_t n_groups = (n_blocks + G - 1) / G;
    for (uint64_t bg = blockIdx.x; bg < n_groups; bg += gridDim.x) {
        // this thread's block: the wave's for a modeler, the lane's for the coder
        const uint64_t b = bg * G + (is_coder ? lane : mi);
        bool valid = (is_coder ? lane < G : !is_idle) && b < n_blocks;
        uint64_t s0 = 0, s1 = 0;
        if (valid) { s0 = blk_begin[b]; s1 = blk_begin[b + 1]; }
        if (valid && s1 - s0 >= 0xFFFFFF00ull) {                 // the models' counts are 32-bit words (upstream's are 64-bit [RECALLED]: it would go on)
            if (is_coder || lane == 0) atomicExch(err, 2);
            if (is_coder) out_size[b] = 0;
            valid = false;
        }
        const uint32_t ntiles = valid ? (uint32_t)((s1 - s0 + 63) / 64) : 0;
        if (!is_coder && !is_idle && lane == 0) ntiles_s[mi] = ntiles;
        // coder state (wave 0, lane = block)
        uint64_t low = 0, range = ~0ull;
        uint32_t nout = 0;
        uint8_t* dst = nullptr;
        uint32_t cap = 0;                                        // stores stop at the block's room; the block reports overflow at its end (the cursor only grows)
        if (is_coder && valid) {
            dst = out + out_off[b];
            const uint64_t room = out_off[b + 1] - out_off[b];
            cap = (uint32_t)(room < 0xFFFFFFFFull ? room : 0xFFFFFFFFull);
        }
        if (!is_coder && !is_idle && valid)                        // AbstractDnaCoder::startBlock
            M.start_block(s0, s1, scratch + b * (uint64_t)(RC_NNUM - RC_NSLOT_SMALL) * RC_STRIDE, lane);
        __syncthreads();
        uint32_t T = 0;
        for (uint32_t w = 0; w < G; w++) T = ntiles_s[w] > T ? ntiles_s[w] : T;

        for (uint32_t t = 0; t <= T; t++) {
            if (is_idle) {
            } else if (!is_coder) {
                if (t < ntiles) {
                    // =================== modeler: tile t -> ring[mi][t & 1] ===================
                    uint32_t lo, hi, tot;
                    M.tile(t, lane, lo, hi, tot);
                    const uint64_t inv = ~0ull / (uint64_t)tot;        // per lane, off the serial chains
                    ring_a[mi][t & 1][lane] = make_uint4(lo, hi - lo, tot, hi);
                    ring_b[mi][t & 1][lane] = make_uint2((uint32_t)inv, (uint32_t)(inv >> 32));
                    if (BIGOK) {
                        const bool big = __ballot(tot >= fast_total) != 0;   // (the chain's 32-bit fix-up needs totals below 2^30)
                        if (lane == 0) tile_big[mi][t & 1] = big ? 1u : 0u;
                    }
                } else if (t < T) {
                    // the group's longer blocks go on: records that leave a chain as it is (cumLow 0, freq = total = 1)
                    ring_a[mi][t & 1][lane] = make_uint4(0u, 1u, 1u, 1u);
                    ring_b[mi][t & 1][lane] = make_uint2(~0u, ~0u);
                    if (BIGOK && lane == 0) tile_big[mi][t & 1] = 0u;
                }
            } else if (t > 0) {
                // =================== coder: tile t-1 of every block of the group, lane = block ===================
                // (symbols past a block's end are "leave as it is" records, so the 64 steps are uniform)
                if (valid) {
                    const uint4* ra = &ring_a[lane][(t - 1) & 1][0];
                    const uint2* rb = &ring_b[lane][(t - 1) & 1][0];
                    // (a tile in which some block's total has reached fast_total takes the same steps with the exact division)
                    bool any_big = false;
                    if (BIGOK) any_big = __ballot(tile_big[lane < G ? lane : 0][(t - 1) & 1] != 0 && lane < G) != 0;
                    if (!BIGOK || __builtin_expect(!any_big, 1)) rc_coder_tile<false>(ra, rb, low, range, nout, dst, cap);
                    else rc_coder_tile<true>(ra, rb, low, range, nout, dst, cap);
                }
            }
            __syncthreads();
        }
        if (is_coder && valid) {
            for (int i = 0; i < 8; i++) {                               // RangeEncoder::flush
                if (nout < cap) dst[nout] = (uint8_t)(low >> 56);
                nout++;
                low <<= 8;
            }
            out_size[b] = nout;
            if (nout > cap) atomicExch(err, 1);
        }
        __syncthreads();
    }
}

// ---- the modelers alone: the records of every symbol, for chains that run on HOST cores -------------------------------------------
// A launch of a few hundred blocks leaves most of the chip idle behind ONE block's serial chain per CU (126 ms for 1.16 M symbols:
// ~280 cycles per symbol on a lone wave), and a host core runs such a chain ~50 times faster.  So for small launches the device
// only does what it is good at -- the adaptive models' cumulative counts for every symbol, lane = symbol -- and writes a 64-bit
// record per symbol: cumLow | freq << 22 | model << 44 (the host keeps the models' totals itself: they are the symbols counted).
// The blocks go through in CHUNKS of tiles so that a chunk's records cross PCIe and are coded while the next chunk is modelled:
// a block's model state (its LDS image) waits in global memory between two launches.
constexpr uint32_t RCR_MW = RC_SMALL_WORDS + RC_NSLOT_BIG * RC_STRIDE;
constexpr uint32_t RCR_STATE_WORDS = RCR_MW + RC_NNUM / 4 + 4;     // models, slot map, number of slots used
size_t rc_records_state_bytes(uint64_t n_blocks) { return (size_t)n_blocks * RCR_STATE_WORDS * sizeof(uint32_t); }

__global__ void __launch_bounds__(64) k_rc_records(const uint8_t* syms, const uint64_t* blk_begin, uint64_t n_blocks, uint32_t tile0, uint32_t tile1,
                                                  uint64_t* recs, const uint64_t* rec_off, uint32_t* state, uint32_t* scratch, int* err, uint32_t small_sizes) {
    __shared__ uint32_t models[RCR_MW];
    __shared__ uint32_t slotmap_w[RC_NNUM / 4];
    uint8_t* slotmap = (uint8_t*)slotmap_w;
    const uint32_t lane = threadIdx.x;
    RcModeler<RC_NSLOT_BIG, false> M;
    M.init(models, slotmap, (const uint16_t*)syms, small_sizes, lane, err);
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t s0 = blk_begin[b], s1 = blk_begin[b + 1];
        if (s1 - s0 >= (1ull << 22) - 512) { if (lane == 0) atomicExch(err, 2); continue; }     // (the host checks before it launches: 22-bit counts)
        const uint32_t ntiles = (uint32_t)((s1 - s0 + 63) / 64);
        const uint32_t ta = tile0 < ntiles ? tile0 : ntiles, tb = tile1 < ntiles ? tile1 : ntiles;
        if (ta >= tb) continue;
        uint32_t* st = state + b * (uint64_t)RCR_STATE_WORDS;
        uint32_t* gm = scratch + b * (uint64_t)(RC_NNUM - RC_NSLOT_SMALL) * RC_STRIDE;
        if (ta == 0) M.start_block(s0, s1, gm, lane);
        else {                                                   // the block goes on where the launch before left it
            for (uint32_t i = lane; i < RCR_MW; i += 64) models[i] = st[i];
            for (uint32_t i = lane; i < RC_NNUM / 4; i += 64) slotmap_w[i] = st[RCR_MW + i];
            M.s0 = s0; M.s1 = s1; M.gmodels = gm;
            M.nused = st[RCR_MW + RC_NNUM / 4];
            const uint64_t base = s0 + (uint64_t)ta * 64;
            M.raw_next = lane < (uint32_t)((s1 - base) < 64 ? (s1 - base) : 64) ? M.sym16[base + lane] : 0xFFFFu;
        }
        __syncthreads();
        uint64_t* out = recs + rec_off[b];
        for (uint32_t t = ta; t < tb; t++) {
            uint32_t lo, hi, tot;
            const uint32_t raw = M.raw_next;                     // (the tile's own symbols: tile() replaces them by the next tile's)
            M.tile(t, lane, lo, hi, tot);
            const uint64_t at = (uint64_t)(t - ta) * 64 + lane;
            if (s0 + (uint64_t)t * 64 + lane < s1) out[at] = (uint64_t)lo | ((uint64_t)(hi - lo) << 22) | ((uint64_t)(raw & 0xFFu) << 44);
        }
        __syncthreads();
        if (tb < ntiles) {                                       // to be continued
            for (uint32_t i = lane; i < RCR_MW; i += 64) st[i] = models[i];
            for (uint32_t i = lane; i < RC_NNUM / 4; i += 64) st[RCR_MW + i] = slotmap_w[i];
            if (lane == 0) st[RCR_MW + RC_NNUM / 4] = M.nused;
        }
        __syncthreads();
    }
}
// The same with FOUR waves per block (round 5).  A tile's 64-step rank loop -- nine tenths of the modeler's instructions -- depends on
// the tile's own symbols only, so wave w takes the loops of tiles w, w + 4, ... with counts that start from zero; what must go in tile
// order -- a new numeric model's slot, the counts at the tile start (added to the loop's), the record, Order0Model::update -- is a
// short serial section that the waves enter in turn (`turn` in LDS, raised behind the section's own LDS operations, which execute in
// order).  One block's pass: ~0.6 us per tile instead of a lone wave's 2.8.
__global__ void __launch_bounds__(256) k_rc_records4(const uint8_t* syms, const uint64_t* blk_begin, uint64_t n_blocks, uint32_t tile0, uint32_t tile1,
                                                    uint64_t* recs, const uint64_t* rec_off, uint32_t* state, uint32_t* scratch, int* err, uint32_t small_sizes) {
    __shared__ uint32_t models[RCR_MW];
    __shared__ uint32_t slotmap_w[RC_NNUM / 4];
    __shared__ uint32_t turn, nused_s;
    uint8_t* slotmap = (uint8_t*)slotmap_w;
    const uint16_t* sym16 = (const uint16_t*)syms;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr uint32_t NSLOT = RC_NSLOT_BIG;
    // per-lane constants of the overflow area's update (RcModeler::init)
    const bool is_lw = lane < 16;
    const uint32_t upd_lane = is_lw ? lane : (lane < 33 ? lane - 16 : 0), upd_base = is_lw ? RC_LW + lane : upd_lane, upd_blkmask = is_lw ? ~0u : 0u;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t s0 = blk_begin[b], s1 = blk_begin[b + 1];
        if (s1 - s0 >= (1ull << 22) - 512) { if (threadIdx.x == 0) atomicExch(err, 2); continue; }     // (the host checks before it launches: 22-bit counts)
        const uint32_t ntiles = (uint32_t)((s1 - s0 + 63) / 64);
        const uint32_t ta = tile0 < ntiles ? tile0 : ntiles, tb = tile1 < ntiles ? tile1 : ntiles;
        if (ta >= tb) continue;
        uint32_t* st = state + b * (uint64_t)RCR_STATE_WORDS;
        uint32_t* gm = scratch + b * (uint64_t)(RC_NNUM - RC_NSLOT_SMALL) * RC_STRIDE;
        __syncthreads();
        if (ta == 0) {                                           // AbstractDnaCoder::startBlock
            if (wv == 0) for (uint32_t m = 0; m < N_SMALL_MODELS; m++) model_init(&models[m * RC_SSTRIDE], lane, true);
            for (uint32_t i = threadIdx.x; i < RC_NNUM; i += 256) slotmap[i] = 255;
            if (threadIdx.x == 0) nused_s = 0;
        } else {                                                 // the block goes on where the launch before left it
            for (uint32_t i = threadIdx.x; i < RCR_MW; i += 256) models[i] = st[i];
            for (uint32_t i = threadIdx.x; i < RC_NNUM / 4; i += 256) slotmap_w[i] = st[RCR_MW + i];
            if (threadIdx.x == 0) nused_s = st[RCR_MW + RC_NNUM / 4];
        }
        if (threadIdx.x == 0) turn = ta;
        __syncthreads();
        uint64_t* out = recs + rec_off[b];
        auto load_raw = [&](uint32_t t) -> uint32_t {
            const uint64_t base = s0 + (uint64_t)t * 64;
            return (t < tb && lane < (uint32_t)((s1 - base) < 64 ? (s1 - base) : 64)) ? sym16[base + lane] : 0xFFFFu;
        };
        uint32_t raw_next = load_raw(ta + wv);
        for (uint32_t t = ta + wv; t < tb; t += 4) {
            const uint64_t base = s0 + (uint64_t)t * 64;
            const bool act = base + lane < s1;
            const uint32_t raw = raw_next;
            raw_next = load_raw(t + 4);                          // (a global load costs ~2000 cycles: the next tile's symbols one tile ahead)
            const uint32_t m = raw & 0xff, c = raw >> 8, key = (m << 8) | c;
            // ---- on its own: the tile's 64-step loop
            uint32_t lo = 0, hi = 0, tot = 0;
            rc_rank_loop(key, c, lo, hi, tot);
            // ---- in tile order
            while (__hip_atomic_load(&turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != t) __builtin_amdgcn_s_sleep(0);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            const bool numeric = act && m >= N_SMALL_MODELS;
            uint32_t slot = numeric ? slotmap[m - N_SMALL_MODELS] : 0;
            unsigned long long need = __ballot(numeric && slot == 255);
            if (need) {
                uint32_t nused = nused_s;
                while (need) {                                   // slots for numeric models first seen in this tile
                    const uint32_t l = (uint32_t)__builtin_ctzll(need);
                    const uint32_t mm = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)l);
                    const uint32_t ns = nused++;
                    if (lane == 0) slotmap[mm - N_SMALL_MODELS] = (uint8_t)ns;
                    if (ns < NSLOT) model_init(&models[RC_SMALL_WORDS + ns * RC_STRIDE], lane, false);
                    else { model_init(gm + (uint64_t)(ns - NSLOT) * RC_STRIDE, lane, false); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
                    if (numeric && m == mm) slot = ns;
                    need &= ~__ballot(numeric && m == mm);
                }
                if (lane == 0) nused_s = nused;
            }
            uint32_t mb = 0;                                     // word offset of this lane's model (RC_GLOBAL | offset for the overflow area)
            if (act) mb = !numeric ? m * RC_SSTRIDE : (slot < NSLOT ? RC_SMALL_WORDS + slot * RC_STRIDE : (RC_GLOBAL | ((slot - NSLOT) * RC_STRIDE)));
            __builtin_amdgcn_wave_barrier();
            uint32_t blo = 0, bhi = 1;                           // the counts at the tile start (the records carry no totals: the host counts them)
            if (act) {
                if (!(mb & RC_GLOBAL)) {
                    const uint32_t* sm = &models[mb];
                    blo = sm[c >> 4] + sm[RC_LW + c]; bhi = sm[(c + 1) >> 4] + sm[RC_LW + c + 1];
                } else {                                         // (through L2: another wave's updates)
                    const uint32_t* sg = gm + (mb & ~RC_GLOBAL);
                    auto ld = [&](uint32_t i) { return __hip_atomic_load(sg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
                    blo = ld(c >> 4) + ld(RC_LW + c); bhi = ld((c + 1) >> 4) + ld(RC_LW + c + 1);
                }
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if (act) out[(uint64_t)(t - ta) * 64 + lane] = (uint64_t)(blo + lo) | ((uint64_t)((bhi + hi) - (blo + lo)) << 22) | ((uint64_t)(raw & 0xFFu) << 44);
            {   // Order0Model::update for the whole tile (RcModeler::tile's)
                const bool in_lds = act && !(mb & RC_GLOBAL);
                uint32_t* mp = &models[in_lds ? mb : 0];
                const uint32_t h4 = (in_lds && numeric) ? c >> 4 : 64u;
                const uint32_t l4 = in_lds ? c & 15u : 64u, ymax = numeric ? 15u : small_size_of(small_sizes, m);
                uint32_t* lp = mp + RC_LW + (in_lds ? (c & ~15u) : 0u);
#pragma unroll
                for (uint32_t k = 1; k <= 16; k++)
                    if (k > h4) (void)__hip_atomic_fetch_add(&mp[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                for (uint32_t y = 1; y <= 15; y++)
                    if (y > l4 && y <= ymax) (void)__hip_atomic_fetch_add(&lp[y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                unsigned long long gl = __ballot(act && (mb & RC_GLOBAL));
                while (gl) {
                    const uint32_t i = (uint32_t)__builtin_ctzll(gl);
                    gl &= gl - 1;
                    const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)i);
                    const uint32_t mbi = (uint32_t)__builtin_amdgcn_readlane((int)mb, (int)i);
                    const uint32_t thr = is_lw ? (ci & 15u) : (ci >> 4);
                    const uint32_t idx = upd_base + ((ci & ~15u) & upd_blkmask);
                    if (upd_lane > thr) (void)__hip_atomic_fetch_add(gm + (mbi & ~RC_GLOBAL) + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __hip_atomic_store(&turn, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        if (tb < ntiles) {                                       // to be continued
            for (uint32_t i = threadIdx.x; i < RCR_MW; i += 256) st[i] = models[i];
            for (uint32_t i = threadIdx.x; i < RC_NNUM / 4; i += 256) st[RCR_MW + i] = slotmap_w[i];
            if (threadIdx.x == 0) st[RCR_MW + RC_NNUM / 4] = nused_s;
        }
    }
}
void launch_rc_records(hipStream_t s, const uint8_t* syms, const uint64_t* blk_begin, uint64_t n_blocks, uint32_t tile0, uint32_t tile1, uint64_t* recs,
                       const uint64_t* rec_off, uint32_t* state, uint32_t* model_scratch, int* err, uint32_t small_sizes) {
    if (!n_blocks || tile0 >= tile1) return;
    // (grid cap 256 * 4 blocks: tests/many_blocks.py's N_BLOCKS must stay above twice that, so that a workgroup takes a second trip)
    static const bool one_wave = [] { const char* e = getenv("LEON_RC_RECORDS_WAVES"); return e && atoi(e) == 1; }();     // (measurement: the round-4 kernel)
    if (one_wave) hipLaunchKernelGGL(k_rc_records, dim3((uint32_t)std::min<uint64_t>(n_blocks, 256 * 4)), dim3(64), 0, s, syms, blk_begin, n_blocks, tile0, tile1, recs, rec_off,
                                     state, model_scratch, err, small_sizes);
    else hipLaunchKernelGGL(k_rc_records4, dim3((uint32_t)std::min<uint64_t>(n_blocks, 256 * 4)), dim3(256), 0, s, syms, blk_begin, n_blocks, tile0, tile1, recs, rec_off,
                            state, model_scratch, err, small_sizes);
}

void launch_rc_encode(hipStream_t s, const uint8_t* syms, const uint64_t* blk_begin, uint64_t n_blocks, uint8_t* out,
                      const uint64_t* out_off, uint64_t* out_size, uint32_t* model_scratch, int* err, uint64_t max_block_syms, uint32_t small_sizes, bool counts_apart) {
    if (!n_blocks) return;
    // blocks per workgroup: as few as keeps every block resident on the 256 CUs (LDS: 8 blocks of 19.6 KB per CU)
    const uint64_t per_cu = (n_blocks + 255) / 256;
    const char* force = getenv("LEON_RC_GROUP");              // measurement / test override: blocks per workgroup
    uint32_t G = per_cu <= 1 ? 1u : per_cu <= 2 ? 2u : per_cu <= 4 ? 4u : 8u;
    if (force) { int v = atoi(force); if (v == 1 || v == 2 || v == 4 || v == 8) G = (uint32_t)v; }
    const uint64_t n_groups = (n_blocks + G - 1) / G;
    // (grid cap 256 * (8 / G) groups = 2048 blocks for every G: tests/many_blocks.py's N_BLOCKS must stay above twice that)
    const uint32_t g = (uint32_t)std::min<uint64_t>(n_groups, 256ull * (8 / G));
    // totals at which the coder switches to the exact division (test hook: a low value sends ordinary data down that path)
    uint32_t fast_total = RC_MAX_TOTAL;
    if (const char* e = getenv("LEON_RC_FAST_TOTAL_LOG2")) { const int v = atoi(e); if (v >= 4 && v <= 30) fast_total = 1u << v; }
    const bool big = max_block_syms + 512 >= fast_total;      // (a model's total is at most its block's symbol count + 256)
    // (streams of 2^22 - 1024 symbols and more come here, not to the host chains' 22-bit records; tests/rc_edges.py has a stream of 2^22 - 1025 symbols and one of
    // one more, each held to the oracle's bytes -- which coder took which is not observed there)
    // counts_apart (the read blocks' symbols, made by k_symbols: a numeric group's first model only ever sees 0..8): the byte-count models apart from
    // the 256-symbol slots (round 5); every other caller's streams -- the header stream's 14 byte models, leon_rc_encode_streams' arbitrary symbols --
    // as before.  LEON_RC_CMP=0: measurement / test, the round-4 layout for the read blocks too
    const bool cmp = counts_apart && [] { const char* e = getenv("LEON_RC_CMP"); return !e || atoi(e) != 0; }();
#define RC_LAUNCH(GG, N, B, C) hipLaunchKernelGGL((k_rc_encode<GG, N, B, C>), dim3(g), dim3(64 * rc_waves(GG)), 0, s, syms, blk_begin, n_blocks, out, out_off, out_size, model_scratch, err, small_sizes, fast_total)
#define RC_PICK(GG, N, C) do { if (big) RC_LAUNCH(GG, N, true, C); else RC_LAUNCH(GG, N, false, C); } while (0)
    if (cmp) {                                                // (slots at 8 blocks per workgroup: what 160 KB of LDS leave room for)
        if (G == 1) RC_PICK(1, RC_NSLOT_BIG, true);
        else if (G == 2) RC_PICK(2, RC_NSLOT_BIG, true);
        else if (G == 4) RC_PICK(4, RC_NSLOT_BIG, true);
        else RC_PICK(8, RC_NSLOT_SMALL, true);
    } else {
        if (G == 1) RC_PICK(1, RC_NSLOT_BIG, false);
        else if (G == 2) RC_PICK(2, RC_NSLOT_BIG, false);
        else if (G == 4) RC_PICK(4, RC_NSLOT_BIG, false);
        else RC_PICK(8, RC_NSLOT_SMALL + 1, false);
    }
#undef RC_PICK
#undef RC_LAUNCH
}

// ---- the context's calls that end in this file's kernels (ctx.h): the block-coding tail of a stream and the raw range coder ----
uint32_t usable_cpus();                                          // (host_streams.cpp)
namespace {
constexpr uint32_t kRbHostChainsErr = 500;   // slot of the pinned read-back words (h_rb, 512 of them) the host chains' first chunk brings the modelers' error flag to
// Launches of at most this many blocks have their chains coded on host cores (0 = never): LEON_RC_HOST_BLOCKS, default 400.
// With 2 000 blocks (8 per CU) the device's chains all run at once and win: 126 ms for 2.3 G symbols is 18 G symbols/s, 16 host cores at ~2.3 ns do 7.
uint64_t rc_host_blocks() {
    if (const char* e = getenv("LEON_RC_HOST_BLOCKS")) return (uint64_t)std::max<long long>(0, atoll(e));
    return 400;
}
uint32_t rc_host_threads(uint64_t n_blocks, uint32_t world) {
    // (all but one of the process's CPUs: the dictionary chain and its helpers are busy for the first part of a small file's step only --
    // configuration #2, 200 blocks: 88.9 ms with 12 threads and 4 chunks, 73.4 with 15 and 8, 63.9 with 15 and 16; profiles/r4_hostchains_sweep_config2.txt.
    // A rank of a job of `world` (leon_dna_set_shard: the GPUs of ONE node) shares the host, and its CPU quota, with the others: an equal share of
    // what rank 0's dictionary chain and its helpers leave.  Eight ranks taking 32 threads each would run the cgroup out of its quota, and the
    // throttling that follows stops the chain -- the one thing the job's step waits for -- along with everything else.)
    const uint32_t cpus = usable_cpus();
    uint32_t n_thr = world > 1 ? std::max<uint32_t>(2, (cpus > 6 ? cpus - 6 : 0) / world) : (cpus > 2 ? cpus - 1 : 2);
    n_thr = std::max<uint32_t>(2, std::min<uint32_t>(32, n_thr));
    if (const char* e = getenv("LEON_RC_HOST_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 256) n_thr = (uint32_t)v; }
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_thr, n_blocks));
}
// Who codes a launch's chains.  The device's coder waves take about as long as the LONGEST block's chain whatever the number of
// blocks (~100 ns per symbol of it, up to 8 blocks per CU); the host's way takes the slowest of three things that run side by side --
// the modelers' pass over the longest block (four waves per block since round 5), the records' 8 bytes per symbol over PCIe, the host
// threads' chains (two side by side per thread) -- a chunk behind one another.  10 M reads of 150 bp in 200 blocks: 116 against ~42 ms,
// the host (measured 134 and 45); 20 M reads of 250 bp in 400 blocks of 1.9 M symbols: 190 against ~140 (measured 174 and 142): left to the device, see below.
bool rc_on_host(uint64_t n_blocks, uint64_t n_syms, uint64_t max_block_syms, uint32_t world) {
    if (!n_blocks || n_blocks > rc_host_blocks() || max_block_syms + 1024 >= (1ull << HB_COUNT_BITS) || n_syms * 8 > (12ull << 30)) return false;
    if (getenv("LEON_RC_HOST_BLOCKS")) return true;              // (asked for by name: the tests, measurements)
    const double device_ns = 100.0 * (double)max_block_syms * (double)((n_blocks + 2047) / 2048);
    // (round 5: four modeler waves per block -- ~12 ns per symbol of the longest block --, the records' 8 bytes per symbol over PCIe at ~52 GB/s,
    // the chains two side by side per thread at ~2.6 ns per symbol; whichever is slowest, a sixteenth later for the first chunk's way in)
    const double thr = (double)rc_host_threads(n_blocks, world);
    const double host_ns = 1.0625 * std::max(12.0 * (double)max_block_syms, std::max(0.16 * (double)n_syms, 2.6 * (double)n_syms / thr));
    // (a near tie goes to the device: the host's cores have other work -- the dictionary chain, which is what a step waits for: at the k = 63 / 250 bp
    // shape, 400 blocks of 1.9 M symbols, the host's way takes 142 ms against the device's 174 and the step 554 ms against 542)
    return host_ns < 0.7 * device_ns;
}

// The range coder stage of a small launch: the device's modeler waves turn the symbols of every block into records, chunk of tiles
// by chunk; a chunk crosses PCIe while the next is modelled, and host threads -- each owning every n-th block -- code it while the
// one after that crosses.  On return c->hb.coders[b] holds block b's payload.  Bytes: exactly k_rc_encode's (the tests run both).
int rc_blocks_on_host(leon_dna_ctx* c, const uint8_t* d_syms, const uint64_t* d_blk_begin, uint64_t nbl, uint64_t n_syms, uint32_t small_sizes,
                      uint32_t n_small) {
    hipStream_t s = c->stream;
    HostChains& H = c->hb;
    if (!H.copy_stream) {
        // A stream of HIGH priority: the runtime maps streams onto a few hardware queues, and in a process that also holds a
        // communicator's streams (RCCL: every rank of an N-rank job) this one landed on the queue of `s` -- every chunk's copy then
        // waited behind all sixteen modeler launches and the chains started when the modelers had finished (a seat of 8: 110 ms for
        // the stage instead of ~75).  Streams of another priority get queues of their own.
        int lo = 0, hi = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(c, hipStreamCreateWithPriority(&H.copy_stream.s, hipStreamNonBlocking, hi));
    }
    std::vector<uint64_t> bb(nbl + 1);
    HIPCHK(c, hipMemcpyAsync(bb.data(), d_blk_begin, (nbl + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint64_t max_tiles = 0;
    for (uint64_t b = 0; b < nbl; b++) max_tiles = std::max<uint64_t>(max_tiles, (bb[b + 1] - bb[b] + 63) / 64);
    uint32_t n_chunks = 16;                                      // (a chunk = a pipeline stage: the first must be modelled and cross before a chain starts, the last is coded after everything)
    if (const char* e = getenv("LEON_RC_HOST_CHUNKS")) { const int v = atoi(e); if (v >= 1 && v <= 64) n_chunks = (uint32_t)v; }
    n_chunks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, max_tiles));
    const uint64_t Tc = (max_tiles + n_chunks - 1) / std::max<uint32_t>(n_chunks, 1);
    // where block b's records of chunk ch lie inside the chunk, and the chunks inside the pinned buffer
    std::vector<uint64_t> rec_off((size_t)n_chunks * nbl), rec_cnt((size_t)n_chunks * nbl), chunk_base(n_chunks + 1, 0);
    uint64_t chunk_max = 0;
    for (uint32_t ch = 0; ch < n_chunks; ch++) {
        uint64_t at = 0;
        for (uint64_t b = 0; b < nbl; b++) {
            const uint64_t len = bb[b + 1] - bb[b], a0 = std::min<uint64_t>(len, ch * Tc * 64), a1 = std::min<uint64_t>(len, (ch + 1) * Tc * 64);
            rec_off[(size_t)ch * nbl + b] = at; rec_cnt[(size_t)ch * nbl + b] = a1 - a0;
            at += a1 - a0;
        }
        chunk_base[ch + 1] = chunk_base[ch] + at;
        chunk_max = std::max(chunk_max, at);
    }
    if (chunk_base[n_chunks] != n_syms) return fail(c, LEON_E_STATE, "block symbol ranges do not add up (internal error)");
    // (memory this way needs and the device's coder does not: when it is not to be had, the caller takes the device's coder -- return 1)
    auto no_room = [&](hipError_t e) { if (e == hipSuccess) return false; (void)hipGetLastError(); return true; };
    for (auto& b : H.recs) if (no_room(b.ensure(chunk_max * 8 + 64))) return 1;
    if (no_room(H.recoff.ensure((size_t)n_chunks * nbl * 8)) || no_room(H.state.ensure(rc_records_state_bytes(nbl)))) return 1;
    HIPCHK(c, c->rc_scratch.ensure(rc_model_scratch_bytes(nbl)));
    if (n_syms * 8 + 64 > H.h_recs.cap) HIPCHK(c, H.h_recs.release());       // (only the allocation may send the launch to the device's coder)
    if (no_room(H.h_recs.ensure(n_syms * 8 + 64, n_syms * 8 + n_syms + 4096))) return 1;
    HIPCHK(c, H.ev.ensure(2 * (size_t)n_chunks));
    HIPCHK(c, hipMemcpyAsync(H.recoff.p, rec_off.data(), rec_off.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->errflag.p, 0, 4, s));
    if (H.coders.size() < nbl) H.coders.resize(nbl);
    // the host threads
    const uint32_t n_thr = rc_host_threads(nbl, c->shard_world);
    static const bool trace = getenv("LEON_TRACE_RC_HOST") != nullptr;     // measurement aid: when each chunk was modelled / had crossed / was coded, on stderr
    const auto t_begin = std::chrono::steady_clock::now();
    auto ms_now = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    std::vector<double> t_coded(n_chunks, 0.0), t_copied(n_chunks, 0.0);
    std::mutex trace_mu;
    (void)hb_recip_table();                                      // (built before the threads ask for it)
    std::atomic<uint32_t> chunks_ready{0};
    std::atomic<int> abort_flag{0};
    std::vector<std::thread> workers;
    uint64_t* const h_recs = H.h_recs.as<uint64_t>();
    HostBlockCoder* const coders = H.coders.data();
    for (uint32_t w = 0; w < n_thr; w++)
        workers.emplace_back([&, w] {
            try {
            for (uint64_t b = w; b < nbl; b += n_thr) coders[b].start(small_sizes, n_small);
            for (uint32_t ch = 0; ch < n_chunks; ch++) {
                for (uint32_t spin = 0; chunks_ready.load(std::memory_order_acquire) <= ch; spin++) {
                    if (abort_flag.load()) return;
                    if (spin < 2000) __builtin_ia32_pause(); else std::this_thread::yield();
                }
                // two of the thread's blocks side by side (HostBlockCoder::code2: two dependent chains fill the core one leaves half idle)
                static const bool pairs = [] { const char* e = getenv("LEON_RC_HOST_PAIRS"); return !(e && e[0] == '0'); }();
                for (uint64_t b = w; b < nbl; b += 2 * (uint64_t)n_thr) {
                    const uint64_t b2 = b + n_thr;
                    const uint64_t* ra = h_recs + chunk_base[ch] + rec_off[(size_t)ch * nbl + b];
                    if (b2 < nbl && pairs) HostBlockCoder::code2(coders[b], ra, rec_cnt[(size_t)ch * nbl + b], coders[b2], h_recs + chunk_base[ch] + rec_off[(size_t)ch * nbl + b2], rec_cnt[(size_t)ch * nbl + b2]);
                    else {
                        coders[b].code(ra, rec_cnt[(size_t)ch * nbl + b]);
                        if (b2 < nbl) coders[b2].code(h_recs + chunk_base[ch] + rec_off[(size_t)ch * nbl + b2], rec_cnt[(size_t)ch * nbl + b2]);
                    }
                }
                if (trace) { const double t = ms_now(); std::lock_guard<std::mutex> g(trace_mu); t_coded[ch] = std::max(t_coded[ch], t); }
            }
            for (uint64_t b = w; b < nbl; b += n_thr) coders[b].flush();
            } catch (...) { abort_flag.store(2); }               // (an output buffer that could not grow: the call fails, nothing is thrown across threads)
        });
    struct Join { std::vector<std::thread>& t; std::atomic<int>& a; bool ok = false; ~Join() { if (!ok) a.store(1); for (auto& x : t) if (x.joinable()) x.join(); } } join{workers, abort_flag};
    for (uint32_t ch = 0; ch < n_chunks; ch++) {
        if (ch >= 2) HIPCHK(c, hipStreamWaitEvent(s, H.ev[2 * (ch - 2) + 1], 0));            // the buffer's previous chunk has left it
        launch_rc_records(s, d_syms, d_blk_begin, nbl, (uint32_t)(ch * Tc), (uint32_t)((ch + 1) * Tc), H.recs[ch & 1].as<uint64_t>(),
                          H.recoff.as<uint64_t>() + (size_t)ch * nbl, H.state.as<uint32_t>(), c->rc_scratch.as<uint32_t>(), c->errflag.as<int>(), small_sizes);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(H.ev[2 * ch], s));
        HIPCHK(c, hipStreamWaitEvent(H.copy_stream, H.ev[2 * ch], 0));
        const uint64_t bytes = (chunk_base[ch + 1] - chunk_base[ch]) * 8;
        if (bytes) HIPCHK(c, hipMemcpyAsync(h_recs + chunk_base[ch], H.recs[ch & 1].p, bytes, hipMemcpyDeviceToHost, H.copy_stream));
        // (the modelers' one refusal travels with the first chunk, on this stream: a blocking hipMemcpy of the flag waited for EVERY launch
        // queued on `s` in a process that holds a communicator -- each rank of an N-rank job --, and the chains began when the modelers had finished)
        if (ch == 0) HIPCHK(c, hipMemcpyAsync(c->rb() + kRbHostChainsErr, c->errflag.p, 4, hipMemcpyDeviceToHost, H.copy_stream));
        HIPCHK(c, hipEventRecord(H.ev[2 * ch + 1], H.copy_stream));
    }
    const double t_enqueued = ms_now();
    for (uint32_t ch = 0; ch < n_chunks; ch++) {
        HIPCHK(c, hipEventSynchronize(H.ev[2 * ch + 1]));
        if (ch == 0 && (int)(uint32_t)c->rb()[kRbHostChainsErr]) return fail(c, LEON_E_OVERFLOW, "a block has more symbols than the host chains' records can count");
        chunks_ready.store(ch + 1, std::memory_order_release);
        t_copied[ch] = ms_now();
    }
    for (auto& t : workers) t.join();
    join.ok = true;
    if (abort_flag.load() == 2) return fail(c, LEON_E_OVERFLOW, "a host chain ran out of memory for its output");
    if (trace) {
        fprintf(stderr, "[leon rc host] %llu blocks, %llu symbols, %u chunks, %u threads, launches enqueued at %.1f ms:", (unsigned long long)nbl, (unsigned long long)n_syms, n_chunks, n_thr, t_enqueued);
        for (uint32_t ch = 0; ch < n_chunks; ch++) fprintf(stderr, " chunk %u in host memory at %.1f ms, coded at %.1f;", ch, t_copied[ch], t_coded[ch]);
        fprintf(stderr, " done at %.1f ms\n", ms_now());
    }
    return LEON_OK;
}

}  // namespace
int ensure_block_bufs(leon_dna_ctx* c, uint64_t nbl) {                  // the blocks' symbol ranges and payload offsets
    HIPCHK(c, c->blk_begin.ensure((nbl + 1) * 8)); HIPCHK(c, c->out_off.ensure((nbl + 1) * 8));
    HIPCHK(c, c->out_size.ensure(nbl * 8)); HIPCHK(c, c->dst_off.ensure((nbl + 1) * 8));
    return LEON_OK;
}
int ensure_rc_bufs(leon_dna_ctx* c, uint64_t nbl, uint64_t n_syms) {     // k_rc_encode's output and models
    HIPCHK(c, c->rc_out.ensure(3 * n_syms + 72 * (nbl + 1)));
    HIPCHK(c, c->rc_scratch.ensure(rc_model_scratch_bytes(nbl)));
    return LEON_OK;
}

// The block-coding tail of a stream, the DNA stream's and the header stream's: the share's symbols, counted then emitted by `symbols`
// (nullptr: the count pass; the counts, then the offsets, in c->sym_off indexed from the share's first read), cut into blocks, the blocks'
// chains coded on host cores or by k_rc_encode, the payloads brought to host memory.  ev[6] / [7] / [8]: symbols / range coder / D2H done.
int code_blocks(leon_dna_ctx* c, const Share& sh, const std::function<void(uint8_t* syms)>& symbols, uint32_t small_sizes, bool counts_apart,
                const char* unit, CodedBlocks& out) {
    hipStream_t s = c->stream;
    const uint64_t rpb = c->cfg.reads_per_block, nl = sh.nl, nbl = sh.nbl;
    HIPCHK(c, c->sym_off.ensure((nl + 1) * 8));
    uint64_t* const sym_off = c->sym_off.as<uint64_t>();
    HIPCHK(c, hipMemsetAsync(sym_off + nl, 0, 8, s));
    symbols(nullptr);
    if (int rc = run_prim(c, [&](void* t, size_t& b) { return prim::ExclusiveSum(t, b, sym_off, sym_off, nl + 1, s); })) return rc;
    uint64_t max_block_syms = 0; unsigned long long* d_max = reinterpret_cast<unsigned long long*>(c->counters.as<uint32_t>() + 8);
    HIPCHK(c, hipMemsetAsync(d_max, 0, 8, s));
    launch_max_block_syms(s, sym_off, nl, rpb, nbl, d_max);
    HIPCHK(c, hipMemcpyAsync(&out.n_syms, sym_off + nl, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&max_block_syms, d_max, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint64_t n_syms = out.n_syms;
    HIPCHK(c, c->syms.ensure(n_syms * 2 + 256));
    symbols(c->syms.as<uint8_t>());
    if (int rc = ensure_block_bufs(c, nbl)) return rc;
    launch_block_ranges(s, sym_off, nl, rpb, nbl, c->blk_begin.as<uint64_t>(), c->out_off.as<uint64_t>());
    HIPCHK(c, hipEventRecord(c->ev[6], s));

    // ---- range coder ----
    out.sizes.assign(nbl, 0); out.dst.assign(nbl + 1, 0);
    out.host_chains = rc_on_host(nbl, n_syms, max_block_syms, c->shard_world);
    if (out.host_chains) {
        // a small launch: the chains run on host cores, from the modelers' records (host_blocks.h)
        const int rc = rc_blocks_on_host(c, c->syms.as<uint8_t>(), c->blk_begin.as<uint64_t>(), nbl, n_syms, small_sizes, N_SMALL_MODELS);
        if (rc == 1) out.host_chains = false;                    // (no room for the records: the device's coder)
        else if (rc) return rc;
    }
    if (out.host_chains) {
        HIPCHK(c, hipEventRecord(c->ev[7], s));
        for (uint64_t b = 0; b < nbl; b++) out.sizes[b] = c->hb.coders[b].size();
    } else {
        if (int rc = ensure_rc_bufs(c, nbl, n_syms)) return rc;
        HIPCHK(c, hipMemsetAsync(c->errflag.p, 0, 4, s));
        launch_rc_encode(s, c->syms.as<uint8_t>(), c->blk_begin.as<uint64_t>(), nbl, c->rc_out.as<uint8_t>(), c->out_off.as<uint64_t>(),
                         c->out_size.as<uint64_t>(), c->rc_scratch.as<uint32_t>(), c->errflag.as<int>(), max_block_syms, small_sizes, counts_apart);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev[7], s));
        int errflag = 0;
        HIPCHK(c, hipMemcpyAsync(out.sizes.data(), c->out_size.p, nbl * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&errflag, c->errflag.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (errflag == 3) return fail(c, LEON_E_STATE, "a numeric value's byte count above 8 in the symbol stream (internal error)");   // (counts_apart only)
        if (errflag) return fail(c, LEON_E_OVERFLOW, errflag == 2 ? std::string("a ") + unit + " block has 2^32 symbols or more"
                                                                  : std::string("range coder output exceeded its 3 bytes/symbol bound"));
    }
    for (uint64_t b = 0; b < nbl; b++) out.dst[b + 1] = out.dst[b] + out.sizes[b];
    const uint64_t payload_bytes = out.payload_bytes = out.dst[nbl];
    if (!out.host_chains) {
        // ---- gather + D2H ----
        HIPCHK(c, c->payload.ensure(payload_bytes + 16));
        HIPCHK(c, hipMemcpyAsync(c->dst_off.p, out.dst.data(), (nbl + 1) * 8, hipMemcpyHostToDevice, s));
        launch_gather_payload(s, c->rc_out.as<uint8_t>(), c->out_off.as<uint64_t>(), c->dst_off.as<uint64_t>(), c->out_size.as<uint64_t>(),
                              nbl, c->payload.as<uint8_t>());
        HIPCHK(c, c->h_payload.ensure(payload_bytes + 16, payload_bytes + payload_bytes / 4 + 4096));
        HIPCHK(c, hipMemcpyAsync(c->h_payload.p, c->payload.p, payload_bytes, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipEventRecord(c->ev[8], s));
    HIPCHK(c, hipStreamSynchronize(s));
    return LEON_OK;
}

// Leon::writeBlock, in block order, the batch's first block numbered first_block; a sink that refuses one poisons the stream
int deliver_blocks(leon_dna_ctx* c, const CodedBlocks& out, const Share& sh, uint64_t n, uint64_t first_block, leon_block_sink sink, void* user) {
    const uint64_t rpb = c->cfg.reads_per_block;
    for (uint64_t b = 0; b < sh.nbl; b++) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(rpb, n - (sh.lb0 + b) * rpb);
        const uint8_t* pay = out.host_chains ? c->hb.coders[b].data() : c->h_payload.as<uint8_t>() + out.dst[b];
        if (sink(user, first_block + sh.lb0 + b, pay, out.sizes[b], nr)) {
            c->poisoned = true;                                  // the caller holds part of the batch's blocks
            return fail(c, LEON_E_SINK, "block sink returned non-zero");
        }
    }
    return LEON_OK;
}

int RcStreamsDev::code(leon_dna_ctx* c, const uint8_t* d_syms, const uint64_t* begin_host, uint64_t n_streams, uint64_t longest, const char* overflow,
                       uint64_t* sizes) {
    hipStream_t s = c->stream;
    HIPCHK(c, begin.ensure((n_streams + 1) * 8)); HIPCHK(c, d_off.ensure((n_streams + 1) * 8));
    HIPCHK(c, size.ensure(n_streams * 8)); HIPCHK(c, scr.ensure(rc_model_scratch_bytes(n_streams)));
    off.resize(n_streams + 1);
    for (uint64_t b = 0; b <= n_streams; b++) off[b] = ((3 * begin_host[b] + 7) & ~7ull) + 64 * b;
    HIPCHK(c, out.ensure(off[n_streams] + 64));
    HIPCHK(c, hipMemcpy(begin.p, begin_host, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_off.p, off.data(), (n_streams + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->errflag.p, 0, 4, s));
    launch_rc_encode(s, d_syms, begin.as<uint64_t>(), n_streams, out.as<uint8_t>(), d_off.as<uint64_t>(), size.as<uint64_t>(), scr.as<uint32_t>(),
                     c->errflag.as<int>(), longest);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    int errflag = 0;
    HIPCHK(c, hipMemcpy(&errflag, c->errflag.p, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(sizes, size.p, n_streams * 8, hipMemcpyDeviceToHost));
    return errflag ? fail(c, LEON_E_OVERFLOW, overflow) : LEON_OK;
}
}  // namespace leon

using namespace leon;
extern "C" {
// ------------------------------------------------------------------------------------------------ raw range coder
int leon_rc_encode_streams(leon_dna_ctx* c, const uint8_t* syms, const uint64_t* begin, uint64_t n_streams,
                           uint8_t* out, uint64_t out_cap, uint64_t* sizes) {
    if (!c || !begin || !sizes || (!out && out_cap)) return LEON_E_INVALID;
    if (!n_streams) return LEON_OK;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t n_syms = begin[n_streams] - begin[0];
    if (begin[0] != 0) return fail(c, LEON_E_INVALID, "begin[0] must be 0");
    for (uint64_t i = 0; i < n_syms; i++) {
        uint32_t m = syms[2 * i], v = syms[2 * i + 1];
        if (m >= N_MODELS || (m < N_SMALL_MODELS && v >= small_model_size(m))) return fail(c, LEON_E_INVALID, "bad symbol");
    }
    OwnBuf dsyms, dbegin; RcStreamsDev D;
    HIPCHK(c, dsyms.ensure(n_syms * 2 + 256));
    if (n_syms) HIPCHK(c, hipMemcpy(dsyms.p, syms, n_syms * 2, hipMemcpyHostToDevice));
    uint64_t longest = 0;
    for (uint64_t b = 0; b < n_streams; b++) longest = std::max(longest, begin[b + 1] - begin[b]);
    // (test hook, LEON_RC_STREAMS_ON_HOST=1: the same streams through the host chains fed by the device's modelers -- host_blocks.h --
    // so that the tests hold the two coders against each other and against the oracle on the same symbols)
    // (the hand-over is rc_on_host's: a longest stream of 2^22 - 1025 symbols still goes to the host chains, one more to the device; tests/rc_edges.py's pack22_host /
    // pack22_device are of these two lengths and are held to the oracle's bytes, whichever coder takes them)
    if (const char* e = getenv("LEON_RC_STREAMS_ON_HOST")) if (e[0] == '1' && longest + 1024 < (1ull << HB_COUNT_BITS)) {
        HIPCHK(c, dbegin.ensure((n_streams + 1) * 8));
        HIPCHK(c, hipMemcpy(dbegin.p, begin, (n_streams + 1) * 8, hipMemcpyHostToDevice));
        if (int rc = rc_blocks_on_host(c, dsyms.as<uint8_t>(), dbegin.as<uint64_t>(), n_streams, n_syms, SMALL_SIZES_DNA, N_SMALL_MODELS))
            return rc == 1 ? fail(c, LEON_E_HIP, "no memory for the host chains' records") : rc;
        uint64_t w = 0;
        for (uint64_t b = 0; b < n_streams; b++) {
            sizes[b] = c->hb.coders[b].size();
            if (w + sizes[b] > out_cap) return fail(c, LEON_E_OVERFLOW, "out_cap too small");
            memcpy(out + w, c->hb.coders[b].data(), sizes[b]);
            w += sizes[b];
        }
        return LEON_OK;
    }
    if (int rc = D.code(c, dsyms.as<uint8_t>(), begin, n_streams, longest, "range coder output exceeded its bound", sizes)) return rc;
    uint64_t w = 0;
    for (uint64_t b = 0; b < n_streams; b++) {
        if (w + sizes[b] > out_cap) return fail(c, LEON_E_OVERFLOW, "out_cap too small");
        hipError_t e = hipMemcpy(out + w, D.out.as<uint8_t>() + D.off[b], sizes[b], hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(c, LEON_E_HIP, hipGetErrorString(e));
        w += sizes[b];
    }
    return LEON_OK;
}
}  // extern "C"
