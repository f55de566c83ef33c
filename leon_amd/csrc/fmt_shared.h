// fmt_shared.h -- what the two output-driven record formatters share (fmt_kernels.hip: FASTA / FASTQ text, DESIGN.md 4.9;
// bam_kernels.hip: unaligned BAM records): the pair the scan carries, the tile geometry, the look-up of the record a
// byte lies in and the staging of a tile's record offsets in LDS.
#pragma once
#include "kernels.h"

namespace leon {

struct FmtPair {                                               // what the scan carries: a record's output offset and its first base
    uint64_t rec, base;
    FmtPair() = default;
    __host__ __device__ FmtPair(int v) : rec((uint64_t)v), base((uint64_t)v) {}
    __host__ __device__ FmtPair(uint64_t r, uint64_t b) : rec(r), base(b) {}
    __host__ __device__ FmtPair operator+(const FmtPair& o) const { return FmtPair(rec + o.rec, base + o.base); }
};

constexpr uint32_t FMT_THREADS = 256;
constexpr uint32_t FMT_TILE = FMT_THREADS * 16;                 // output bytes a workgroup owns
constexpr uint32_t FMT_STAGE = 256;                             // records whose offsets one pass holds in LDS

// fmt_kernels.hip: exclusive, n_reads + 1 entries, out[n_reads] = the totals; and rec_off[0 .. n_reads] = off[].rec
hipError_t fmt_scan(void* tmp, size_t& bytes, const FmtPair* in, FmtPair* out, uint64_t n_reads, hipStream_t s);
void launch_fmt_rec_off(hipStream_t s, const FmtPair* off, uint64_t n_reads, uint64_t* rec_off);

namespace {

__constant__ uint64_t kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                    10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
                                    1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull,
                                    10000000000000000000ull};

__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
    uint32_t n = 1;
#pragma unroll
    for (uint32_t k = 1; k < 20; k++) n += v >= kPow10[k];
    return n;
}

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// The record output byte t lies in: the r with off[r].rec <= t < off[r + 1].rec (off[0].rec == 0, off[n_reads].rec == the size > t).
// The search starts from a guess g < n_reads, brackets the answer by doubling steps away from it and bisects inside the bracket: a
// handful of dependent loads for a good guess where a bisection of all of off[] takes log2(n_reads) of them.
__device__ __forceinline__ uint64_t fmt_record_of(const FmtPair* __restrict__ off, uint64_t n_reads, uint64_t t, uint64_t g) {
    uint64_t lo, hi;
    if (off[g].rec <= t) {
        lo = g; hi = n_reads;
        for (uint64_t step = 1; lo + step < n_reads; step <<= 1) {
            if (off[lo + step].rec <= t) lo += step; else { hi = lo + step; break; }
        }
    } else {
        lo = 0; hi = g;
        for (uint64_t step = 1; hi > step; step <<= 1) {
            if (off[hi - step].rec <= t) { lo = hi - step; break; }
            hi -= step;
        }
    }
    while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (off[mid].rec <= t) lo = mid; else hi = mid; }
    return lo;
}

// one pass's staging: the offsets of records first .. first + cnt (cnt <= FMT_STAGE, first + cnt <= n_reads) into the workgroup's three
// tables of FMT_STAGE + 1 entries; the caller puts a barrier behind it
__device__ __forceinline__ void fmt_stage(const FmtPair* __restrict__ off, const uint64_t* __restrict__ hdr_off, uint64_t hdr0, uint64_t first, uint32_t cnt,
                                          uint64_t* s_rec, uint64_t* s_base, uint64_t* s_hdr) {
    for (uint32_t i = threadIdx.x; i <= cnt; i += FMT_THREADS) {
        const FmtPair p = off[first + i];
        s_rec[i] = p.rec; s_base[i] = p.base;
        s_hdr[i] = hdr_off ? hdr_off[first + i] - hdr0 : 0;
    }
}

}  // namespace
}  // namespace leon
