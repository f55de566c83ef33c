// bam_kernels.hip -- the restored reads as unaligned BAM records, formatted on the device (leon_records_bam_device).
//
// The record's shape is host_bam.h's.  Like the text of fmt_kernels.hip it is a gather: k_bam_sizes finds every name's end, checks the
// header offset table and the names' lengths and gives every record's size, the device-wide exclusive scan of fmt_kernels.hip turns the
// sizes into rec_off[] and the lengths into base offsets, and k_bam_records writes the records OUTPUT-driven: a lane per 16 aligned
// output bytes, every byte a function of (record, offset in the record).
#include "kernels.h"
#include "fmt_shared.h"
#include "host_bam.h"
#include "device_call.h"

#include <algorithm>

namespace leon {
namespace {

struct BamLayout { uint64_t first_read_index, hdr_bytes; uint32_t with_quals; };

// flag words of a call (64 bytes, the first 16 zeroed, the two minima set to all ones by the caller)
enum { BAM_F_BACKWARDS = 0, BAM_F_END = 1, BAM_F_NAME = 2, BAM_F_QUAL = 3 };
struct BamFlags { uint32_t f[4]; unsigned long long min_name, min_qual; };

constexpr uint32_t BAM_MAX_PASSES = FMT_TILE / BAM_MIN_RECORD / FMT_STAGE + 2;

// a lane per read: in[r] = (the record's bytes, the read's bases), in[n] = (0, 0); name_len[r] = the bytes before the header's first
// space or tab (the index's digits without a header stream).  A lane reads its header only where its two offsets lie inside the
// hdr_bytes the call was given and in order: offsets that do not are reported by flags f[BAM_F_BACKWARDS] / f[BAM_F_END] (as
// k_fmt_sizes reports them) and the call ends before anything else is indexed with them.
__global__ __launch_bounds__(256) void k_bam_sizes(BamLayout L, const uint32_t* __restrict__ len, const uint8_t* __restrict__ hdr,
                                                   const uint64_t* __restrict__ hdr_off, uint64_t n, FmtPair* __restrict__ in,
                                                   uint32_t* __restrict__ name_len, BamFlags* __restrict__ flags) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        in[n].rec = 0; in[n].base = 0;
        if (hdr_off && hdr_off[n] - hdr_off[0] != L.hdr_bytes) flags->f[BAM_F_END] = 1;
        return;
    }
    const uint64_t l = len[r];
    uint64_t hl, nl;
    if (hdr_off) {
        const uint64_t h0 = hdr_off[0], a = hdr_off[r], b = hdr_off[r + 1];
        hl = b >= a ? b - a : 0;
        if (b < a) flags->f[BAM_F_BACKWARDS] = 1;
        nl = hl;
        if (a >= h0 && b >= a && b - h0 <= L.hdr_bytes) {
            const uint8_t* h = hdr + (a - h0);
            for (uint64_t i = 0; i < hl; i++) { const uint8_t c = h[i]; if (c == ' ' || c == '\t') { nl = i; break; } }
        }
    } else hl = nl = dec_digits(L.first_read_index + r);
    if (nl > BAM_MAX_NAME) { flags->f[BAM_F_NAME] = 1; atomicMin(&flags->min_name, (unsigned long long)r); }
    name_len[r] = (uint32_t)min64(nl, 0xFFFFFFFFull);
    in[r].rec = bam_record_size(nl, hl, l);
    in[r].base = l;
}

// what a lane keeps of the record it is in: its bytes [rec0, rec1), and where its parts begin as offsets in the record
struct BamRec {
    uint64_t rec0, rec1;
    uint64_t len, bbase, hbase;     // bases; first base (and quality); first header byte
    uint64_t index;                 // its read index
    uint32_t nl, l_name;            // the name as the header gives it; as written, with its NUL
    uint64_t o_seq, o_qual, o_aux;  // the first byte of the base codes, of the qualities, of the aux field (== the size: none)
};

// Output-driven, the geometry of k_fmt_records: workgroup b owns the 16-byte-aligned tile [b * FMT_TILE, (b + 1) * FMT_TILE) of
// "virtual" positions, position v being output byte v - mis (mis = out & 15), lane t its bytes [16 t, 16 t + 16).  The tile's first and
// last record come from fmt_record_of; the offsets of the records between them are staged in LDS (fmt_stage), with the names'
// lengths beside them; a record has at least BAM_MIN_RECORD bytes, so a tile touches at most 109 records and one pass holds them (the
// pass loop is kept for the bound's sake).  A lane walks its 16 bytes one by one, gathers them into two 64-bit registers and stores
// them once: one aligned 16-byte store -- a wave's 64 stores are one contiguous KiB --, or single bytes in the first and last partial
// chunk.  Its loads are byte gathers: neighbouring lanes read neighbouring bytes of the header, the qualities and (every second byte)
// the bases.  The base codes come from a 256-byte table in LDS.
// Bounds: off[] and hdr_off[] are indexed up to n_reads, name_len[] below it; bases / quals below off[n].base == n_bases and hdr below
// hdr_off[n] - hdr_off[0] == hdr_bytes, both verified by the caller before this launch; out below out_size == off[n].rec.
// A quality byte below 33 sets f[BAM_F_QUAL] and lowers min_qual to its read: the caller fails the call.
__global__ __launch_bounds__(256) void k_bam_records(BamLayout L, const FmtPair* __restrict__ off, const uint64_t* __restrict__ hdr_off,
                                                     const uint32_t* __restrict__ name_len, uint64_t n_reads, const uint8_t* __restrict__ bases,
                                                     const uint8_t* __restrict__ hdr, const uint8_t* __restrict__ quals, uint8_t* __restrict__ out,
                                                     uint64_t out_size, BamFlags* __restrict__ flags) {
    __shared__ uint64_t s_rec[FMT_STAGE + 1], s_base[FMT_STAGE + 1], s_hdr[FMT_STAGE + 1];
    __shared__ uint32_t s_nl[FMT_STAGE];
    __shared__ uint8_t s_code[256];
    s_code[threadIdx.x] = (uint8_t)bam_base_code(threadIdx.x);
    const uint32_t mis = (uint32_t)((uintptr_t)out & 15);
    const uint64_t v0 = blockIdx.x * (uint64_t)FMT_TILE;
    const uint64_t tile_lo = v0 > mis ? v0 - mis : 0, tile_hi = min64(v0 + FMT_TILE - mis, out_size);
    if (tile_lo >= tile_hi) return;                              // (the grid is sized by the output: not taken)
    const uint64_t cv = v0 + threadIdx.x * 16u;
    uint64_t c_lo = cv > mis ? cv - mis : 0, c_hi = min64(cv + 16 - mis, out_size);
    if (c_lo > c_hi) c_lo = c_hi;
    uint64_t first = fmt_record_of(off, n_reads, tile_lo, min64((uint64_t)((double)tile_lo / (double)out_size * (double)n_reads), n_reads - 1));
    const uint64_t last = fmt_record_of(off, n_reads, tile_hi - 1, first);
    const uint64_t hdr0 = hdr_off ? hdr_off[0] : 0;
    uint64_t acc0 = 0, acc1 = 0;
    for (uint32_t pass = 0; pass < BAM_MAX_PASSES; pass++) {
        if (first > last) break;
        const uint32_t cnt = (uint32_t)min64(FMT_STAGE, last + 1 - first);
        fmt_stage(off, hdr_off, hdr0, first, cnt, s_rec, s_base, s_hdr);
        for (uint32_t i = threadIdx.x; i < cnt; i += FMT_THREADS) s_nl[i] = name_len[first + i];
        __syncthreads();
        const uint64_t p_end = s_rec[cnt];
        const uint64_t t = max64(c_lo, s_rec[0]);
        const uint64_t t_end = min64(c_hi, p_end);
        if (t < t_end) {
            uint32_t a = 0, b = cnt;                             // s_rec[a] <= t < s_rec[b]
            while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (s_rec[m] <= t) a = m; else b = m; }
            BamRec R;
            auto enter = [&](uint32_t r) {
                R.rec0 = s_rec[r]; R.rec1 = s_rec[r + 1];
                R.bbase = s_base[r]; R.len = s_base[r + 1] - R.bbase;
                R.hbase = s_hdr[r];
                R.index = L.first_read_index + first + r;
                R.nl = s_nl[r];
                R.l_name = (R.nl ? R.nl : 1) + 1;
                R.o_seq = BAM_FIXED + R.l_name;
                R.o_qual = R.o_seq + (R.len + 1) / 2;
                R.o_aux = R.o_qual + R.len;
            };
            enter(a);
            uint32_t j = (uint32_t)(t + mis - cv);               // 0..15: the byte's place in the lane's 16
            const uint32_t j_end = (uint32_t)(t_end + mis - cv);
            uint64_t o = t - R.rec0;
            bool low = false;
            for (; j < j_end; j++, o++) {
                if (o >= R.rec1 - R.rec0) {
                    if (low) { flags->f[BAM_F_QUAL] = 1; atomicMin(&flags->min_qual, (unsigned long long)(R.index - L.first_read_index)); low = false; }
                    enter(++a); o = 0;
                }
                uint32_t byte;
                if (o < BAM_FIXED)
                    byte = bam_fixed_word((uint32_t)o >> 2, (uint32_t)(R.rec1 - R.rec0 - 4), R.l_name, (uint32_t)R.len) >> (8 * ((uint32_t)o & 3));
                else if (o < R.o_seq) {
                    const uint32_t i = (uint32_t)o - BAM_FIXED;
                    if (i + 1 == R.l_name) byte = 0;
                    else if (!R.nl) byte = '*';
                    else if (hdr) byte = hdr[R.hbase + i];
                    else byte = (uint32_t)('0' + (R.index / kPow10[R.nl - 1 - i]) % 10);
                } else if (o < R.o_qual) {
                    const uint64_t i = 2 * (o - R.o_seq);
                    byte = (uint32_t)s_code[bases[R.bbase + i]] << 4;
                    if (i + 1 < R.len) byte |= s_code[bases[R.bbase + i + 1]];
                } else if (o < R.o_aux) {
                    if (L.with_quals) { const uint32_t q = quals[R.bbase + (o - R.o_qual)]; low |= q < 33; byte = q - 33; }
                    else byte = 0xFF;
                } else {
                    const uint64_t i = o - R.o_aux;                // 'C' 'O' 'Z', the comment behind the separator, NUL
                    if (i < 3) byte = i == 0 ? 'C' : i == 1 ? 'O' : 'Z';
                    else if (o + 1 == R.rec1 - R.rec0) byte = 0;
                    else byte = hdr[R.hbase + R.nl + 1 + (i - 3)];
                }
                const uint64_t v = byte & 0xFF;
                if (j < 8) acc0 |= v << (8 * j); else acc1 |= v << (8 * (j - 8));
            }
            if (low) { flags->f[BAM_F_QUAL] = 1; atomicMin(&flags->min_qual, (unsigned long long)(R.index - L.first_read_index)); }
        }
        __syncthreads();
        if (p_end >= tile_hi) break;
        first += cnt;
    }
    if (c_hi - c_lo == 16) {
        *reinterpret_cast<uint4*>(out + c_lo) = make_uint4((uint32_t)acc0, (uint32_t)(acc0 >> 32), (uint32_t)acc1, (uint32_t)(acc1 >> 32));
    } else {
        for (uint64_t t = c_lo; t < c_hi; t++) {
            const uint32_t j = (uint32_t)(t + mis - cv);
            out[t] = (uint8_t)((j < 8 ? acc0 >> (8 * j) : acc1 >> (8 * (j - 8))));
        }
    }
}

}  // namespace
}  // namespace leon

using namespace leon;

extern "C" int leon_records_bam_device(int device_id, const leon_record_layout* lay, const uint8_t* d_bases, const uint32_t* d_len, uint64_t n_reads,
                                       uint64_t n_bases, const uint8_t* d_hdr_text, const uint64_t* d_hdr_off, const uint8_t* d_quals, uint8_t* d_out,
                                       uint64_t out_cap, uint64_t* d_rec_off, uint64_t* out_size) {
    static const char* const who = "leon_records_bam_device";
    if (out_size) *out_size = 0;
    {
        const std::string why = bam_args_refusal(who, lay, d_bases, d_len, n_reads, n_bases, d_hdr_text, d_hdr_off, out_size);
        if (!why.empty()) return dev_fail(LEON_E_INVALID, why);
    }
    CallStream st;
    if (!n_reads) {                                              // no record: rec_off = [0]
        if (!d_rec_off) return LEON_OK;
        if (const int rc = dev_open(who, device_id, st)) return rc;
        DEVCHK(hipMemsetAsync(d_rec_off, 0, 8, st.s));
        DEVCHK(hipStreamSynchronize(st.s));
        return LEON_OK;
    }
    if (const int rc = dev_open(who, device_id, st)) return rc;
    hipStream_t s = st.s;
    const uint64_t* hdr_off = d_hdr_text ? d_hdr_off : nullptr;
    BamLayout L{};
    L.first_read_index = lay->first_read_index; L.hdr_bytes = lay->hdr_bytes; L.with_quals = lay->fastq && d_quals ? 1 : 0;
    OwnBuf d_in, d_off, d_nl, d_flags, d_tmp;
    DEVCHK(d_in.ensure((n_reads + 1) * sizeof(FmtPair))); DEVCHK(d_off.ensure((n_reads + 1) * sizeof(FmtPair)));
    DEVCHK(d_nl.ensure(n_reads * sizeof(uint32_t)));
    DEVCHK(d_flags.ensure(64));
    static_assert(sizeof(BamFlags) == 32, "the flag words and the two minima");
    DEVCHK(hipMemsetAsync(d_flags.p, 0, 16, s));
    DEVCHK(hipMemsetAsync((uint8_t*)d_flags.p + 16, 0xFF, 16, s));
    const uint32_t size_blocks = (uint32_t)((n_reads + 1 + 255) / 256);
    hipLaunchKernelGGL(k_bam_sizes, dim3(size_blocks), dim3(256), 0, s, L, d_len, d_hdr_text, hdr_off, n_reads, d_in.as<FmtPair>(), d_nl.as<uint32_t>(),
                       d_flags.as<BamFlags>());
    DEVCHK(hipGetLastError());
    size_t tmp_bytes = 0;
    DEVCHK(fmt_scan(nullptr, tmp_bytes, d_in.as<FmtPair>(), d_off.as<FmtPair>(), n_reads, s));
    DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    DEVCHK(fmt_scan(d_tmp.p, tmp_bytes, d_in.as<FmtPair>(), d_off.as<FmtPair>(), n_reads, s));
    BamFlags flags;
    uint64_t totals[2] = {0, 0};
    DEVCHK(hipMemcpyAsync(&flags, d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
    DEVCHK(hipMemcpyAsync(totals, d_off.as<FmtPair>() + n_reads, 16, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    // what the arrays say against what the call was told, before anything is indexed with it
    if (flags.f[BAM_F_BACKWARDS]) return dev_fail(LEON_E_INVALID, bam_offsets_backwards(who));
    if (flags.f[BAM_F_END]) return dev_fail(LEON_E_INVALID, bam_offsets_end(who, lay->hdr_bytes));
    if (totals[1] != n_bases) return dev_fail(LEON_E_INVALID, bam_lengths_sum(who, totals[1], n_bases));
    if (flags.f[BAM_F_NAME]) {
        if (flags.min_name >= n_reads) return dev_fail(LEON_E_STATE, std::string(who) + ": a name was refused without its read");
        uint32_t bytes = 0;
        DEVCHK(hipMemcpyAsync(&bytes, d_nl.as<uint32_t>() + flags.min_name, 4, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
        return dev_fail(LEON_E_INVALID, bam_name_refusal(who, lay->first_read_index + flags.min_name, bytes));
    }
    *out_size = totals[0];
    if (totals[0] > out_cap || !d_out) return dev_fail(LEON_E_OVERFLOW, bam_need(who, totals[0]));
    const uint64_t mis = (uintptr_t)d_out & 15;
    const uint64_t blocks = (mis + totals[0] + FMT_TILE - 1) / FMT_TILE;
    hipLaunchKernelGGL(k_bam_records, dim3((uint32_t)blocks), dim3(FMT_THREADS), 0, s, L, d_off.as<FmtPair>(), hdr_off, d_nl.as<uint32_t>(), n_reads, d_bases,
                       d_hdr_text, d_quals, d_out, totals[0], d_flags.as<BamFlags>());
    DEVCHK(hipGetLastError());
    if (d_rec_off) { launch_fmt_rec_off(s, d_off.as<FmtPair>(), n_reads, d_rec_off); DEVCHK(hipGetLastError()); }
    DEVCHK(hipMemcpyAsync(&flags, d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    if (flags.f[BAM_F_QUAL]) return dev_fail(LEON_E_INVALID, bam_qual_refusal(who, lay->first_read_index + flags.min_qual));
    return LEON_OK;
}
