// fmt_kernels.hip -- FASTA / FASTQ records formatted on the device (leon_records_format_device).
//
// A record, as the host's format_range writes it (leon_host.cpp):
//     lead  header | decimal(first_read_index + r)  '\n'
//     sequence: len bytes + '\n'  (wrap == 0 or len <= wrap), else ceil(len / wrap) lines of at most wrap bytes, each + '\n'
//     FASTQ:  '+'  [the header again]  '\n'  len quality bytes  '\n'
// Every byte's place follows from the lengths, so the text is a gather: k_fmt_sizes gives every record's size (and checks the header
// offset table), a device-wide exclusive scan turns the sizes into rec_off[] and the lengths into base offsets, and k_fmt_records
// writes the text OUTPUT-driven: a lane per 16 aligned output bytes, the way k_pack writes its slots.
#include "kernels.h"
#include "prim.h"
#include "fmt_shared.h"
#include "device_call.h"

#include <algorithm>

namespace leon {

struct FmtLayout { uint64_t first_read_index, hdr_bytes; uint32_t wrap; uint8_t lead, fastq, plus_kind; };
namespace {

constexpr uint32_t FMT_MIN_RECORD = 3;                          // lead, '\n', '\n': an empty header and an empty FASTA read
constexpr uint32_t FMT_MAX_PASSES = FMT_TILE / FMT_MIN_RECORD / FMT_STAGE + 2;

__device__ __forceinline__ uint64_t seq_text_len(uint64_t len, uint32_t wrap) {
    return wrap && len > wrap ? len + (len + wrap - 1) / wrap : len + 1;
}

// a lane per read: in[r] = (the record's bytes, the read's bases); in[n] = (0, 0), so that the scan's last entry is the totals.
// flags[0]: the header offsets run backwards somewhere; flags[1]: they do not end at the header bytes the call was given.
__global__ __launch_bounds__(256) void k_fmt_sizes(FmtLayout L, const uint32_t* __restrict__ len, const uint64_t* __restrict__ hdr_off, uint64_t n,
                                                   FmtPair* __restrict__ in, uint32_t* __restrict__ flags) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        in[n].rec = 0; in[n].base = 0;
        if (hdr_off && hdr_off[n] - hdr_off[0] != L.hdr_bytes) flags[1] = 1;
        return;
    }
    const uint64_t l = len[r];
    uint64_t hl;
    if (hdr_off) {
        const uint64_t a = hdr_off[r], b = hdr_off[r + 1];
        hl = b >= a ? b - a : 0;
        if (b < a) flags[0] = 1;
    } else hl = dec_digits(L.first_read_index + r);
    in[r].rec = 1 + hl + 1 + seq_text_len(l, L.wrap) + (L.fastq ? 1 + (L.plus_kind ? hl : 0) + 1 + l + 1 : 0);
    in[r].base = l;
}

// what a lane keeps of the record it is in
struct FmtRec {
    uint64_t rec0, rec1;            // the record's text [rec0, rec1)
    uint64_t hl, len, seq_text;     // header (or index digits), bases, the sequence's lines with their newlines
    uint64_t hbase, bbase;          // first header byte / first base (and quality) of the record
    uint64_t index;                 // its read index (no header stream)
};

// The run of record R that byte o begins: its bytes either lie back to back in one of the sources (the pointer to byte o's source,
// the run ending before record offset `end`) or are one byte the record's shape gives (nullptr, the byte in lit, end = o + 1)
__device__ __forceinline__ const uint8_t* fmt_run(const FmtLayout& L, const FmtRec& R, uint64_t o, const uint8_t* __restrict__ bases,
                                                  const uint8_t* __restrict__ hdr, const uint8_t* __restrict__ quals, uint64_t& end, uint32_t& lit) {
    lit = '\n'; end = o + 1;
    if (o == 0) { lit = L.lead; return nullptr; }
    if (o <= R.hl) {
        if (hdr) { end = R.hl + 1; return hdr + R.hbase + o - 1; }
        lit = (uint32_t)('0' + (R.index / kPow10[R.hl - o]) % 10);
        return nullptr;
    }
    if (o == R.hl + 1) return nullptr;
    const uint64_t s = o - (R.hl + 2);
    if (s < R.seq_text) {
        if (!(L.wrap && R.len > L.wrap)) {
            if (s >= R.len) return nullptr;
            end = o + (R.len - s);
            return bases + R.bbase + s;
        }
        const uint64_t w1 = (uint64_t)L.wrap + 1;                 // a line at a time
        uint64_t line, col;
        if (((s | w1) >> 32) == 0) { line = (uint32_t)s / (uint32_t)w1; col = (uint32_t)s - (uint32_t)line * (uint32_t)w1; }
        else { line = s / w1; col = s - line * w1; }
        const uint64_t i = line * L.wrap + col;
        if (col == L.wrap || i >= R.len) return nullptr;
        end = o + min64(L.wrap - col, R.len - i);
        return bases + R.bbase + i;
    }
    const uint64_t q = s - R.seq_text, phl = L.plus_kind ? R.hl : 0;          // (FASTQ: a FASTA record ends with its sequence)
    if (q == 0) { lit = '+'; return nullptr; }
    if (q <= phl) { end = o + (phl - (q - 1)); return hdr + R.hbase + q - 1; }
    if (q == phl + 1) return nullptr;
    const uint64_t u = q - (phl + 2);
    if (u >= R.len) return nullptr;
    end = o + (R.len - u);
    return quals + R.bbase + u;
}

// Output-driven: workgroup b owns the 16-byte-aligned tile [b * FMT_TILE, (b + 1) * FMT_TILE) of "virtual" positions, position v
// being text byte v - mis (mis = text & 15, so that v = 0 is the aligned address below the text), lane t its bytes [16 t, 16 t + 16).
// The tile's first and last record come from a bracketed bisection of off[].rec (fmt_record_of); the offsets of the records between
// them are staged in LDS, FMT_STAGE at a time, until a pass reaches the tile's end (a tile of 3-byte records takes FMT_MAX_PASSES - 1
// passes, a 300 kb read is one record in 150 tiles).
// A lane walks its 16 bytes run by run -- a run being bytes that lie back to back in one source (header, bases, qualities), or one
// byte the record's shape gives (lead, newline, '+', an index digit) --, loads the source bytes one by one (byte gathers: neighbouring
// lanes read neighbouring bytes of the same lines), gathers them into four registers -- its 16 bytes may lie in two passes -- and stores
// them once: one aligned 16-byte store, or single bytes where the chunk holds the text's first or last partial 16 bytes.
// Bounds: off[] is indexed up to n_reads, hdr_off[] likewise; bases / quals below off[n].base == n_bases and hdr below
// hdr_off[n] - hdr_off[0] == hdr_bytes, both verified by the caller before this launch; text below text_size == off[n].rec.
__global__ __launch_bounds__(256) void k_fmt_records(FmtLayout L, const FmtPair* __restrict__ off, const uint64_t* __restrict__ hdr_off,
                                                     uint64_t n_reads, const uint8_t* __restrict__ bases, const uint8_t* __restrict__ hdr,
                                                     const uint8_t* __restrict__ quals, uint8_t* __restrict__ text, uint64_t text_size) {
    __shared__ uint64_t s_rec[FMT_STAGE + 1], s_base[FMT_STAGE + 1], s_hdr[FMT_STAGE + 1];
    const uint32_t mis = (uint32_t)((uintptr_t)text & 15);
    const uint64_t v0 = blockIdx.x * (uint64_t)FMT_TILE;
    const uint64_t tile_lo = v0 > mis ? v0 - mis : 0, tile_hi = min64(v0 + FMT_TILE - mis, text_size);
    if (tile_lo >= tile_hi) return;                              // (the grid is sized by the text: not taken)
    const uint64_t cv = v0 + threadIdx.x * 16u;
    uint64_t c_lo = cv > mis ? cv - mis : 0, c_hi = min64(cv + 16 - mis, text_size);
    if (c_lo > c_hi) c_lo = c_hi;
    // the tile's first and last record: records are of much the same size in most files, so the first is looked for around
    // tile_lo / text_size * n_reads, the last from the first on; only the offsets of the records between them are staged
    uint64_t first = fmt_record_of(off, n_reads, tile_lo, min64((uint64_t)((double)tile_lo / (double)text_size * (double)n_reads), n_reads - 1));
    const uint64_t last = fmt_record_of(off, n_reads, tile_hi - 1, first);
    const uint64_t hdr0 = hdr_off ? hdr_off[0] : 0;
    uint64_t acc0 = 0, acc1 = 0;
    for (uint32_t pass = 0; pass < FMT_MAX_PASSES; pass++) {
        if (first > last) break;
        const uint32_t cnt = (uint32_t)min64(FMT_STAGE, last + 1 - first);
        fmt_stage(off, hdr_off, hdr0, first, cnt, s_rec, s_base, s_hdr);
        __syncthreads();
        const uint64_t p_end = s_rec[cnt];
        const uint64_t t = max64(c_lo, s_rec[0]);
        const uint64_t t_end = min64(c_hi, p_end);
        if (t < t_end) {
            uint32_t a = 0, b = cnt;                             // s_rec[a] <= t < s_rec[b]
            while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (s_rec[m] <= t) a = m; else b = m; }
            FmtRec R;
            auto enter = [&](uint32_t r) {
                R.rec0 = s_rec[r]; R.rec1 = s_rec[r + 1];
                R.bbase = s_base[r]; R.len = s_base[r + 1] - R.bbase;
                R.hbase = s_hdr[r];
                R.index = L.first_read_index + first + r;
                R.hl = hdr ? s_hdr[r + 1] - R.hbase : dec_digits(R.index);
                R.seq_text = seq_text_len(R.len, L.wrap);
            };
            enter(a);
            // run by run: which segment of which record a byte belongs to is worked out once per run, not once per byte
            uint32_t j = (uint32_t)(t + mis - cv);               // 0..15: the byte's place in the lane's 16
            const uint32_t j_end = (uint32_t)(t_end + mis - cv);
            uint64_t o = t - R.rec0;
            while (j < j_end) {
                if (o >= R.rec1 - R.rec0) { enter(++a); o = 0; }
                uint64_t end;
                uint32_t lit;
                const uint8_t* p = fmt_run(L, R, o, bases, hdr, quals, end, lit);
                const uint32_t n = (uint32_t)min64(end - o, j_end - j);
                for (uint32_t i = 0; i < n; i++, j++) {
                    const uint64_t byte = p ? p[i] : lit;
                    if (j < 8) acc0 |= byte << (8 * j); else acc1 |= byte << (8 * (j - 8));
                }
                o += n;
            }
        }
        __syncthreads();
        if (p_end >= tile_hi) break;
        first += cnt;
    }
    if (c_hi - c_lo == 16) {
        *reinterpret_cast<uint4*>(text + c_lo) = make_uint4((uint32_t)acc0, (uint32_t)(acc0 >> 32), (uint32_t)acc1, (uint32_t)(acc1 >> 32));
    } else {
        for (uint64_t t = c_lo; t < c_hi; t++) {
            const uint32_t j = (uint32_t)(t + mis - cv);
            text[t] = (uint8_t)((j < 8 ? acc0 >> (8 * j) : acc1 >> (8 * (j - 8))));
        }
    }
}

// in[n_reads + 1] = every record's (text bytes, bases) and a last (0, 0); flags[0]: the header offsets run backwards, flags[1]: they do
// not end at L.hdr_bytes (both zeroed by the caller); hdr_off == nullptr: the read index stands in for the header
void launch_fmt_sizes(hipStream_t s, const FmtLayout& L, const uint32_t* len, const uint64_t* hdr_off, uint64_t n_reads, FmtPair* in, uint32_t* flags) {
    const uint64_t blocks = (n_reads + 1 + 255) / 256;
    hipLaunchKernelGGL(k_fmt_sizes, dim3((uint32_t)blocks), dim3(256), 0, s, L, len, hdr_off, n_reads, in, flags);
}

// the text itself; the caller has verified off[n_reads] == (text_size, the bases given) and both flags of launch_fmt_sizes
void launch_fmt_records(hipStream_t s, const FmtLayout& L, const FmtPair* off, const uint64_t* hdr_off, uint64_t n_reads, const uint8_t* bases,
                        const uint8_t* hdr, const uint8_t* quals, uint8_t* text, uint64_t text_size) {
    if (!text_size) return;
    const uint64_t mis = (uintptr_t)text & 15;
    const uint64_t blocks = (mis + text_size + FMT_TILE - 1) / FMT_TILE;
    hipLaunchKernelGGL(k_fmt_records, dim3((uint32_t)blocks), dim3(FMT_THREADS), 0, s, L, off, hdr_off, n_reads, bases, hdr, quals, text, text_size);
}

}  // namespace

// (both shared with bam_kernels.hip: fmt_shared.h)
__global__ __launch_bounds__(256) void k_fmt_rec_off(const FmtPair* __restrict__ off, uint64_t n, uint64_t* __restrict__ rec_off) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r <= n) rec_off[r] = off[r].rec;
}

// exclusive, n_reads + 1 entries: out[n_reads] = the totals
hipError_t fmt_scan(void* tmp, size_t& bytes, const FmtPair* in, FmtPair* out, uint64_t n_reads, hipStream_t s) {
    return prim::ExclusiveSum(tmp, bytes, in, out, n_reads + 1, s);
}

void launch_fmt_rec_off(hipStream_t s, const FmtPair* off, uint64_t n_reads, uint64_t* rec_off) {
    const uint64_t blocks = (n_reads + 1 + 255) / 256;
    hipLaunchKernelGGL(k_fmt_rec_off, dim3((uint32_t)blocks), dim3(256), 0, s, off, n_reads, rec_off);
}

}  // namespace leon

using namespace leon;

extern "C" int leon_records_format_device(int device_id, const leon_record_layout* lay, const uint8_t* d_bases, const uint32_t* d_len, uint64_t n_reads,
                                          uint64_t n_bases, const uint8_t* d_hdr_text, const uint64_t* d_hdr_off, const uint8_t* d_quals, uint8_t* d_text,
                                          uint64_t text_cap, uint64_t* d_rec_off, uint64_t* text_size) {
    if (!lay || !text_size) return dev_fail(LEON_E_INVALID, "leon_records_format_device: null argument");
    *text_size = 0;
    if (lay->struct_size != sizeof(leon_record_layout))
        return dev_fail(LEON_E_INVALID, "leon_records_format_device: unknown struct_size " + std::to_string(lay->struct_size) + " of leon_record_layout");
    if (lay->plus_kind > 1) return dev_fail(LEON_E_INVALID, "leon_records_format_device: plus_kind must be 0 (bare) or 1 (the header again)");
    if (n_reads > (1ull << 40) || n_bases > (1ull << 46)) return dev_fail(LEON_E_INVALID, "leon_records_format_device: implausible sizes");
    if ((n_reads && !d_len) || (n_bases && !d_bases)) return dev_fail(LEON_E_INVALID, "leon_records_format_device: null argument");
    if (lay->fastq && !d_quals) return dev_fail(LEON_E_INVALID, "leon_records_format_device: FASTQ records need the qualities (d_quals)");
    if (lay->plus_kind == 1 && !d_hdr_text)
        return dev_fail(LEON_E_INVALID, "leon_records_format_device: '+' lines that repeat the header need the headers (d_hdr_text)");
    if (d_hdr_text && !d_hdr_off) return dev_fail(LEON_E_INVALID, "leon_records_format_device: headers without their offsets (d_hdr_off)");
    if (!n_reads) return LEON_OK;
    CallStream st;
    if (const int rc = dev_open("leon_records_format_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    const uint64_t* hdr_off = d_hdr_text ? d_hdr_off : nullptr;
    FmtLayout L{};
    L.first_read_index = lay->first_read_index; L.hdr_bytes = lay->hdr_bytes; L.wrap = lay->wrap;
    L.lead = lay->lead; L.fastq = lay->fastq ? 1 : 0; L.plus_kind = lay->fastq ? lay->plus_kind : 0;
    OwnBuf d_in, d_off, d_flags, d_tmp;
    DEVCHK(d_in.ensure((n_reads + 1) * sizeof(FmtPair))); DEVCHK(d_off.ensure((n_reads + 1) * sizeof(FmtPair)));
    DEVCHK(d_flags.ensure(64));
    DEVCHK(hipMemsetAsync(d_flags.p, 0, 64, s));
    launch_fmt_sizes(s, L, d_len, hdr_off, n_reads, d_in.as<FmtPair>(), d_flags.as<uint32_t>());
    DEVCHK(hipGetLastError());
    size_t tmp_bytes = 0;
    DEVCHK(fmt_scan(nullptr, tmp_bytes, d_in.as<FmtPair>(), d_off.as<FmtPair>(), n_reads, s));
    DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    DEVCHK(fmt_scan(d_tmp.p, tmp_bytes, d_in.as<FmtPair>(), d_off.as<FmtPair>(), n_reads, s));
    uint32_t flags[2] = {0, 0};
    uint64_t totals[2] = {0, 0};
    DEVCHK(hipMemcpyAsync(flags, d_flags.p, 8, hipMemcpyDeviceToHost, s));
    DEVCHK(hipMemcpyAsync(totals, d_off.as<FmtPair>() + n_reads, 16, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    // what the arrays say against what the call was told, before anything is indexed with it
    if (flags[0]) return dev_fail(LEON_E_INVALID, "leon_records_format_device: the header offsets (d_hdr_off) run backwards");
    if (flags[1]) return dev_fail(LEON_E_INVALID, "leon_records_format_device: the header offsets (d_hdr_off) do not end at the " + std::to_string(lay->hdr_bytes) + " header bytes given");
    if (totals[1] != n_bases)
        return dev_fail(LEON_E_INVALID, "leon_records_format_device: the lengths (d_len) add up to " + std::to_string(totals[1]) + " bases, not the " + std::to_string(n_bases) + " given");
    *text_size = totals[0];
    if (totals[0] > text_cap || !d_text) return dev_fail(LEON_E_OVERFLOW, "leon_records_format_device: the text needs " + std::to_string(totals[0]) + " bytes");
    launch_fmt_records(s, L, d_off.as<FmtPair>(), hdr_off, n_reads, d_bases, d_hdr_text, d_quals, d_text, totals[0]);
    DEVCHK(hipGetLastError());
    if (d_rec_off) { launch_fmt_rec_off(s, d_off.as<FmtPair>(), n_reads, d_rec_off); DEVCHK(hipGetLastError()); }
    DEVCHK(hipStreamSynchronize(s));
    return LEON_OK;
}
