// host_streams.cpp -- the host-side entry points of the C-ABI that need no GPU:
//   * HeaderDecoder over read blocks (gatb HeaderCoder.cpp [RECALLED lo]; record layout: DESIGN.md section 1.3), blocks in
//     parallel on host threads: inside a block every header is rebuilt from the one before it, so a block is one serial
//     chain, and `-d` has as many chains as the file has blocks;
//   * the quality stream in its lossless form (`-lossless`): per read block, the qualities joined by '\n' through zlib
//     (upstream: DnaEncoder buffers the block's quality lines and deflates them, Leon::writeBlockLena [RECALLED med]).
// Nothing here is on the DNA encode path; these are the streams either side of it.
#include "../../include/leon_dna.h"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host_bgzf.h"
#include "host_fastq.h"
#include "host_fasta.h"
#include "host_bam.h"

namespace leon { void set_create_error(const std::string& msg); }

namespace {

int fail(int code, const std::string& msg) { leon::set_create_error(msg); return code; }

// "all cores" = what this process may actually use: the container's CPU quota (cgroup v2 cpu.max, v1 cfs_quota) when it is
// below the number of logical CPUs -- 256 threads on a 16-CPU quota only get each other throttled
uint32_t usable_cpus() {
    uint32_t n = std::max(1u, std::thread::hardware_concurrency());
    long long quota = -1, period = -1;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64] = {0};
        if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else {
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &quota) != 1) quota = -1; fclose(g); }
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &period) != 1) period = -1; fclose(g); }
    }
    if (quota > 0 && period > 0) n = std::min<uint32_t>(n, (uint32_t)std::max<long long>(1, (quota + period - 1) / period));
    return n;
}
}  // namespace
namespace leon { uint32_t usable_cpus() { return ::usable_cpus(); } }       // (rc_kernels.hip sizes its host-chain pool by it)
namespace {

template <typename F> void parallel_blocks(uint64_t n_blocks, uint32_t n_threads, F&& f) {
    if (n_threads == 0) n_threads = usable_cpus();
    n_threads = (uint32_t)std::min<uint64_t>(n_threads, std::max<uint64_t>(n_blocks, 1));
    std::atomic<uint64_t> next{0};
    auto work = [&] { for (uint64_t b; (b = next.fetch_add(1)) < n_blocks;) f(b); };
    if (n_threads <= 1) { work(); return; }
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < n_threads; t++) th.emplace_back(work);
    for (auto& t : th) t.join();
}

// ---- Order0Model with the two-level layout of the device coder (F(x) = H[x >> 4] + Lw[x]): update touches <= 31 words ----
struct Model256 {
    uint32_t H[17], Lw[257];
    uint32_t size;
    void init(uint32_t n) { size = n; for (uint32_t x = 0; x <= 256; x++) Lw[x] = x < 256 ? (x & 15u) : 0u; for (uint32_t j = 0; j <= 16; j++) H[j] = 16 * j; }
    uint32_t F(uint32_t x) const { return H[x >> 4] + Lw[x]; }
    uint32_t total() const { return F(size); }
    uint32_t find(uint64_t value) const {                    // last c < size with F(c) <= value
        uint32_t j = 0;
        const uint32_t jmax = (size - 1) >> 4;
        while (j < jmax && H[j + 1] <= value) j++;
        uint32_t c = 16 * j;
        const uint32_t cmax = std::min(size - 1, 16 * j + 15);
        while (c < cmax && F(c + 1) <= value) c++;
        return c;
    }
    void update(uint32_t c) {                                // Order0Model::update: F(x) += 1 for x > c
        for (uint32_t x = c + 1; x <= (c | 15u); x++) Lw[x]++;
        for (uint32_t j = (c >> 4) + 1; j <= 16; j++) H[j]++;
    }
};
struct RangeDecoder {
    uint64_t low = 0, range = ~0ull, code = 0;
    const uint8_t* p; uint64_t n, i = 0;
    uint32_t past = 0;
    bool bad = false;                                         // the payload is not a stream this coder wrote (checked by the caller per header)
    RangeDecoder(const uint8_t* p_, uint64_t n_) : p(p_), n(n_) { for (int k = 0; k < 8; k++) code = (code << 8) | byte(); }
    uint8_t byte() { if (i < n) return p[i++]; past++; return 0; }   // bytes beyond the end read as 0 and are counted, the constructor's included
    uint32_t next(Model256& m) {
        range /= m.total();
        if (range == 0 || bad) { bad = true; return 0; }
        const uint32_t c = m.find((code - low) / range);
        low += (uint64_t)m.F(c) * range;
        range *= (uint64_t)(m.F(c + 1) - m.F(c));
        while ((low ^ (low + range)) < (1ull << 56) || (range < (1ull << 48) && ((range = (0 - low) & ((1ull << 48) - 1)), true))) {
            code = (code << 8) | byte();
            range <<= 8;
            low <<= 8;
            if (past > 16) { bad = true; return 0; }         // the 17th byte beyond the end, as the device's Dec (a range of 0 would spin here)
        }
        m.update(c);
        return c;
    }
};

enum { H_END = 1, H_END_MATCH, H_FIELD_ASCII, H_FIELD_NUMERIC, H_FIELD_DELTA, H_FIELD_DELTA_2, H_FIELD_ZERO_ONLY, H_FIELD_ZERO_AND_NUMERIC, H_TYPE_COUNT };

struct HeaderModels {
    Model256 type, field_index, field_column, mis_size, ascii, zero, numeric[9];
    HeaderModels() {
        type.init(H_TYPE_COUNT); field_index.init(256); field_column.init(256); mis_size.init(256); ascii.init(256); zero.init(256);
        for (auto& m : numeric) m.init(256);
    }
};
// Where the header decoder's symbols come from: the block's range-coded payload (decoded here, on a host thread), or the
// block's symbols already decoded on the device (leon_header_decode_blocks: the arithmetic decoding is the expensive part
// of a header block and a serial chain per block -- the device runs all the chains at once --, the text is not).
enum ModelId { MI_TYPE, MI_FIELD_INDEX, MI_FIELD_COLUMN, MI_MIS_SIZE, MI_ASCII, MI_ZERO, MI_NUMERIC0 };   // MI_NUMERIC0 + i: byte-count model, then one per byte
struct RangeSource {
    RangeDecoder d;
    HeaderModels* M;
    RangeSource(const uint8_t* p, uint64_t n) : d(p, n), M(new HeaderModels()) {}
    ~RangeSource() { delete M; }
    RangeSource(const RangeSource&) = delete;
    bool bad() const { return d.bad; }
    uint32_t next(uint32_t id) {
        Model256& m = id == MI_TYPE ? M->type : id == MI_FIELD_INDEX ? M->field_index : id == MI_FIELD_COLUMN ? M->field_column
                    : id == MI_MIS_SIZE ? M->mis_size : id == MI_ASCII ? M->ascii : id == MI_ZERO ? M->zero : M->numeric[id - MI_NUMERIC0];
        return d.next(m);
    }
};
struct SymbolSource {
    const uint8_t* p; uint64_t n, i = 0;
    bool over = false;
    SymbolSource(const uint8_t* p_, uint64_t n_) : p(p_), n(n_) {}
    bool bad() const { return over; }
    uint32_t next(uint32_t) { if (i < n) return p[i++]; over = true; return 0; }
};
template <typename S> uint64_t decode_numeric(S& d) {
    uint32_t bc = d.next(MI_NUMERIC0);
    if (bc > 8) bc = 8;
    uint64_t v = 0;
    for (uint32_t i = 0; i < bc; i++) v |= (uint64_t)d.next(MI_NUMERIC0 + 1 + i) << (8 * i);
    return v;
}
template <typename S> uint64_t decode_count(S& d, uint32_t id) {
    const uint64_t x = d.next(id);
    return x < 255 ? x : 255 + decode_numeric(d);
}
inline bool is_alnum(uint8_t c) { return (uint8_t)(c - '0') < 10 || (uint8_t)((c | 32) - 'a') < 26; }
struct Field { uint64_t len = 0; bool numeric = false, has_sep = false; uint8_t sep = 0; uint64_t value = 0; };
// the field of h starting at pos: token + one separator; numeric = digits without a leading zero, 1..18 of them
Field field_at(const uint8_t* h, uint64_t len, uint64_t pos) {
    Field f;
    uint64_t e = pos;
    bool digits = true;
    while (e < len && is_alnum(h[e])) { digits = digits && (uint8_t)(h[e] - '0') < 10; e++; }
    const uint64_t tok = e - pos;
    if (e < len) { f.has_sep = true; f.sep = h[e]; e++; }
    f.len = e - pos;
    if (digits && tok >= 1 && tok <= 18 && (tok == 1 || h[pos] != '0') && !(f.has_sep && f.sep == 0)) {
        f.numeric = true;
        for (uint64_t i = pos; i < pos + tok; i++) f.value = f.value * 10 + (uint64_t)(h[i] - '0');
    }
    return f;
}

// one block; out receives the headers back to back, off[n + 1] (relative to out); false when the payload does not decode
template <typename S>
bool decode_header_block(S& d, uint32_t n, const uint8_t* first, uint64_t first_len, std::string& out, std::vector<uint64_t>& off) {
    out.clear(); off.assign(1, 0);
    std::string prev(reinterpret_cast<const char*>(first), first_len), cur;
    const uint64_t max_header = 1ull << 31;
    for (uint32_t r = 0; r < n; r++) {
        cur.clear();
        const uint8_t* ph = reinterpret_cast<const uint8_t*>(prev.data());
        const uint64_t lp = prev.size();
        uint64_t pp = 0, nf = 0;
        auto copy_prev_until = [&](uint64_t limit) {             // fields nf .. limit-1 are the previous header's
            while (nf < limit && pp < lp) { const Field p = field_at(ph, lp, pp); cur.append(prev, pp, p.len); pp += p.len; nf++; }
        };
        for (;;) {
            const uint32_t t = d.next(MI_TYPE);
            if (d.bad()) return false;
            if (t == H_END_MATCH) { copy_prev_until(~0ull); break; }
            if (t == H_END) {
                const uint64_t f = decode_count(d, MI_FIELD_INDEX);
                if (f < nf) return false;
                copy_prev_until(f);
                if (nf != f) return false;
                break;
            }
            if (t < H_FIELD_ASCII || t >= H_TYPE_COUNT) return false;
            const uint64_t idx = decode_count(d, MI_FIELD_INDEX);
            if (idx < nf) return false;
            copy_prev_until(idx);
            if (nf != idx) return false;
            Field p;
            const bool have_p = pp < lp;
            const uint64_t p0 = pp;
            if (have_p) { p = field_at(ph, lp, pp); pp += p.len; }
            if (t == H_FIELD_ASCII) {
                const uint64_t col = decode_count(d, MI_FIELD_COLUMN), sz = decode_count(d, MI_MIS_SIZE);
                if (col > p.len || sz > max_header || cur.size() + col + sz > max_header) return false;
                cur.append(prev, p0, col);
                for (uint64_t j = 0; j < sz && !d.bad(); j++) cur.push_back((char)d.next(MI_ASCII));
            } else {
                uint64_t v = 0, z = 0; uint8_t sep = 0; bool has_sep = false;
                if (t == H_FIELD_DELTA || t == H_FIELD_DELTA_2) {
                    const uint64_t dv = decode_numeric(d);
                    if (!have_p || !p.numeric) return false;
                    v = t == H_FIELD_DELTA ? p.value + dv : p.value - dv;
                    sep = p.sep; has_sep = p.has_sep;
                } else {
                    if (t != H_FIELD_NUMERIC) z = decode_count(d, MI_ZERO);
                    if (t != H_FIELD_ZERO_ONLY) v = decode_numeric(d);
                    sep = (uint8_t)d.next(MI_ASCII); has_sep = sep != 0;
                }
                if (z > max_header || cur.size() + z > max_header) return false;
                cur.append(z, '0');
                if (t != H_FIELD_ZERO_ONLY) cur += std::to_string(v);
                if (has_sep) cur.push_back((char)sep);
            }
            nf++;
        }
        out += cur;
        off.push_back(out.size());
        prev.swap(cur);
    }
    return true;
}

// blocks in parallel on host threads, then the texts back to back with the offsets of every header
template <typename F>
int header_blocks_common(uint64_t n_blocks, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint64_t* out_size, uint32_t n_threads, F&& decode_one) {
    std::vector<std::string> texts(n_blocks);
    std::vector<std::vector<uint64_t>> offs(n_blocks);
    std::atomic<int64_t> bad{-1};
    parallel_blocks(n_blocks, n_threads, [&](uint64_t b) {
        if (!decode_one(b, texts[b], offs[b])) {
            int64_t expect = -1;
            bad.compare_exchange_strong(expect, (int64_t)b);
        }
    });
    if (bad.load() >= 0) return fail(LEON_E_INVALID, "header block " + std::to_string(bad.load()) + " does not decode");
    uint64_t w = 0;
    for (uint64_t b = 0; b < n_blocks; b++) w += texts[b].size();
    *out_size = w;
    if (w > out_cap || !out) return fail(LEON_E_OVERFLOW, "header output needs " + std::to_string(w) + " bytes");
    // every block's text and offsets to their final places, again by all threads (gigabytes: not a job for one core)
    std::vector<uint64_t> w0(n_blocks + 1, 0), r0(n_blocks + 1, 0);
    for (uint64_t b = 0; b < n_blocks; b++) { w0[b + 1] = w0[b] + texts[b].size(); r0[b + 1] = r0[b] + (offs[b].empty() ? 0 : offs[b].size() - 1); }
    out_off[0] = 0;
    parallel_blocks(n_blocks, n_threads, [&](uint64_t b) {
        if (!texts[b].empty()) memcpy(out + w0[b], texts[b].data(), texts[b].size());
        for (size_t i = 1; i < offs[b].size(); i++) out_off[r0[b] + i] = w0[b] + offs[b][i];
        std::string().swap(texts[b]);
    });
    return LEON_OK;
}

}  // namespace

namespace leon {
// the text of header blocks whose symbols the device has decoded (hdr_kernels.hip, leon_header_decode_blocks): block b's symbols are
// syms[sym_begin[b] .. + sym_count[b]), one byte each, in the order the HeaderDecoder asks for them
int header_blocks_from_symbols(const uint8_t* syms, const uint64_t* sym_begin, const uint64_t* sym_count, const uint32_t* block_n_reads, uint64_t n_blocks,
                               const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                               uint64_t* out_size, uint32_t n_threads) {
    return header_blocks_common(n_blocks, out, out_cap, out_off, out_size, n_threads, [&](uint64_t b, std::string& text, std::vector<uint64_t>& off) {
        SymbolSource src(syms + sym_begin[b], sym_count[b]);
        return decode_header_block(src, block_n_reads[b], first_header, first_header_len, text, off) && !src.over && src.i == src.n;
    });
}
}  // namespace leon

extern "C" {

int leon_host_header_decode_blocks(const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads, uint64_t n_blocks,
                                   const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_off, uint64_t* out_size, uint32_t n_threads) {
    if (!out_size || (n_blocks && (!payloads || !payload_off || !block_n_reads || !out_off)) || (!first_header && first_header_len))
        return fail(LEON_E_INVALID, "null argument");
    *out_size = 0;
    if (!n_blocks) return LEON_OK;
    for (uint64_t b = 0; b < n_blocks; b++)
        if (payload_off[b + 1] < payload_off[b]) return fail(LEON_E_INVALID, "payload offsets are not monotonic");
    return header_blocks_common(n_blocks, out, out_cap, out_off, out_size, n_threads, [&](uint64_t b, std::string& text, std::vector<uint64_t>& off) {
        RangeSource src(payloads + payload_off[b], payload_off[b + 1] - payload_off[b]);
        return decode_header_block(src, block_n_reads[b], first_header, first_header_len, text, off) && !src.bad();   // (a block's last symbols are checked here)
    });
}

// ---- quality stream, lossless: one zlib stream per read block over the block's quality lines, each followed by '\n' ----
int leon_host_qual_encode_blocks(const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads, uint32_t reads_per_block,
                                 int zlib_level, uint32_t n_threads, leon_block_sink sink, void* user, uint64_t first_block_id) {
    if ((n_reads && (!quals || !offsets)) || !sink || !reads_per_block) return fail(LEON_E_INVALID, "null argument");
    if (zlib_level < -1 || zlib_level > 9) return fail(LEON_E_INVALID, "zlib level must be in -1..9");
    const uint64_t n_blocks = (n_reads + reads_per_block - 1) / reads_per_block;
    for (uint64_t i = 0; i < n_reads; i++)
        if (offsets[i + 1] < offsets[i]) return fail(LEON_E_INVALID, "offsets are not monotonic");
    std::vector<std::vector<uint8_t>> outs(n_blocks);
    std::atomic<int> zerr{0};
    parallel_blocks(n_blocks, n_threads, [&](uint64_t b) {
        const uint64_t r0 = b * reads_per_block, r1 = std::min<uint64_t>(n_reads, r0 + reads_per_block);
        std::vector<uint8_t> text;
        text.reserve((size_t)(offsets[r1] - offsets[r0] + (r1 - r0)));
        for (uint64_t r = r0; r < r1; r++) {
            text.insert(text.end(), quals + offsets[r], quals + offsets[r + 1]);
            text.push_back('\n');
        }
        uLongf cap = compressBound((uLong)text.size());
        outs[b].resize(cap);
        if (compress2(outs[b].data(), &cap, text.data(), (uLong)text.size(), zlib_level) != Z_OK) zerr.store(1);
        outs[b].resize(cap);
    });
    if (zerr.load()) return fail(LEON_E_INVALID, "zlib compress2 failed");
    for (uint64_t b = 0; b < n_blocks; b++) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(reads_per_block, n_reads - b * reads_per_block);
        if (sink(user, first_block_id + b, outs[b].data(), outs[b].size(), nr)) return fail(LEON_E_SINK, "block sink returned non-zero");
    }
    return LEON_OK;
}

int leon_host_qual_decode_blocks(const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                                 const uint64_t* block_n_bytes, uint64_t n_blocks, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                 uint32_t n_threads) {
    if (n_blocks && (!payloads || !payload_off || !block_n_reads || !block_n_bytes || !out || !out_off)) return fail(LEON_E_INVALID, "null argument");
    if (!n_blocks) return LEON_OK;
    // block_n_bytes: quality bytes per block WITHOUT the newlines (what the container's block table records)
    std::vector<uint64_t> o0(n_blocks + 1, 0), r0(n_blocks + 1, 0);
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (payload_off[b + 1] < payload_off[b]) return fail(LEON_E_INVALID, "payload offsets are not monotonic");
        o0[b + 1] = o0[b] + block_n_bytes[b];
        r0[b + 1] = r0[b] + block_n_reads[b];
        if (o0[b + 1] < o0[b] || o0[b + 1] > out_cap) return fail(LEON_E_INVALID, "output capacity below the sum of block_n_bytes");
    }
    std::atomic<int64_t> bad{-1};
    parallel_blocks(n_blocks, n_threads, [&](uint64_t b) {
        std::vector<uint8_t> text((size_t)(block_n_bytes[b] + block_n_reads[b]));
        uLongf got = (uLongf)text.size();
        bool ok = uncompress(text.data(), &got, payloads + payload_off[b], (uLong)(payload_off[b + 1] - payload_off[b])) == Z_OK && got == text.size();
        uint64_t w = o0[b], r = r0[b], at = 0;
        if (ok && b == 0) out_off[0] = 0;
        for (uint32_t i = 0; ok && i < block_n_reads[b]; i++) {
            const uint8_t* nl = (const uint8_t*)memchr(text.data() + at, '\n', text.size() - at);
            if (!nl) { ok = false; break; }
            const uint64_t len = (uint64_t)(nl - (text.data() + at));
            if (w + len > o0[b + 1]) { ok = false; break; }
            memcpy(out + w, text.data() + at, len);
            w += len; at += len + 1;
            out_off[++r] = w;
        }
        if (ok && (w != o0[b + 1] || at != text.size())) ok = false;
        // the SMALLEST failing block is the one named, whichever thread fails first
        if (!ok) { int64_t seen = bad.load(); while ((seen < 0 || (int64_t)b < seen) && !bad.compare_exchange_weak(seen, (int64_t)b)) {} }
    });
    if (bad.load() >= 0) return fail(LEON_E_INVALID, "quality block " + std::to_string(bad.load()) + " does not decode");
    return LEON_OK;
}

}  // extern "C"

// ---- zlib's CRC-32 of segments of a buffer: the host form of leon_crc32_segments_device ----
namespace leon {
// what both forms refuse, in the same words; nullptr: the arguments are in order.  Reads seg_off only.
const char* crc32_segments_refusal(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, const uint32_t* crc) {
    if (!n_seg) return nullptr;
    if (!seg_off || !crc) return "crc32 segments: null argument";
    for (uint64_t s = 0; s < n_seg; s++)
        if (seg_off[s + 1] < seg_off[s]) return "crc32 segments: segment offsets are not monotonic";
    if (seg_off[n_seg] > n_bytes) return "crc32 segments: the segments end behind the bytes given";
    if (n_bytes >> 62) return "crc32 segments: implausible sizes";
    if (seg_off[n_seg] > seg_off[0] && !bytes) return "crc32 segments: null argument";
    return nullptr;
}
}  // namespace leon

int leon_host_crc32_segments(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, uint32_t n_threads, uint32_t* crc) {
    if (const char* why = leon::crc32_segments_refusal(bytes, n_bytes, seg_off, n_seg, crc)) return fail(LEON_E_INVALID, why);
    // pieces of at most 4 MiB, so that one long segment is shared among the threads too; zlib's crc32_combine joins them
    constexpr uint64_t kPiece = 4ull << 20;
    struct Piece { uint64_t at, size; uint32_t crc; };
    std::vector<Piece> pieces;
    std::vector<uint64_t> first(n_seg + 1, 0);
    for (uint64_t s = 0; s < n_seg; s++) {
        for (uint64_t at = seg_off[s]; at < seg_off[s + 1]; at += kPiece) pieces.push_back(Piece{at, std::min(kPiece, seg_off[s + 1] - at), 0});
        first[s + 1] = pieces.size();
    }
    parallel_blocks(pieces.size(), n_threads, [&](uint64_t i) {
        pieces[i].crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), bytes + pieces[i].at, (uInt)pieces[i].size);
    });
    for (uint64_t s = 0; s < n_seg; s++) {
        uLong c = crc32(0L, Z_NULL, 0);
        for (uint64_t i = first[s]; i < first[s + 1]; i++) c = i == first[s] ? pieces[i].crc : crc32_combine(c, pieces[i].crc, (z_off_t)pieces[i].size);
        crc[s] = (uint32_t)c;
    }
    return LEON_OK;
}

// ---- BGZF input: the member walk, and the host form of leon_bgzf_inflate_device ----
namespace leon {

// The member that begins at p, of which `avail` bytes are in sight: 1f 8b 08, FLG exactly 4, XLEN, the subfields walked for
// B C 02 00 BSIZE (others in front of it are skipped), BSIZE + 1 at least the header and the 8-byte trailer.
// BGZF_MEMBER: *size = BSIZE + 1 <= avail, *pay0 = 12 + XLEN; BGZF_PARTIAL: nothing in sight contradicts a member, but it does not end
// inside the bytes in sight; BGZF_FOREIGN: not a BGZF member.
int bgzf_header(const uint8_t* p, uint64_t avail, uint64_t* size, uint64_t* pay0) {
    static const uint8_t magic[4] = {0x1f, 0x8b, 0x08, 0x04};
    for (uint64_t i = 0; i < 4 && i < avail; i++) if (p[i] != magic[i]) return BGZF_FOREIGN;
    if (avail < 12) return BGZF_PARTIAL;
    const uint64_t xlen = p[10] | (uint64_t)p[11] << 8, head = 12 + xlen;
    if (head + 8 > 65536) return BGZF_FOREIGN;                   // (BSIZE has 16 bits)
    if (avail < head) return BGZF_PARTIAL;
    uint64_t bsize = ~0ull;
    for (uint64_t at = 12; at + 4 <= head;) {
        const uint64_t slen = p[at + 2] | (uint64_t)p[at + 3] << 8;
        if (at + 4 + slen > head) return BGZF_FOREIGN;
        if (p[at] == 'B' && p[at + 1] == 'C' && slen == 2) { bsize = p[at + 4] | (uint64_t)p[at + 5] << 8; break; }
        at += 4 + slen;
    }
    if (bsize == ~0ull || bsize + 1 < head + 8) return BGZF_FOREIGN;
    if (bsize + 1 > avail) return BGZF_PARTIAL;
    *size = bsize + 1; *pay0 = head;
    return BGZF_MEMBER;
}

// What both forms of the inflate refuse, in the same words, before anything is decoded; fills m (a member that is no BGZF member of
// exactly its span, or whose ISIZE is above 65 536, is marked !ok and counts no text: it "does not decode" when its turn comes) and
// *n_text.  LEON_OK, or the code with `why`.
int bgzf_prepare(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* member_off, uint64_t n_members, const void* text, uint64_t text_cap,
                 uint64_t* n_text, std::vector<BgzfMember>& m, std::string& why) {
    if (!n_text) { why = "BGZF inflate: null argument"; return LEON_E_INVALID; }
    *n_text = 0;
    m.clear();
    if (!n_members) return LEON_OK;
    if (!bytes || !member_off) { why = "BGZF inflate: null argument"; return LEON_E_INVALID; }
    if (n_members >> 31) { why = "BGZF inflate: implausible number of members"; return LEON_E_INVALID; }
    for (uint64_t i = 0; i < n_members; i++)
        if (member_off[i + 1] < member_off[i]) { why = "BGZF inflate: member offsets are not monotonic"; return LEON_E_INVALID; }
    if (member_off[n_members] > n_bytes) { why = "BGZF inflate: the members end behind the bytes given"; return LEON_E_INVALID; }
    m.resize(n_members);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_members; i++) {
        const uint64_t at = member_off[i], span = member_off[i + 1] - at;
        uint64_t size = 0, pay0 = 0;
        BgzfMember& M = m[i];
        M = BgzfMember{at, 0, total, 0, 0, 0, false};
        if (bgzf_header(bytes + at, span, &size, &pay0) != BGZF_MEMBER || size != span) continue;
        const uint8_t* t = bytes + at + span - 8;
        M.crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (isize > 65536) continue;
        M.pay0 = at + pay0; M.pay_size = span - pay0 - 8; M.isize = isize; M.ok = true;
        total += isize;
    }
    *n_text = total;
    if (total > text_cap || (total && !text)) { why = "BGZF inflate: the text needs " + std::to_string(total) + " bytes"; return LEON_E_OVERFLOW; }
    return LEON_OK;
}
std::string bgzf_refusal(uint64_t member, uint64_t at) {
    return "BGZF member " + std::to_string(member) + " (at byte " + std::to_string(at) + ") does not decode";
}

}  // namespace leon

int leon_host_bgzf_members(const uint8_t* bytes, uint64_t n_bytes, int last, uint64_t* member_off, uint64_t off_cap, uint64_t* n_members,
                           uint64_t* n_text, uint64_t* consumed, uint32_t* stop) {
    if (!n_members || !n_text || !consumed || !stop || (n_bytes && !bytes) || (off_cap && !member_off) || (last != 0 && last != 1))
        return fail(LEON_E_INVALID, "BGZF members: null argument, or a `last` other than 0 or 1");
    uint64_t at = 0, n = 0, text = 0;
    uint32_t why = LEON_BGZF_WHOLE;
    while (at < n_bytes) {
        uint64_t size = 0, pay0 = 0;
        const int kind = leon::bgzf_header(bytes + at, n_bytes - at, &size, &pay0);
        if (kind == leon::BGZF_PARTIAL) { why = last ? LEON_BGZF_TRUNCATED : LEON_BGZF_PARTIAL; break; }
        if (kind == leon::BGZF_FOREIGN) { why = LEON_BGZF_FOREIGN; break; }
        const uint8_t* t = bytes + at + size - 4;
        const uint32_t isize = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if (isize <= 65536) text += isize;                       // (a larger one is refused by the inflate: it counts no text there either)
        if (n < off_cap) member_off[n] = at;
        n++; at += size;
    }
    if (n < off_cap) member_off[n] = at;
    *n_members = n; *n_text = text; *consumed = at; *stop = why;
    if (n + 1 > off_cap) return fail(LEON_E_OVERFLOW, "BGZF members: the table needs " + std::to_string(n + 1) + " entries");
    if (why == LEON_BGZF_TRUNCATED) return fail(LEON_E_INVALID, "BGZF member " + std::to_string(n) + " (at byte " + std::to_string(at) + ") is truncated");
    if (why == LEON_BGZF_FOREIGN) return fail(LEON_E_INVALID, "no BGZF member at byte " + std::to_string(at) + " (member " + std::to_string(n) + ")");
    return LEON_OK;
}

int leon_host_bgzf_inflate(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* member_off, uint64_t n_members, uint8_t* text, uint64_t text_cap,
                           uint64_t* n_text, uint32_t n_threads) {
    std::vector<leon::BgzfMember> m;
    std::string why;
    if (const int rc = leon::bgzf_prepare(bytes, n_bytes, member_off, n_members, text, text_cap, n_text, m, why)) return fail(rc, why);
    std::atomic<uint64_t> bad{~0ull};
    parallel_blocks(n_members, n_threads, [&](uint64_t i) {
        const leon::BgzfMember& M = m[i];
        bool ok = M.ok;
        if (ok) {
            uint8_t none = 0;
            uint8_t* const dst = M.isize ? text + M.text0 : &none;
            z_stream z{};
            ok = inflateInit2(&z, -15) == Z_OK;
            if (ok) {
                z.next_in = const_cast<Bytef*>(bytes + M.pay0); z.avail_in = (uInt)M.pay_size;
                z.next_out = dst; z.avail_out = (uInt)M.isize;
                // the stream ends with the payload's last byte and gives exactly ISIZE bytes, whose CRC-32 is the trailer's
                ok = inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_in == 0 && z.total_out == M.isize;
                inflateEnd(&z);
                ok = ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, (uInt)M.isize) == M.crc;
            }
        }
        if (!ok) { uint64_t seen = bad.load(); while (i < seen && !bad.compare_exchange_weak(seen, i)) {} }
    });
    if (bad.load() != ~0ull) return fail(LEON_E_INVALID, leon::bgzf_refusal(bad.load(), member_off[bad.load()]));
    return LEON_OK;
}

// ---- lower-case runs and bytes outside ACGTN put back: the host form of leon_letters_apply_device ----
namespace leon {
// what both forms refuse, in the same words; nullptr: the tables are in order.  Reads the tables only.
const char* letters_tables_refusal(const uint8_t* bases, uint64_t n_bytes, const uint64_t* runs, uint64_t n_runs, const uint64_t* odd_pos,
                                   const uint8_t* odd_byte, uint64_t n_odd) {
    if ((n_runs && !runs) || (n_odd && (!odd_pos || !odd_byte))) return "letters: null argument";
    if ((n_bytes >> 62) || (n_runs >> 58) || (n_odd >> 58)) return "letters: implausible sizes";
    for (uint64_t r = 0; r < n_runs; r++) {
        if (runs[2 * r] >= runs[2 * r + 1]) return "letters: a run is empty or runs backwards";
        if (runs[2 * r + 1] > n_bytes) return "letters: a run ends behind the bytes given";
        if (r && runs[2 * r - 1] > runs[2 * r]) return "letters: the runs overlap or are not ascending";
    }
    for (uint64_t i = 0; i < n_odd; i++) {
        if (odd_pos[i] >= n_bytes) return "letters: a position lies behind the bytes given";
        if (i && odd_pos[i - 1] >= odd_pos[i]) return "letters: the positions are not strictly ascending";
    }
    if ((n_runs || n_odd) && !bases) return "letters: null argument";
    return nullptr;
}
}  // namespace leon

int leon_host_letters_apply(uint8_t* bases, uint64_t n_bytes, const uint64_t* runs, uint64_t n_runs, const uint64_t* odd_pos, const uint8_t* odd_byte,
                            uint64_t n_odd, uint32_t n_threads) {
    if (const char* why = leon::letters_tables_refusal(bases, n_bytes, runs, n_runs, odd_pos, odd_byte, n_odd)) return fail(LEON_E_INVALID, why);
    // the case first, then the bytes: a lower-case odd byte inside a run is its own record's.  Pieces of 4 MiB of the buffer, so that
    // one long run is shared among the threads; a piece looks its first run up
    constexpr uint64_t kPiece = 4ull << 20;
    if (n_runs) {
        const uint64_t first = runs[0] / kPiece, last = (runs[2 * n_runs - 1] - 1) / kPiece;
        parallel_blocks(last - first + 1, n_threads, [&](uint64_t i) {
            const uint64_t a = (first + i) * kPiece, b = std::min(n_bytes, a + kPiece);
            uint64_t lo = 0, hi = n_runs;                         // the first run that ends behind a
            while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (runs[2 * mid + 1] > a) hi = mid; else lo = mid + 1; }
            for (uint64_t r = lo; r < n_runs && runs[2 * r] < b; r++)
                for (uint64_t p = std::max(a, runs[2 * r]), e = std::min(b, runs[2 * r + 1]); p < e; p++)
                    if ((uint8_t)(bases[p] - 'A') < 26) bases[p] |= 0x20;
        });
    }
    constexpr uint64_t kRecords = 1ull << 16;
    parallel_blocks((n_odd + kRecords - 1) / kRecords, n_threads, [&](uint64_t i) {
        for (uint64_t j = i * kRecords, e = std::min(n_odd, j + kRecords); j < e; j++) bases[odd_pos[j]] = odd_byte[j];
    });
    return LEON_OK;
}

// ---- BGZF members cut at record starts: the host form of k_bgzf_cuts' rule ----
namespace leon {
// what leon_text_bgzf_records_device and leon_host_bgzf_record_cuts both refuse, in the same words; nullptr: the arguments are in order
const char* bgzf_records_refusal(bool have_off, uint64_t n_records, uint64_t n_head, uint64_t n_body, int last) {
    if (last != 0 && last != 1) return "bgzf records: last is neither 0 nor 1";
    if (n_head > LEON_BGZF_MEMBER_TEXT) return "bgzf records: n_head is above LEON_BGZF_MEMBER_TEXT";
    if (n_records && !have_off) return "bgzf records: records given with rec_off NULL";
    if (!n_records && n_body && (have_off || n_head)) return "bgzf records: n_body != 0 without records in record mode";
    if ((n_records >> 58) || (n_body >> 62)) return "bgzf records: implausible sizes";
    return nullptr;
}
// flags: 1 the offsets run backwards or stand still somewhere, 2 the first is not 0, 4 the last is not n_body
const char* bgzf_offsets_refusal(uint32_t flags) {
    if (flags & 2u) return "bgzf records: the record offsets do not start at 0";
    if (flags & 1u) return "bgzf records: the record offsets are not strictly ascending";
    if (flags & 4u) return "bgzf records: the record offsets do not end at n_body";
    return nullptr;
}
}  // namespace leon

int leon_host_bgzf_record_cuts(const uint64_t* rec_off, uint64_t n_records, uint64_t n_head, int last, uint64_t* begin, uint32_t* len,
                               uint64_t cap, uint64_t* n_members, uint64_t* n_taken) {
    constexpr uint64_t W = LEON_BGZF_MEMBER_TEXT;
    if (!n_members || !n_taken) return fail(LEON_E_INVALID, "bgzf records: n_members or n_taken is NULL");
    *n_members = 0; *n_taken = 0;
    if ((begin == nullptr) != (len == nullptr) || (!begin && cap)) return fail(LEON_E_INVALID, "bgzf records: a half-given member table");
    if (n_records && !rec_off) return fail(LEON_E_INVALID, leon::bgzf_records_refusal(false, n_records, n_head, 0, last));
    const uint64_t n_body = rec_off ? rec_off[n_records] : 0;
    if (const char* why = leon::bgzf_records_refusal(rec_off != nullptr, n_records, n_head, n_body, last)) return fail(LEON_E_INVALID, why);
    uint32_t flags = rec_off && rec_off[0] != 0 ? 2u : 0u;
    for (uint64_t r = 0; r < n_records; r++) if (rec_off[r + 1] <= rec_off[r]) { flags |= 1u; break; }
    if (const char* why = leon::bgzf_offsets_refusal(flags)) return fail(LEON_E_INVALID, why);
    // the record starts of the call's text: 0 when there is a head (one record as far as the rule goes), then the body's
    const uint64_t hs = n_head ? 1 : 0, n_starts = hs + n_records + 1, n_text = n_head + n_body;
    auto S = [&](uint64_t k) { return k < hs ? 0 : n_head + (rec_off ? rec_off[k - hs] : 0); };
    uint64_t n = 0, k = 0;
    auto emit = [&](uint64_t a, uint64_t m) { if (n < cap) { begin[n] = a; len[n] = (uint32_t)m; } n++; };
    while (k + 1 < n_starts) {
        const uint64_t p = S(k);
        if (!last && n_text - p <= W) break;
        const uint64_t next = S(k + 1);
        if (next - p > W) {                                       // an oversized record: members of its own
            for (uint64_t a = p; a < next; a += W) emit(a, std::min(W, next - a));
            k++;
            continue;
        }
        uint64_t lo = k + 1, hi = std::min(n_starts - 1, k + W);  // the largest start <= p + W (records have at least one byte)
        while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (S(mid) <= p + W) lo = mid; else hi = mid - 1; }
        emit(p, S(lo) - p);
        k = lo;
    }
    *n_members = n; *n_taken = S(k);
    if (n > 3 * (n_text / W) + 2) return fail(LEON_E_OVERFLOW, "bgzf records: more members than the bound allows");
    if (begin && n > cap) return fail(LEON_E_OVERFLOW, "bgzf records: the member table needs " + std::to_string(n) + " entries");
    return LEON_OK;
}

// ---- FASTQ text split into records: the host form of leon_fastq_split_device, the loop itself in host_fastq.h ----
extern "C"
int leon_host_fastq_split(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, int plus_kind, uint8_t* headers,
                          uint64_t* header_off, uint8_t* bases, uint64_t* base_off, uint8_t* quals, uint64_t bytes_cap, uint64_t records_cap,
                          leon_fastq_split_result* res) {
    if (const char* why = leon::fastq_split_refusal(text, n_text, plus_kind, headers, header_off, bases, base_off, quals, res))
        return fail(LEON_E_INVALID, std::string("leon_host_fastq_split: ") + why);
    const int rc = leon::fastq_split(text, n_text, last, max_records, plus_kind, headers, header_off, bases, base_off, quals, bytes_cap, records_cap, res);
    if (rc == LEON_E_OVERFLOW)
        return fail(rc, "leon_host_fastq_split: " + std::to_string(res->n_records) + " records need " + std::to_string(res->header_bytes) + " header bytes, " +
                            std::to_string(res->base_bytes) + " bases and " + std::to_string(res->n_records + 1) + " table entries");
    return rc;
}

// ---- FASTA text split into records: the host form of leon_fasta_split_device, the loop itself in host_fasta.h ----
extern "C"
int leon_host_fasta_split(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap, uint8_t* headers, uint64_t* header_off,
                          uint8_t* bases, uint64_t* base_off, uint64_t bytes_cap, uint64_t records_cap, leon_fasta_split_result* res) {
    if (const char* why = leon::fasta_split_refusal(text, n_text, headers, header_off, bases, base_off, res))
        return fail(LEON_E_INVALID, std::string("leon_host_fasta_split: ") + why);
    const int rc = leon::fasta_split(text, n_text, last, max_records, wrap, headers, header_off, bases, base_off, bytes_cap, records_cap, res);
    if (rc == LEON_E_OVERFLOW)
        return fail(rc, "leon_host_fasta_split: " + std::to_string(res->n_records) + " records need " + std::to_string(res->header_bytes) + " header bytes, " +
                            std::to_string(res->base_bytes) + " bases and " + std::to_string(res->n_records + 1) + " table entries");
    return rc;
}

extern "C"
int leon_host_records_bam(const leon_record_layout* lay, const uint8_t* bases, const uint32_t* len, uint64_t n_reads, uint64_t n_bases, const uint8_t* hdr_text,
                          const uint64_t* hdr_off, const uint8_t* quals, uint8_t* out, uint64_t out_cap, uint64_t* rec_off, uint64_t* out_size,
                          uint32_t n_threads) {
    static const char* const who = "leon_host_records_bam";
    if (out_size) *out_size = 0;
    std::string why = leon::bam_args_refusal(who, lay, bases, len, n_reads, n_bases, hdr_text, hdr_off, out_size);
    if (!why.empty()) return fail(LEON_E_INVALID, why);
    const int rc = leon::bam_records_host(who, lay, bases, len, n_reads, n_bases, hdr_text, hdr_off, quals, out, out_cap, rec_off, out_size,
                                          n_threads ? n_threads : usable_cpus(), why);
    return rc ? fail(rc, why) : LEON_OK;
}

extern "C"
int leon_bam_header(uint8_t* out, uint64_t cap, uint64_t* size) {
    if (!size) return fail(LEON_E_INVALID, "leon_bam_header: size is NULL");
    const std::string h = leon::bam_header_bytes();
    *size = h.size();
    if (h.size() > cap || !out) return fail(LEON_E_OVERFLOW, "leon_bam_header: the header needs " + std::to_string(h.size()) + " bytes");
    memcpy(out, h.data(), h.size());
    return LEON_OK;
}
