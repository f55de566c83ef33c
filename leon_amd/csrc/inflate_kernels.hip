// inflate_kernels.hip -- the quality blocks inflated on the device (leon_qual_inflate_blocks_device).
//
// A quality block is one zlib stream (RFC 1950 around RFC 1951) over the block's quality lines, each followed by '\n'.
//   k_qual_inflate   one wave per block: the stream's symbol chain, run uniformly by the wave; the lanes build the decode tables,
//                    copy the matches and the stored blocks, and store the text 1 KiB at a time.  The last 32 KiB of the text -- the
//                    window a match may reach into -- live in an LDS ring: LDS operations of one wave execute in order, so a match
//                    reads what the instructions before it wrote without waiting for anything.
//   k_qual_tiles     every 4 KiB tile of every block's text: its newlines, and its share of the block's Adler-32 (the sums are
//                    written so that they ADD across tiles: s1 = sum d[i], s2 = sum (n - i) d[i], both mod 65521)
//   k_qual_check     a thread per block: newlines == reads, the last byte a newline, the Adler-32 against the stream's own
//   k_qual_lines     every tile again: the text without its newlines to d_quals (through LDS, aligned 16-byte stores), the reads' offsets
//   k_qual_lens      (d_len given) a lane per read: its line's length against d_len
// The verdict is the one of leon_host_qual_decode_blocks (zlib's uncompress and the line rules), host_streams.cpp.
//
// The same decoder (qi_stream) reads the members of a BGZF file (leon_bgzf_inflate_device):
//   k_bgzf_inflate   one wave per member, a raw RFC 1951 stream into the member's 16-byte aligned share of a temporary
//   k_bgzf_gather    every 4 KiB tile of every share to its place in the contiguous text (through LDS, aligned 16-byte stores)
// with the members' CRC-32 taken over the temporary by crc_kernels.hip.  The verdict is leon_host_bgzf_inflate's.
#include "kernels.h"
#include "prim.h"
#include "device_call.h"
#include "staging.h"
#include "host_bgzf.h"

#include <algorithm>
#include <vector>

namespace leon {

// a block of one launch: its payload in the launch's payload buffer, its share of the temporary text (16-byte aligned, text_size =
// its quality bytes + its reads: the lines with their newlines), its first 4 KiB tile of the text, its place in d_quals and d_qual_off.
// A BGZF member is a QiBlock too: pay0 / pay_size = its raw deflate stream in the launch's payload buffer, text0 = its 16-byte aligned
// share of the temporary, text_size = its ISIZE, tile0 = its first 4 KiB tile, q0 = its first byte in the contiguous text (read0, n_reads: 0).
struct QiBlock { uint64_t pay0, pay_size, text0, text_size, tile0, q0, read0, n_reads; };
enum : uint32_t { QI_OK = 0, QI_HEADER = 1, QI_TYPE = 2, QI_STORED = 3, QI_TABLE = 4, QI_CODE = 5, QI_DIST = 6, QI_LONG = 7, QI_EARLY = 8,
                  QI_SHORT = 9, QI_LINES = 10, QI_ADLER = 11, QI_SLACK = 12 /* (BGZF) bytes between the stream's end and the trailer */ };

namespace {

constexpr uint32_t QI_RING = 32768, QI_RMASK = QI_RING - 1;      // deflate's window
constexpr uint32_t QI_LBITS = 10, QI_DBITS = 9;                  // primary look-up: literal/length, distance (longer codes: the canonical walk)
constexpr uint32_t QI_FLUSH = 1024;                              // 64 lanes x 16 bytes
constexpr uint32_t ADLER_P = 65521;

__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};     // RFC 1951, 3.2.7

#define QI_WAVE_ORDER() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ uint32_t qi_uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// The stream's bits: the payload through a 2 x 256-byte register window (a dword per lane, the second window loaded while the first
// is consumed), 33..64 bits of it in a uniform 64-bit buffer.  Nothing is loaded outside [0, n_words) of the payload buffer; bits
// beyond the block's own payload may be read into the buffer (they belong to the next block, or are the buffer's padding), but
// `left` -- the bits of the block not yet consumed -- goes negative when one of them is consumed, and every caller checks it before
// it acts on what it decoded.
struct QiBits {
    const uint32_t* words; uint64_t n_words;
    uint32_t w0, w1;                 // per lane
    uint64_t next;                   // word index of w1's lane 0
    uint32_t wpos;                   // next dword of w0 to take
    uint64_t buf; uint32_t cnt;      // uniform
    int64_t left;
    uint32_t lane;
    __device__ __forceinline__ uint32_t load(uint64_t base) const { const uint64_t i = base + lane; return i < n_words ? words[i] : 0u; }
    __device__ __forceinline__ void refill() {
        while (cnt <= 32) {
            const uint32_t d = __builtin_amdgcn_readlane(w0, qi_uni(wpos));
            buf |= (uint64_t)d << cnt; cnt += 32;
            if (++wpos == 64) { wpos = 0; w0 = w1; next += 64; w1 = load(next); }
        }
    }
    // byte `at` of the buffer becomes the next bit; `bytes_left` bytes of the block remain from there
    __device__ __forceinline__ void seek(uint64_t at, uint64_t bytes_left) {
        const uint64_t w = at >> 2;
        w0 = load(w); next = w + 64; w1 = load(next); wpos = 0; buf = 0; cnt = 0;
        left = (int64_t)(bytes_left * 8);
        refill();
        const uint32_t skip = (uint32_t)(at & 3) * 8;
        buf >>= skip; cnt -= skip;
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(uint32_t n) { buf >>= n; cnt -= n; left -= n; }
    __device__ __forceinline__ uint32_t get(uint32_t n) { refill(); const uint32_t v = peek(n); drop(n); return v; }   // n <= 16
};

// One canonical Huffman code: a primary table of `pbits` bits (entry = symbol << 4 | length, 0 = not here), the symbols sorted by
// (length, symbol) for the codes that are longer, and the count of every length (lane L holds count[L]).
// The wave builds it from lens[0 .. n): zlib's inflate_table rules -- an over-subscribed set is refused, an incomplete one too
// unless it is a literal/length or distance set whose longest code has one bit (zlib's one-code case); a set without any code is
// accepted and every attempt to decode with it fails.
__device__ __forceinline__ bool qi_build(const uint8_t* lens, uint32_t n, uint16_t* tab, uint32_t pbits, uint16_t* sorted, bool code_lengths,
                                         uint32_t lane, uint32_t& cntv) {
    for (uint32_t i = lane; i < (1u << pbits); i += 64) tab[i] = 0;
    cntv = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane, len = i < n ? lens[i] : 0u;
        for (uint32_t L = 1; L <= 15; L++) {
            const unsigned long long m = __ballot(len == L);
            if (lane == L) cntv += (uint32_t)__popcll(m);
        }
    }
    int32_t left = 1;
    uint32_t maxl = 0, code = 0, off = 0, nc = 0, po = 0;
    for (uint32_t L = 1; L <= 15; L++) {
        const uint32_t c = __builtin_amdgcn_readlane(cntv, L);
        left = (left << 1) - (int32_t)c;
        if (left < 0) return false;
        if (c) maxl = L;
        if (lane == L) { nc = code; po = off; }                  // the first code of length L, and where its symbols begin in sorted[]
        code = (code + c) << 1; off += c;
    }
    if (!maxl) return true;
    if (left > 0 && (code_lengths || maxl != 1)) return false;
    QI_WAVE_ORDER();                                             // the cleared table before its entries
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane, len = i < n ? lens[i] : 0u;
        uint32_t rank = 0, add = 0;
        for (uint32_t L = 1; L <= 15; L++) {
            const unsigned long long m = __ballot(len == L);
            if (len == L) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == L) add = (uint32_t)__popcll(m);
        }
        const uint32_t my_code = (uint32_t)__shfl((int)nc, (int)len) + rank, my_pos = (uint32_t)__shfl((int)po, (int)len) + rank;
        nc += add; po += add;
        if (len) {
            sorted[my_pos] = (uint16_t)i;                        // my_pos < n: the counts add up to at most n
            if (len <= pbits) {
                const uint32_t rev = __brev(my_code) >> (32 - len);
                for (uint32_t j = rev; j < (1u << pbits); j += 1u << len) tab[j] = (uint16_t)(i << 4 | len);
            }
        }
    }
    QI_WAVE_ORDER();
    return true;
}

// the next symbol of a code, or 0xFFFF when the bits are no code of it; B holds at least 15 bits (QiBits::refill)
__device__ __forceinline__ uint32_t qi_symbol(QiBits& B, const uint16_t* tab, uint32_t pbits, const uint16_t* sorted, uint32_t cntv) {
    const uint32_t e = qi_uni(tab[B.peek(pbits)]);
    if (e & 15) { B.drop(e & 15); return e >> 4; }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t L = 1; L <= 15; L++) {
        code |= (uint32_t)(B.buf >> (L - 1)) & 1u;
        const uint32_t c = __builtin_amdgcn_readlane(cntv, L);
        if (code < first + c) { B.drop(L); return qi_uni(sorted[index + (code - first)]); }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    B.drop(15);
    return 0xFFFFu;
}

// What differs between the two streams the decoder reads: a quality block is an RFC 1950 stream the way zlib's uncompress reads it
// (header, Adler-32, bytes behind the stream ignored, an empty destination given one byte of room); a BGZF member's payload is the
// bare RFC 1951 stream, which has to end with the payload's last byte and to give exactly ISIZE bytes.
struct QiZlib { static constexpr bool kZlib = true; };
struct QiRaw { static constexpr bool kZlib = false; };

// One deflate stream, decoded by one wave: block headers, tables, symbols, matches, stored blocks, the ring, its flush and the
// bookkeeping of `left`.  The stream is pay_size bytes at byte pay0 of the payload buffer; its text goes to out_text[0, size)
// (16-byte aligned).  Returns the status; `check` is the stream's own Adler-32 (QiZlib) or 0.
// Bounds: the payload is read through QiBits (inside the buffer, and `left` says when the stream's own bytes
// are used up) or, for a stored block, byte by byte below the stream's end; the text is written below out_text + size, size being the
// stream's share (a symbol that would pass it ends the stream with QI_LONG before it is written); a distance is checked against
// `out`, the bytes of THIS stream written so far, so that no match reads what another stream left in the ring; LDS indices are masked
// or checked against the tables' sizes.  Every turn of every loop consumes at least one bit of `left` or is counted by a bounded
// index, so the function returns on every input.
template <class P>
__device__ __forceinline__ uint32_t qi_stream(const uint32_t* __restrict__ pay, uint64_t pay_words, uint64_t pay0, uint64_t pay_size, uint64_t size,
                                              uint8_t* __restrict__ out_text, uint32_t lane, uint32_t& check, uint64_t& syms) {
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[QI_RING];
    __shared__ uint16_t s_lt[1u << QI_LBITS], s_dt[1u << QI_DBITS], s_ls[288], s_ds[32];
    __shared__ uint8_t s_lens[320], s_cl[19];
    const uint64_t limit = P::kZlib && !size ? 1 : size;         // (zlib's uncompress gives an empty destination one byte of room)
    const uint8_t* const pay_bytes = reinterpret_cast<const uint8_t*>(pay);
    QiBits B;
    B.words = pay; B.n_words = pay_words; B.lane = lane;
    B.seek(pay0, pay_size);
    uint32_t st = QI_OK;
    uint64_t out = 0, flushed = 0;
    uint32_t cnt_l = 0, cnt_d = 0;
    bool fixed_built = false;
    syms = 0;

    // RFC 1950: CMF, FLG
    if constexpr (P::kZlib) {
        const uint32_t cmf = B.get(8), flg = B.get(8);
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) st = QI_HEADER;
        if (B.left < 0) st = QI_EARLY;
    }
    uint32_t last = 0;
    while (st == QI_OK && !last) {
        last = B.get(1);
        const uint32_t type = B.get(2);
        if (B.left < 0) { st = QI_EARLY; break; }
        if (type == 3) { st = QI_TYPE; break; }
        if (type == 0) {
            // stored: to the byte boundary, LEN, NLEN, LEN bytes -- a plain wave-wide copy from the payload
            B.drop((uint32_t)(B.left & 7));
            const uint32_t len = B.get(16), nlen = B.get(16);
            if (B.left < 0) { st = QI_EARLY; break; }
            if ((len ^ 0xFFFFu) != nlen) { st = QI_STORED; break; }
            const uint64_t bytes_left = (uint64_t)B.left >> 3;
            if (len > bytes_left) { st = QI_EARLY; break; }
            if (out + len > limit) { st = QI_LONG; break; }
            const uint64_t src = pay0 + (pay_size - bytes_left);
            for (uint32_t done = 0; done < len;) {
                const uint32_t step = min(len - done, 256u);
                for (uint32_t k = lane; k < step; k += 64) s_ring[(out + k) & QI_RMASK] = pay_bytes[src + done + k];
                QI_WAVE_ORDER();
                done += step; out += step;
                while (size && out - flushed >= QI_FLUSH) {
                    *reinterpret_cast<uint4*>(out_text + flushed + 16u * lane) = *reinterpret_cast<const uint4*>(s_ring + (flushed & QI_RMASK) + 16u * lane);
                    flushed += QI_FLUSH;
                }
            }
            B.seek(src + len, bytes_left - len);
            continue;
        }
        if (type == 1) {
            if (!fixed_built) {
                for (uint32_t i = lane; i < 320; i += 64) s_lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
                QI_WAVE_ORDER();
                (void)qi_build(s_lens, 288, s_lt, QI_LBITS, s_ls, false, lane, cnt_l);
                (void)qi_build(s_lens + 288, 32, s_dt, QI_DBITS, s_ds, false, lane, cnt_d);
                fixed_built = true;
            }
        } else {
            fixed_built = false;
            const uint32_t nlen = B.get(5) + 257, ndist = B.get(5) + 1, ncode = B.get(4) + 4;
            if (B.left < 0) { st = QI_EARLY; break; }
            if (nlen > 286 || ndist > 30) { st = QI_TABLE; break; }
            if (lane < 19) s_cl[lane] = 0;
            QI_WAVE_ORDER();
            for (uint32_t i = 0; i < ncode; i++) {
                const uint32_t v = B.get(3);
                if (lane == 0) s_cl[kClOrder[i]] = (uint8_t)v;
            }
            if (B.left < 0) { st = QI_EARLY; break; }
            QI_WAVE_ORDER();
            uint32_t cnt_c;
            if (!qi_build(s_cl, 19, s_lt, 7, s_ls, true, lane, cnt_c)) { st = QI_TABLE; break; }
            const uint32_t total = nlen + ndist;
            uint32_t i = 0, prev = 0;
            while (i < total) {
                B.refill();
                const uint32_t sym = qi_symbol(B, s_lt, 7, s_ls, cnt_c);
                if (B.left < 0) { st = QI_EARLY; break; }
                if (sym < 16) { if (lane == 0) s_lens[i] = (uint8_t)sym; prev = sym; i++; continue; }
                if (sym > 18) { st = QI_TABLE; break; }
                uint32_t rep, v = 0;
                if (sym == 16) { if (!i) { st = QI_TABLE; break; } v = prev; rep = 3 + B.get(2); }
                else if (sym == 17) rep = 3 + B.get(3);
                else rep = 11 + B.get(7);
                if (B.left < 0) { st = QI_EARLY; break; }
                if (i + rep > total) { st = QI_TABLE; break; }
                for (uint32_t k = lane; k < rep; k += 64) s_lens[i + k] = (uint8_t)v;
                prev = v; i += rep;
            }
            if (st != QI_OK) break;
            QI_WAVE_ORDER();
            if (qi_uni(s_lens[256]) == 0) { st = QI_TABLE; break; }                      // no end-of-block code
            if (!qi_build(s_lens, nlen, s_lt, QI_LBITS, s_ls, false, lane, cnt_l)) { st = QI_TABLE; break; }
            if (!qi_build(s_lens + nlen, ndist, s_dt, QI_DBITS, s_ds, false, lane, cnt_d)) { st = QI_TABLE; break; }
        }
        // the block's symbols
        for (;;) {
            B.refill();
            const uint32_t sym = qi_symbol(B, s_lt, QI_LBITS, s_ls, cnt_l);
            syms++;
            if (B.left < 0) { st = QI_EARLY; break; }
            if (sym < 256) {
                if (out >= limit) { st = QI_LONG; break; }
                if (lane == 0) s_ring[out & QI_RMASK] = (uint8_t)sym;
                out++;
            } else if (sym == 256) {
                break;
            } else {
                if (sym > 285) { st = QI_CODE; break; }
                const uint32_t li = sym - 257;
                uint32_t len;
                if (li < 8) len = 3 + li;
                else if (li == 28) len = 258;
                else { const uint32_t e = (li >> 2) - 1; len = 3 + ((4 + (li & 3)) << e) + B.peek(e); B.drop(e); }
                B.refill();
                const uint32_t ds = qi_symbol(B, s_dt, QI_DBITS, s_ds, cnt_d);
                if (ds > 29) { st = B.left < 0 ? QI_EARLY : QI_CODE; break; }
                uint32_t dist;
                if (ds < 4) dist = 1 + ds;
                else { const uint32_t e = (ds >> 1) - 1; dist = 1 + ((2 + (ds & 1)) << e) + B.peek(e); B.drop(e); }
                if (B.left < 0) { st = QI_EARLY; break; }
                if (dist > out) { st = QI_DIST; break; }
                if (out + len > limit) { st = QI_LONG; break; }
                QI_WAVE_ORDER();
                const uint32_t o = (uint32_t)out & QI_RMASK;
                if (dist >= 64) {
                    // 64 bytes a turn: a turn's sources were written before it (by the text, or by the turns before)
                    for (uint32_t base = 0; base < len; base += 64) {
                        const uint32_t k = base + lane;
                        if (k < len) { const uint8_t v = s_ring[(o - dist + k) & QI_RMASK]; s_ring[(o + k) & QI_RMASK] = v; }
                        QI_WAVE_ORDER();
                    }
                } else if (dist == 1) {
                    const uint8_t v = s_ring[(o - 1) & QI_RMASK];
                    for (uint32_t k = lane; k < len; k += 64) s_ring[(o + k) & QI_RMASK] = v;
                } else {
                    // the pattern of `dist` bytes in front of the match, replicated: no lane reads what the match writes
                    for (uint32_t k = lane; k < len; k += 64) { const uint8_t v = s_ring[(o - dist + k % dist) & QI_RMASK]; s_ring[(o + k) & QI_RMASK] = v; }
                }
                out += len;
            }
            if (size && out - flushed >= QI_FLUSH) {
                QI_WAVE_ORDER();
                *reinterpret_cast<uint4*>(out_text + flushed + 16u * lane) = *reinterpret_cast<const uint4*>(s_ring + (flushed & QI_RMASK) + 16u * lane);
                flushed += QI_FLUSH;
            }
        }
    }
    uint32_t adler = 0;
    if (st == QI_OK) {
        B.drop((uint32_t)(B.left & 7));
        if constexpr (P::kZlib) {
            for (uint32_t i = 0; i < 4; i++) adler = adler << 8 | B.get(8);
            if (B.left < 0) st = QI_EARLY;
            else if (out != size) {
                // an empty share: uncompress accepts a stream of one byte (it goes nowhere) when its checksum holds
                const uint32_t d = qi_uni(s_ring[0]);
                if (size || out != 1 || adler != ((1 + d) << 16 | (1 + d))) st = QI_SHORT; else adler = 1;
            }
        } else {
            if (B.left != 0) st = QI_SLACK;                      // bytes between the stream's end and the trailer
            else if (out != size) st = QI_SHORT;
        }
    }
    QI_WAVE_ORDER();
    if (size) for (uint64_t k = flushed + lane; k < out; k += 64) out_text[k] = s_ring[k & QI_RMASK];       // out <= size
    check = adler;
    return st;
}

// One wave per quality block (an RFC 1950 stream).
__global__ __launch_bounds__(64) void k_qual_inflate(const uint32_t* __restrict__ pay, uint64_t pay_words, const QiBlock* __restrict__ blk,
                                                     uint32_t n_blocks, uint8_t* __restrict__ text, uint32_t* __restrict__ status,
                                                     uint32_t* __restrict__ adler_expect, unsigned long long* __restrict__ n_syms) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_blocks) return;
    const QiBlock K = blk[b];
    uint32_t adler; uint64_t syms;
    const uint32_t st = qi_stream<QiZlib>(pay, pay_words, K.pay0, K.pay_size, K.text_size, text + K.text0, lane, adler, syms);
    if (lane == 0) {
        status[b] = st; adler_expect[b] = adler;
        if (n_syms) atomicAdd(n_syms, (unsigned long long)syms);
    }
}

// One wave per BGZF member (leon_bgzf_inflate_device): the member's payload is a raw deflate stream of pay_size bytes
// that gives text_size (the trailer's ISIZE, at most 65 536) bytes, into the member's 16-byte aligned share of a temporary.  The
// members know nothing of one another: qi_stream starts every stream with an empty window.  Bounds: qi_stream's, with the share
// [text0, text0 + text_size) and the payload buffer of pay_words words; status is indexed below n_blocks.
__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint32_t* __restrict__ pay, uint64_t pay_words, const QiBlock* __restrict__ blk,
                                                     uint32_t n_blocks, uint8_t* __restrict__ text, uint32_t* __restrict__ status,
                                                     unsigned long long* __restrict__ n_syms) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_blocks) return;
    const QiBlock K = blk[b];
    uint32_t none; uint64_t syms;
    const uint32_t st = qi_stream<QiRaw>(pay, pay_words, K.pay0, K.pay_size, K.text_size, text + K.text0, lane, none, syms);
    if (lane == 0) {
        status[b] = st;
        if (n_syms) atomicAdd(n_syms, (unsigned long long)syms);
    }
}

constexpr uint32_t QT_THREADS = 256, QT_TILE = QT_THREADS * 16;

// the block a tile belongs to: blk[b].tile0 <= tile < blk[b + 1].tile0 (blk[n_blocks].tile0 = the tiles of the launch)
__device__ __forceinline__ uint32_t qi_block_of(const QiBlock* __restrict__ blk, uint32_t n_blocks, uint64_t tile) {
    uint32_t lo = 0, hi = n_blocks;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (blk[mid].tile0 <= tile) lo = mid; else hi = mid; }
    return lo;
}

__device__ __forceinline__ uint32_t qi_newlines(uint4 v, uint32_t valid) {      // bit j: byte j is a newline (j < valid)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) m |= (uint32_t)(((w[j >> 2] >> (8 * (j & 3))) & 255u) == '\n') << j;
    return valid >= 16 ? m : m & ((1u << valid) - 1u);
}

// sums over the workgroup's 256 threads, in thread 0
__device__ __forceinline__ void qi_block_sum3(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t* s_red /* 12 */) {
    for (int d = 32; d; d >>= 1) { a += __shfl_down(a, d); b += __shfl_down(b, d); c += __shfl_down(c, d); }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[w] = a; s_red[4 + w] = b; s_red[8 + w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) { a = s_red[0] + s_red[1] + s_red[2] + s_red[3]; b = s_red[4] + s_red[5] + s_red[6] + s_red[7]; c = s_red[8] + s_red[9] + s_red[10] + s_red[11]; }
}

// Bounds: a tile lies inside its block's share rounded up to 16 bytes (the shares are 16-byte aligned and the buffer is allocated
// to the rounded sum), tile_nl is indexed below n_tiles, sums below n_blocks.
__global__ __launch_bounds__(256) void k_qual_tiles(const QiBlock* __restrict__ blk, uint32_t n_blocks, uint64_t n_tiles, const uint8_t* __restrict__ text,
                                                    uint32_t* __restrict__ tile_nl, unsigned long long* __restrict__ sums /* 2 per block */,
                                                    uint32_t* __restrict__ last_nl) {
    __shared__ uint32_t s_red[12];
    const uint64_t tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const uint32_t b = qi_block_of(blk, n_blocks, tile);
    const uint64_t n = blk[b].text_size, at = (tile - blk[b].tile0) * QT_TILE + threadIdx.x * 16u;
    uint32_t nl = 0, s1 = 0, s2 = 0;
    if (at < n) {
        const uint32_t valid = (uint32_t)(n - at < 16 ? n - at : 16);
        const uint4 v = *reinterpret_cast<const uint4*>(text + blk[b].text0 + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t sj = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t d = j < valid ? (w[j >> 2] >> (8 * (j & 3))) & 255u : 0u;
            s1 += d; sj += j * d;
        }
        nl = __popc(qi_newlines(v, valid));
        // sum (n - at - j) d[j]  =  (n - at) s1 - sum j d[j],  mod 65521 (sj < 65521)
        s2 = (uint32_t)(((n - at) % ADLER_P * s1 + ADLER_P - sj) % ADLER_P);
        if (at + valid == n) last_nl[b] = ((w[(valid - 1) >> 2] >> (8 * ((valid - 1) & 3))) & 255u) == '\n';
    }
    qi_block_sum3(nl, s1, s2, s_red);
    if (threadIdx.x == 0) {
        tile_nl[tile] = nl;
        atomicAdd(&sums[2 * b], (unsigned long long)s1);
        atomicAdd(&sums[2 * b + 1], (unsigned long long)s2);
    }
}

__global__ __launch_bounds__(256) void k_qual_check(const QiBlock* __restrict__ blk, uint32_t n_blocks, const uint64_t* __restrict__ nl_before /* per tile, + 1 */,
                                                    const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ last_nl,
                                                    const uint32_t* __restrict__ adler_expect, uint32_t* __restrict__ status) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks || status[b] != QI_OK) return;
    const uint64_t n = blk[b].text_size;
    const uint64_t nl = nl_before[blk[b + 1].tile0] - nl_before[blk[b].tile0];
    const uint32_t a = (uint32_t)((1 + sums[2 * b]) % ADLER_P), s = (uint32_t)((n % ADLER_P + sums[2 * b + 1]) % ADLER_P);
    if (nl != blk[b].n_reads || (n && !last_nl[b])) status[b] = QI_LINES;
    else if ((s << 16 | a) != adler_expect[b]) status[b] = QI_ADLER;
}

// The text of a tile without its newlines, to its place in d_quals; launched only when every block of the launch has passed
// k_qual_check, so that a block's newlines are its reads and its other bytes are block_n_bytes.  The compacted bytes are staged in LDS
// at an index congruent to their address mod 16 and leave in aligned 16-byte stores (single bytes at the tile's two ends).
// Bounds (kept although the checks imply them): d_quals below quals_end, d_qual_off up to total_reads.
__global__ __launch_bounds__(256) void k_qual_lines(const QiBlock* __restrict__ blk, uint32_t n_blocks, uint64_t n_tiles, const uint8_t* __restrict__ text,
                                                    const uint64_t* __restrict__ nl_before, uint8_t* __restrict__ quals, uint64_t quals_end,
                                                    uint64_t* __restrict__ qual_off, uint64_t total_reads) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[QT_TILE + 16];
    __shared__ uint32_t s_wave[4];
    const uint64_t tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const uint32_t b = qi_block_of(blk, n_blocks, tile);
    const QiBlock K = blk[b];
    const uint64_t n = K.text_size, toff = (tile - K.tile0) * QT_TILE, at = toff + threadIdx.x * 16u;
    const uint64_t k_tile = nl_before[tile] - nl_before[K.tile0];          // newlines of the block in front of the tile
    const uint64_t o0 = K.q0 + toff - k_tile;                              // the tile's first byte in d_quals
    const uint32_t mis = (uint32_t)((uintptr_t)(quals + o0) & 15);
    uint32_t valid = 0, m = 0;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at < n) {
        valid = (uint32_t)(n - at < 16 ? n - at : 16);
        v = *reinterpret_cast<const uint4*>(text + K.text0 + at);
        m = qi_newlines(v, valid);
    }
    // newlines of the tile in front of this thread
    const uint32_t c = __popc(m), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = c;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d); if ((int)lane >= d) inc += t; }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t before = inc - c;
    for (uint32_t w = 0; w < wv; w++) before += s_wave[w];
    const uint32_t tile_nl = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const uint32_t tile_bytes = (uint32_t)(n - toff < QT_TILE ? n - toff : QT_TILE);
    const uint32_t cnt = tile_bytes - tile_nl;
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    uint32_t k = before;
    for (uint32_t j = 0; j < valid; j++) {
        const uint32_t x = threadIdx.x * 16u + j;                           // the byte's place in the tile
        if (m >> j & 1) {
            const uint64_t r = K.read0 + k_tile + k;                        // the read this newline ends
            if (qual_off && r < total_reads) qual_off[r + 1] = o0 + (x - k);
            k++;
        } else s_out[mis + x - k] = (uint8_t)(w4[j >> 2] >> (8 * (j & 3)));
    }
    __syncthreads();
    uint8_t* const g0 = quals + o0 - mis;                                   // 16-byte aligned
    for (uint32_t ch = threadIdx.x; ch * 16u < mis + cnt; ch += QT_THREADS) {
        const uint32_t lo = ch * 16u, hi = lo + 16;
        if (lo >= mis && hi <= mis + cnt && o0 + (hi - mis) <= quals_end) *reinterpret_cast<uint4*>(g0 + lo) = *reinterpret_cast<const uint4*>(s_out + lo);
        else for (uint32_t i = lo < mis ? mis : lo; i < hi && i < mis + cnt; i++) if (o0 + (i - mis) < quals_end) g0[i] = s_out[i];
    }
}

// A 4 KiB tile of a BGZF member's share to its place in the contiguous text (k_qual_lines without the newlines): the bytes are staged
// in LDS at an index congruent to their address mod 16 and leave in aligned 16-byte stores, single bytes at the tile's two ends -- two
// tiles that meet inside a 16-byte chunk each write their own bytes of it only.
// Bounds: the temporary is read inside the member's share rounded up to 16 bytes (the shares are 16-byte aligned and the buffer is
// allocated to the rounded sum); text is written at [q0 + toff, q0 + toff + the tile's bytes) and below text_end.
__global__ __launch_bounds__(256) void k_bgzf_gather(const QiBlock* __restrict__ blk, uint32_t n_blocks, uint64_t n_tiles, const uint8_t* __restrict__ tmp,
                                                     uint8_t* __restrict__ text, uint64_t text_end) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[QT_TILE + 16];
    const uint64_t tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const uint32_t b = qi_block_of(blk, n_blocks, tile);
    const QiBlock K = blk[b];
    const uint64_t n = K.text_size, toff = (tile - K.tile0) * QT_TILE, at = toff + threadIdx.x * 16u;
    if (toff >= n) return;                                                  // (uniform; no tile of the table is empty)
    const uint64_t o0 = K.q0 + toff;                                        // the tile's first byte in the text
    const uint32_t mis = (uint32_t)((uintptr_t)(text + o0) & 15);
    if (at < n) {
        const uint32_t valid = (uint32_t)(n - at < 16 ? n - at : 16);
        const uint4 v = *reinterpret_cast<const uint4*>(tmp + K.text0 + at);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t j = 0; j < valid; j++) s_out[mis + threadIdx.x * 16u + j] = (uint8_t)(w4[j >> 2] >> (8 * (j & 3)));
    }
    __syncthreads();
    const uint32_t cnt = (uint32_t)(n - toff < QT_TILE ? n - toff : QT_TILE);
    uint8_t* const g0 = text + o0 - mis;                                    // 16-byte aligned
    for (uint32_t ch = threadIdx.x; ch * 16u < mis + cnt; ch += QT_THREADS) {
        const uint32_t lo = ch * 16u, hi = lo + 16;
        if (lo >= mis && hi <= mis + cnt && o0 + (hi - mis) <= text_end) *reinterpret_cast<uint4*>(g0 + lo) = *reinterpret_cast<const uint4*>(s_out + lo);
        else for (uint32_t i = lo < mis ? mis : lo; i < hi && i < mis + cnt; i++) if (o0 + (i - mis) < text_end) g0[i] = s_out[i];
    }
}

__global__ __launch_bounds__(256) void k_qual_lens(const uint64_t* __restrict__ qual_off, const uint32_t* __restrict__ len, uint64_t read0, uint64_t n,
                                                   unsigned long long* __restrict__ bad_read /* ~0 */) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r < n && qual_off[read0 + r + 1] - qual_off[read0 + r] != len[read0 + r]) atomicMin(bad_read, (unsigned long long)(read0 + r));
}

// one wave per block; status[b] = QI_OK or why the stream was refused, adler_expect[b] = the stream's own checksum; n_syms: nullptr,
// or a counter of the literal/length symbols decoded (measurement)
void launch_qual_inflate(hipStream_t s, const uint32_t* pay, uint64_t pay_words, const QiBlock* blk, uint32_t n_blocks, uint8_t* text, uint32_t* status,
                         uint32_t* adler_expect, unsigned long long* n_syms) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_qual_inflate, dim3(n_blocks), dim3(64), 0, s, pay, pay_words, blk, n_blocks, text, status, adler_expect, n_syms);
}

// one wave per member, the decoder of launch_qual_inflate on a raw stream that ends with its payload; status[b] = QI_OK or why
void launch_bgzf_inflate(hipStream_t s, const uint32_t* pay, uint64_t pay_words, const QiBlock* blk, uint32_t n_blocks, uint8_t* tmp, uint32_t* status,
                         unsigned long long* n_syms) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(n_blocks), dim3(64), 0, s, pay, pay_words, blk, n_blocks, tmp, status, n_syms);
}

// the shares of the temporary to text[q0 ..), contiguous, whatever text's alignment; nothing at or behind text_end is written
void launch_bgzf_gather(hipStream_t s, const QiBlock* blk, uint32_t n_blocks, uint64_t n_tiles, const uint8_t* tmp, uint8_t* text, uint64_t text_end) {
    if (!n_tiles) return;
    hipLaunchKernelGGL(k_bgzf_gather, dim3((uint32_t)n_tiles), dim3(QT_THREADS), 0, s, blk, n_blocks, n_tiles, tmp, text, text_end);
}

// per 4 KiB tile of the text: its newlines (tile_nl: n_tiles + 1, the last 0); per block (zeroed by the caller): the two Adler-32 sums,
// whether the last byte is a newline
void launch_qual_tiles(hipStream_t s, const QiBlock* blk, uint32_t n_blocks, uint64_t n_tiles, const uint8_t* text, uint32_t* tile_nl,
                       unsigned long long* sums, uint32_t* last_nl) {
    if (!n_tiles) return;
    hipLaunchKernelGGL(k_qual_tiles, dim3((uint32_t)n_tiles), dim3(QT_THREADS), 0, s, blk, n_blocks, n_tiles, text, tile_nl, sums, last_nl);
}

// exclusive, n_tiles + 1 entries
hipError_t qual_tiles_scan(void* tmp, size_t& bytes, const uint32_t* tile_nl, uint64_t* nl_before, uint64_t n_tiles, hipStream_t s) {
    return prim::ExclusiveSum(tmp, bytes, tile_nl, nl_before, n_tiles + 1, s);
}

void launch_qual_check(hipStream_t s, const QiBlock* blk, uint32_t n_blocks, const uint64_t* nl_before, const unsigned long long* sums,
                       const uint32_t* last_nl, const uint32_t* adler_expect, uint32_t* status) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_qual_check, dim3((n_blocks + 255) / 256), dim3(256), 0, s, blk, n_blocks, nl_before, sums, last_nl, adler_expect, status);
}

// the text without its newlines and the reads' offsets; only after every status of the launch is QI_OK
void launch_qual_lines(hipStream_t s, const QiBlock* blk, uint32_t n_blocks, uint64_t n_tiles, const uint8_t* text, const uint64_t* nl_before,
                       uint8_t* quals, uint64_t quals_end, uint64_t* qual_off, uint64_t total_reads) {
    if (!n_tiles) return;
    hipLaunchKernelGGL(k_qual_lines, dim3((uint32_t)n_tiles), dim3(QT_THREADS), 0, s, blk, n_blocks, n_tiles, text, nl_before, quals, quals_end, qual_off, total_reads);
}

void launch_qual_lens(hipStream_t s, const uint64_t* qual_off, const uint32_t* len, uint64_t read0, uint64_t n, unsigned long long* bad_read) {
    if (!n) return;
    hipLaunchKernelGGL(k_qual_lens, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, qual_off, len, read0, n, bad_read);
}

}  // namespace
}  // namespace leon

using namespace leon;

extern "C" int leon_qual_inflate_blocks_device(int device_id, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                                    const uint64_t* block_n_bytes, uint64_t n_blocks, const uint32_t* d_len, uint8_t* d_quals, uint64_t quals_cap,
                                    uint64_t* d_qual_off, uint64_t* n_symbols) {
    if (n_symbols) *n_symbols = 0;
    if (n_blocks && (!payloads || !payload_off || !block_n_reads || !block_n_bytes || !d_quals)) return dev_fail(LEON_E_INVALID, "null argument");
    if (!n_blocks) return LEON_OK;
    if (n_blocks > (1ull << 31)) return dev_fail(LEON_E_INVALID, "implausible number of blocks");
    std::vector<uint64_t> o0(n_blocks + 1, 0), r0(n_blocks + 1, 0);
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (payload_off[b + 1] < payload_off[b]) return dev_fail(LEON_E_INVALID, "payload offsets are not monotonic");
        o0[b + 1] = o0[b] + block_n_bytes[b];
        r0[b + 1] = r0[b] + block_n_reads[b];
        if (o0[b + 1] < o0[b] || o0[b + 1] > quals_cap) return dev_fail(LEON_E_INVALID, "output capacity below the sum of block_n_bytes");
    }
    const uint64_t total_reads = r0[n_blocks];
    CallStream st;
    if (const int rc = dev_open("leon_qual_inflate_blocks_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    // The blocks in launches of at most kMaxBlocks blocks and kMaxText bytes of temporary text (the lines WITH their newlines, every
    // block's share 16-byte aligned): what bounds the temporaries; a launch holds at least one block.
    constexpr uint64_t kMaxBlocks = 1024, kMaxText = 8ull << 30;
    auto share = [&](uint64_t b) { return (block_n_bytes[b] + block_n_reads[b] + 15) & ~15ull; };
    std::vector<uint64_t> cut{0};
    uint64_t max_text = 0, max_pay = 0, max_tiles = 0, max_blocks = 0;
    for (uint64_t b = 0; b < n_blocks;) {
        uint64_t e = b, text = 0, tiles = 0;
        while (e < n_blocks && (e == b || (e - b < kMaxBlocks && text + share(e) <= kMaxText))) {
            text += share(e); tiles += (block_n_bytes[e] + block_n_reads[e] + 4095) / 4096; e++;
        }
        max_text = std::max(max_text, text); max_tiles = std::max(max_tiles, tiles); max_blocks = std::max(max_blocks, e - b);
        max_pay = std::max(max_pay, payload_off[e] - payload_off[b]);
        cut.push_back(e); b = e;
    }
    if (max_tiles >= (1ull << 31)) return dev_fail(LEON_E_INVALID, "implausible block sizes");
    OwnBuf d_pay, d_text, d_blk, d_status, d_adler, d_tile_nl, d_nl_before, d_sums, d_last, d_tmp, d_cnt, d_off_own;
    DEVCHK(d_pay.ensure(max_pay + 64)); DEVCHK(d_text.ensure(max_text + 64));
    DEVCHK(d_blk.ensure((max_blocks + 1) * sizeof(QiBlock)));
    DEVCHK(d_status.ensure(max_blocks * 4)); DEVCHK(d_adler.ensure(max_blocks * 4)); DEVCHK(d_last.ensure(max_blocks * 4));
    DEVCHK(d_sums.ensure(max_blocks * 16));
    DEVCHK(d_tile_nl.ensure((max_tiles + 1) * 4)); DEVCHK(d_nl_before.ensure((max_tiles + 1) * 8));
    DEVCHK(d_cnt.ensure(16));
    DEVCHK(hipMemsetAsync(d_cnt.p, 0, 8, s));
    DEVCHK(hipMemsetAsync(d_cnt.as<uint8_t>() + 8, 0xFF, 8, s));
    size_t tmp_bytes = 0;
    DEVCHK(qual_tiles_scan(nullptr, tmp_bytes, d_tile_nl.as<uint32_t>(), d_nl_before.as<uint64_t>(), max_tiles, s));
    DEVCHK(d_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    uint64_t* qual_off = d_qual_off;
    if (!qual_off && d_len) { DEVCHK(d_off_own.ensure((total_reads + 1) * 8)); qual_off = d_off_own.as<uint64_t>(); }   // the lengths are checked through the offsets
    if (qual_off) DEVCHK(hipMemsetAsync(qual_off, 0, 8, s));
    std::vector<QiBlock> blk;
    std::vector<uint32_t> status;
    for (size_t g = 0; g + 1 < cut.size(); g++) {
        const uint64_t b0 = cut[g], b1 = cut[g + 1], nb = b1 - b0, pay_bytes = payload_off[b1] - payload_off[b0];
        blk.assign(nb + 1, QiBlock{});
        uint64_t text = 0, tiles = 0;
        for (uint64_t b = b0; b <= b1; b++) {
            QiBlock& K = blk[b - b0];
            K.text0 = text; K.tile0 = tiles;
            if (b == b1) break;
            K.pay0 = payload_off[b] - payload_off[b0]; K.pay_size = payload_off[b + 1] - payload_off[b];
            K.text_size = block_n_bytes[b] + block_n_reads[b];
            K.q0 = o0[b]; K.read0 = r0[b]; K.n_reads = block_n_reads[b];
            text += share(b); tiles += (K.text_size + 4095) / 4096;
        }
        if (staged_h2d(device_id, d_pay.p, payloads + payload_off[b0], pay_bytes) != hipSuccess) { (void)hipGetLastError(); return dev_fail(LEON_E_HIP, "leon_qual_inflate_blocks_device: the payloads' copy to the device failed"); }
        DEVCHK(hipMemcpyAsync(d_blk.p, blk.data(), (nb + 1) * sizeof(QiBlock), hipMemcpyHostToDevice, s));
        DEVCHK(hipMemsetAsync(d_sums.p, 0, nb * 16, s));
        DEVCHK(hipMemsetAsync(d_last.p, 0, nb * 4, s));
        DEVCHK(hipMemsetAsync(d_tile_nl.as<uint32_t>() + tiles, 0, 4, s));
        launch_qual_inflate(s, d_pay.as<uint32_t>(), (pay_bytes + 3) / 4, d_blk.as<QiBlock>(), (uint32_t)nb, d_text.as<uint8_t>(), d_status.as<uint32_t>(),
                            d_adler.as<uint32_t>(), n_symbols ? d_cnt.as<unsigned long long>() : nullptr);
        DEVCHK(hipGetLastError());
        launch_qual_tiles(s, d_blk.as<QiBlock>(), (uint32_t)nb, tiles, d_text.as<uint8_t>(), d_tile_nl.as<uint32_t>(), d_sums.as<unsigned long long>(), d_last.as<uint32_t>());
        DEVCHK(hipGetLastError());
        DEVCHK(qual_tiles_scan(d_tmp.p, tmp_bytes, d_tile_nl.as<uint32_t>(), d_nl_before.as<uint64_t>(), tiles, s));
        launch_qual_check(s, d_blk.as<QiBlock>(), (uint32_t)nb, d_nl_before.as<uint64_t>(), d_sums.as<unsigned long long>(), d_last.as<uint32_t>(),
                          d_adler.as<uint32_t>(), d_status.as<uint32_t>());
        DEVCHK(hipGetLastError());
        // the blocks' status words in one small copy; the smallest failing block is the one the host way names
        status.assign(nb, 0);
        DEVCHK(hipMemcpyAsync(status.data(), d_status.p, nb * 4, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
        for (uint64_t b = 0; b < nb; b++)
            if (status[b] != QI_OK) return dev_fail(LEON_E_INVALID, "quality block " + std::to_string(b0 + b) + " does not decode");
        launch_qual_lines(s, d_blk.as<QiBlock>(), (uint32_t)nb, tiles, d_text.as<uint8_t>(), d_nl_before.as<uint64_t>(), d_quals, o0[n_blocks], qual_off, total_reads);
        DEVCHK(hipGetLastError());
        DEVCHK(hipStreamSynchronize(s));                 // the next launch reuses the temporaries (and the host's blk)
    }
    uint64_t words[2] = {0, ~0ull};
    if (d_len) { launch_qual_lens(s, qual_off, d_len, 0, total_reads, d_cnt.as<unsigned long long>() + 1); DEVCHK(hipGetLastError()); }
    DEVCHK(hipMemcpyAsync(words, d_cnt.p, 16, hipMemcpyDeviceToHost, s));
    DEVCHK(hipStreamSynchronize(s));
    if (n_symbols) *n_symbols = words[0];
    if (words[1] != ~0ull) {
        const uint64_t b = (uint64_t)(std::upper_bound(r0.begin(), r0.end(), words[1]) - r0.begin()) - 1;
        return dev_fail(LEON_E_INVALID, "read " + std::to_string(words[1]) + " (quality block " + std::to_string(b) + "): the quality line's length is not the one given (d_len)");
    }
    return LEON_OK;
}

extern "C" int leon_bgzf_inflate_device(int device_id, const uint8_t* bytes, uint64_t n_bytes, const uint64_t* member_off, uint64_t n_members, uint8_t* d_text,
                             uint64_t text_cap, uint64_t* n_text, uint32_t max_members_per_launch, uint64_t* n_symbols) {
    if (n_symbols) *n_symbols = 0;
    std::vector<BgzfMember> m;
    {
        std::string why;
        if (const int rc = bgzf_prepare(bytes, n_bytes, member_off, n_members, d_text, text_cap, n_text, m, why)) return dev_fail(rc, why);
    }
    if (!n_members) return LEON_OK;
    CallStream st;
    if (const int rc = dev_open("leon_bgzf_inflate_device", device_id, st)) return rc;
    hipStream_t s = st.s;
    // launches of at most `per` members: what bounds the temporaries (a member has at most 64 KiB of payload and of text)
    const uint64_t per = max_members_per_launch ? max_members_per_launch : 4096;
    auto share = [&](uint64_t i) { return ((uint64_t)m[i].isize + 15) & ~15ull; };
    uint64_t max_pay = 0, max_tmp = 0, max_nb = 0;
    for (uint64_t b0 = 0; b0 < n_members; b0 += per) {
        const uint64_t b1 = std::min(n_members, b0 + per);
        uint64_t tmp = 0;
        for (uint64_t i = b0; i < b1; i++) tmp += share(i);
        max_pay = std::max(max_pay, member_off[b1] - member_off[b0]); max_tmp = std::max(max_tmp, tmp); max_nb = std::max(max_nb, b1 - b0);
    }
    OwnBuf d_pay, d_tmp, d_blk, d_status, d_seg, d_acc, d_cnt;
    DEVCHK(d_pay.ensure(max_pay + 64)); DEVCHK(d_tmp.ensure(max_tmp + 64));
    DEVCHK(d_blk.ensure((max_nb + 1) * sizeof(QiBlock)));
    DEVCHK(d_status.ensure(max_nb * 4)); DEVCHK(d_seg.ensure((2 * max_nb + 1) * 8)); DEVCHK(d_acc.ensure(2 * max_nb * 4));
    DEVCHK(d_cnt.ensure(8));
    DEVCHK(hipMemsetAsync(d_cnt.p, 0, 8, s));
    std::vector<QiBlock> blk;
    std::vector<uint64_t> seg;
    std::vector<uint32_t> status, acc;
    for (uint64_t b0 = 0; b0 < n_members; b0 += per) {
        const uint64_t b1 = std::min(n_members, b0 + per), nb = b1 - b0, pay_bytes = member_off[b1] - member_off[b0];
        blk.assign(nb + 1, QiBlock{}); seg.assign(2 * nb + 1, 0);
        uint64_t tmp = 0, tiles = 0;
        for (uint64_t i = b0; i <= b1; i++) {
            QiBlock& K = blk[i - b0];
            K.text0 = tmp; K.tile0 = tiles;
            seg[2 * (i - b0)] = tmp;                              // the member's text, then the share's padding: two segments
            if (i == b1) break;
            if (m[i].ok) { K.pay0 = m[i].pay0 - member_off[b0]; K.pay_size = m[i].pay_size; K.text_size = m[i].isize; }   // (!ok: an empty stream, refused below)
            K.q0 = m[i].text0;
            seg[2 * (i - b0) + 1] = tmp + K.text_size;
            tmp += share(i); tiles += (K.text_size + 4095) / 4096;
        }
        if (staged_h2d(device_id, d_pay.p, bytes + member_off[b0], pay_bytes) != hipSuccess) { (void)hipGetLastError(); return dev_fail(LEON_E_HIP, "leon_bgzf_inflate_device: the payloads' copy to the device failed"); }
        DEVCHK(hipMemcpyAsync(d_blk.p, blk.data(), (nb + 1) * sizeof(QiBlock), hipMemcpyHostToDevice, s));
        DEVCHK(hipMemcpyAsync(d_seg.p, seg.data(), (2 * nb + 1) * 8, hipMemcpyHostToDevice, s));
        DEVCHK(hipMemsetAsync(d_acc.p, 0, 2 * nb * 4, s));
        launch_bgzf_inflate(s, d_pay.as<uint32_t>(), (pay_bytes + 3) / 4, d_blk.as<QiBlock>(), (uint32_t)nb, d_tmp.as<uint8_t>(), d_status.as<uint32_t>(),
                            n_symbols ? d_cnt.as<unsigned long long>() : nullptr);
        DEVCHK(hipGetLastError());
        // the CRC-32 of every member's text where the wave left it, before anything goes to d_text
        launch_crc32_segments(s, d_tmp.as<uint8_t>(), d_seg.as<uint64_t>(), 2 * nb, crc32_tile_count(d_tmp.as<uint8_t>(), 0, tmp), d_acc.as<uint32_t>());
        DEVCHK(hipGetLastError());
        status.assign(nb, 0); acc.assign(2 * nb, 0);
        DEVCHK(hipMemcpyAsync(status.data(), d_status.p, nb * 4, hipMemcpyDeviceToHost, s));
        DEVCHK(hipMemcpyAsync(acc.data(), d_acc.p, 2 * nb * 4, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < nb; i++)
            if (!m[b0 + i].ok || status[i] != QI_OK || acc[2 * i] != m[b0 + i].crc) return dev_fail(LEON_E_INVALID, bgzf_refusal(b0 + i, member_off[b0 + i]));
        launch_bgzf_gather(s, d_blk.as<QiBlock>(), (uint32_t)nb, tiles, d_tmp.as<uint8_t>(), d_text, *n_text);
        DEVCHK(hipGetLastError());
        DEVCHK(hipStreamSynchronize(s));                 // the next launch reuses the temporaries (and the host's tables)
    }
    if (n_symbols) {
        DEVCHK(hipMemcpyAsync(n_symbols, d_cnt.p, 8, hipMemcpyDeviceToHost, s));
        DEVCHK(hipStreamSynchronize(s));
    }
    return LEON_OK;
}
