// bgzf_fuzz_check.cpp -- a stand-alone program for AddressSanitizer / UBSan (tests/test_bgzf_input_cpu.py compiles it together with
// leon_amd/csrc/host_streams.cpp): leon_host_bgzf_members and leon_host_bgzf_inflate on a fixed-seed set of damaged BGZF streams --
// flipped bytes, cut tails, BSIZE / XLEN / ISIZE that lie, member tables that lie.  Nothing may be read or written outside the
// buffers given (they are allocated to their exact sizes, so that the sanitizer sees the first byte beyond); the undamaged streams
// must decode to their text.  Prints "bgzf fuzz: ok" and exits 0.
#include "../include/leon_dna.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace leon { thread_local std::string g_error; void set_create_error(const std::string& m) { g_error = m; } }
extern "C" const char* leon_last_error(const leon_dna_ctx*) { return leon::g_error.c_str(); }

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

void put16(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
void put32(std::vector<uint8_t>& v, uint32_t x) { put16(v, x & 0xFFFF); put16(v, x >> 16); }

void append_member(std::vector<uint8_t>& out, const std::vector<uint8_t>& text, int level, bool extra) {
    z_stream z{};
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    std::vector<uint8_t> pay(deflateBound(&z, (uLong)text.size()) + 16);
    z.next_in = const_cast<Bytef*>(text.data()); z.avail_in = (uInt)text.size();
    z.next_out = pay.data(); z.avail_out = (uInt)pay.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    pay.resize(z.total_out);
    deflateEnd(&z);
    const uint8_t head[10] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff};
    out.insert(out.end(), head, head + 10);
    const uint32_t xlen = extra ? 6 + 7 : 6;
    put16(out, xlen);
    if (extra) { const uint8_t sub[7] = {'X', 'Y', 3, 0, 1, 2, 3}; out.insert(out.end(), sub, sub + 7); }
    const uint8_t bc[4] = {'B', 'C', 2, 0};
    out.insert(out.end(), bc, bc + 4);
    put16(out, (uint32_t)(12 + xlen + pay.size() + 8 - 1));
    out.insert(out.end(), pay.begin(), pay.end());
    put32(out, (uint32_t)crc32(crc32(0L, Z_NULL, 0), text.data(), (uInt)text.size()));
    put32(out, (uint32_t)text.size());
}

// the walk and the inflate over exactly these bytes; returns the text when everything was accepted
bool run(const std::vector<uint8_t>& exact, int last, std::vector<uint8_t>* text_out) {
    std::vector<uint8_t> bytes(exact);                            // (its own allocation of the exact size)
    uint64_t n_members = 0, n_text = 0, consumed = 0;
    uint32_t stop = 0;
    std::vector<uint64_t> off(bytes.size() / 20 + 2);
    int rc = leon_host_bgzf_members(bytes.data(), bytes.size(), last, off.data(), off.size(), &n_members, &n_text, &consumed, &stop);
    if (rc == LEON_E_OVERFLOW) abort();                           // (a member has at least 20 bytes)
    if (consumed > bytes.size() || n_members + 1 > off.size() || off[n_members] != consumed || n_text > 65536 * n_members) abort();
    if ((rc == LEON_OK) != (stop == LEON_BGZF_WHOLE || stop == LEON_BGZF_PARTIAL)) abort();
    // a table with too few entries is refused, not overrun
    if (n_members) {
        std::vector<uint64_t> few(n_members);
        uint64_t a, b, c; uint32_t d;
        if (leon_host_bgzf_members(bytes.data(), bytes.size(), last, few.data(), few.size(), &a, &b, &c, &d) != LEON_E_OVERFLOW || a != n_members) abort();
    }
    std::vector<uint8_t> text(n_text);
    uint64_t got = 0;
    rc = leon_host_bgzf_inflate(bytes.data(), consumed, off.data(), n_members, text.data(), text.size(), &got, 1 + (uint32_t)(rnd() % 3));
    if (rc == LEON_OK && got != n_text) abort();
    if (n_text) {                                                 // one byte too little room: refused with the bytes needed, nothing decoded
        std::vector<uint8_t> small(n_text - 1);
        uint64_t need = 0;
        if (leon_host_bgzf_inflate(bytes.data(), consumed, off.data(), n_members, small.data(), small.size(), &need, 1) != LEON_E_OVERFLOW || need != n_text) abort();
    }
    if (rc == LEON_OK && text_out) *text_out = text;
    return rc == LEON_OK && stop == LEON_BGZF_WHOLE;
}

}  // namespace

int main() {
    uint64_t accepted = 0, refused = 0;
    for (int round = 0; round < 40; round++) {
        // a stream of a few members of FASTQ-like text
        std::vector<uint8_t> text, stream;
        const int n_members = 1 + (int)(rnd() % 5);
        std::vector<size_t> starts;
        for (int m = 0; m < n_members; m++) {
            const size_t n = (rnd() % 4 == 0) ? 0 : (size_t)(rnd() % (m == 0 ? 65536 : 9000));
            std::vector<uint8_t> part(n);
            for (size_t i = 0; i < n; i++) part[i] = (uint8_t)("ACGTN\nIIIIF#@+"[(rnd() >> 9) % 14]);
            starts.push_back(stream.size());
            append_member(stream, part, (int)(rnd() % 10), rnd() % 3 == 0);
            text.insert(text.end(), part.begin(), part.end());
        }
        std::vector<uint8_t> got;
        if (!run(stream, 1, &got) || got != text) { fprintf(stderr, "round %d: the undamaged stream does not decode to its text\n", round); return 1; }
        accepted++;
        for (int k = 0; k < 60; k++) {
            std::vector<uint8_t> bad(stream);
            const size_t at = starts[rnd() % starts.size()];
            switch (rnd() % 7) {
            case 0: for (int f = 1 + (int)(rnd() % 3); f > 0; f--) bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;   // flipped bits
            case 1: bad.resize(rnd() % bad.size()); break;                                                                        // a cut tail
            case 2: bad[at + 10] = (uint8_t)rnd(); bad[at + 11] = (uint8_t)(rnd() % 4 ? 0 : rnd()); break;                        // XLEN lies
            case 3: { size_t p = at + 16; if (bad[at + 12] == 'X') p += 7; bad[p] = (uint8_t)rnd(); bad[p + 1] = (uint8_t)rnd(); } break;   // BSIZE lies
            case 4: { const size_t end = bad.size(); bad[end - 4 + rnd() % 4] = (uint8_t)rnd(); } break;                          // ISIZE lies
            case 5: bad.insert(bad.begin() + (ptrdiff_t)(rnd() % (bad.size() + 1)), (uint8_t)rnd()); break;                         // a byte too many
            default: bad.erase(bad.begin() + (ptrdiff_t)(rnd() % bad.size())); break;                                              // a byte too few
            }
            if (bad.empty()) continue;
            std::vector<uint8_t> t;
            if (run(bad, (int)(rnd() % 2), &t)) {                  // a flip in a field nothing reads (MTIME, XFL, OS, another subfield), or a cut between two members
                if (t.size() > text.size() || (!t.empty() && memcmp(t.data(), text.data(), t.size()) != 0)) return 2;
                accepted++;
            }
            else refused++;
        }
        // a member table that lies: offsets inside members, a last offset one short
        {
            uint64_t n = 0, nt = 0, used = 0; uint32_t stop = 0;
            std::vector<uint64_t> off(stream.size() / 20 + 2);
            if (leon_host_bgzf_members(stream.data(), stream.size(), 1, off.data(), off.size(), &n, &nt, &used, &stop) != LEON_OK) return 3;
            std::vector<uint8_t> out(nt + 1);
            for (int k = 0; k < 20; k++) {
                std::vector<uint64_t> lie(off.begin(), off.begin() + (ptrdiff_t)n + 1);
                const size_t i = rnd() % lie.size();
                lie[i] = (rnd() % 2) ? lie[i] - (lie[i] ? 1 : 0) : rnd() % (stream.size() + 40);
                uint64_t g = 0;
                std::vector<uint8_t> bytes(stream);
                (void)leon_host_bgzf_inflate(bytes.data(), bytes.size(), lie.data(), n, out.data(), nt, &g, 2);
                if (g > 65536 * n) return 4;
            }
        }
    }
    if (!refused) { fprintf(stderr, "no damaged stream was refused\n"); return 5; }
    printf("bgzf fuzz: ok (%llu accepted, %llu refused)\n", (unsigned long long)accepted, (unsigned long long)refused);
    return 0;
}
