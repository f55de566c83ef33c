// bam_records_check.cpp -- leon_host_records_bam and leon_bam_header in a program of their own, for the sanitizers
// (tests/test_bam_records_cpu.py builds it with host_streams.cpp and -fsanitize=address,undefined).  Every buffer is a heap block of
// exactly the bytes the contract names, so a read or write one byte past any of them is reported.  The bytes themselves are judged by
// tests/bam_records.py in the Python tests; here the records only have to tile the output (block_size by block_size).
#include "leon_dna.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

// (what capi.hip gives the library: the message behind leon_last_error(NULL))
namespace leon { thread_local std::string g_error; void set_create_error(const std::string& m) { g_error = m; } }
extern "C" const char* leon_last_error(const leon_dna_ctx*) { return leon::g_error.c_str(); }

namespace {

int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, leon_last_error(nullptr)); failures++; } } while (0)

template <typename T> std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // (an empty vector's block is still a block: never NULL)
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

struct Call {
    std::vector<uint8_t> bases, quals, hdr;
    std::vector<uint32_t> len;
    std::vector<uint64_t> hdr_off;
    leon_record_layout lay;
};

Call draw(std::mt19937_64& rng, uint32_t n, bool with_hdr, uint64_t first) {
    Call c;
    memset(&c.lay, 0, sizeof c.lay);
    c.lay.struct_size = sizeof c.lay; c.lay.fastq = 1; c.lay.lead = '@'; c.lay.first_read_index = first;
    const uint32_t lens[] = {0, 1, 2, 15, 16, 17, 33, 149, 150, 1001};
    const char* const alphabet = "ACGTNacgtnRY.-*=";
    c.hdr_off.push_back(77);                                     // offsets count from a set's first byte
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t l = lens[rng() % 10];
        c.len.push_back(l);
        for (uint32_t i = 0; i < l; i++) { c.bases.push_back((uint8_t)alphabet[rng() % 16]); c.quals.push_back((uint8_t)(33 + rng() % 94)); }
        if (with_hdr) {
            const uint32_t hl = (uint32_t)(rng() % 5 == 0 ? rng() % 3 : rng() % 5 == 1 ? 254 : 10 + rng() % 50);
            for (uint32_t i = 0; i < hl; i++) c.hdr.push_back(hl != 254 && rng() % 12 == 0 ? (rng() & 1 ? ' ' : '\t') : (uint8_t)('A' + rng() % 26));
            c.hdr_off.push_back(77 + c.hdr.size());
        }
    }
    c.lay.hdr_bytes = c.hdr.size();
    return c;
}

// the call on exact blocks; returns its status, *size as the call left it; on success the records must tile the output
int run(const Call& c, bool with_hdr, bool with_quals, uint64_t cap_delta, uint32_t n_threads, uint64_t* size, const std::vector<uint64_t>* bad_off = nullptr,
        const uint64_t* n_bases_told = nullptr) {
    const uint64_t n = c.len.size();
    auto bases = exact(c.bases), quals = exact(c.quals), hdr = exact(c.hdr);
    auto len = exact(c.len);
    auto off = exact(bad_off ? *bad_off : c.hdr_off);
    uint64_t need = 0;
    const uint64_t n_bases = n_bases_told ? *n_bases_told : c.bases.size();
    int rc = leon_host_records_bam(&c.lay, bases.get(), len.get(), n, n_bases, with_hdr ? hdr.get() : nullptr, with_hdr ? off.get() : nullptr,
                                   with_quals ? quals.get() : nullptr, nullptr, 0, nullptr, &need, n_threads);
    *size = need;
    if (rc != LEON_E_OVERFLOW) return rc;                        // (no read: LEON_OK with size 0; or a refusal)
    const uint64_t cap = need + cap_delta;                        // cap_delta = -1 as an unsigned wrap: a byte short
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap ? cap : 1]);
    std::unique_ptr<uint64_t[]> rec(new uint64_t[n + 1]);
    rc = leon_host_records_bam(&c.lay, bases.get(), len.get(), n, n_bases, with_hdr ? hdr.get() : nullptr, with_hdr ? off.get() : nullptr,
                               with_quals ? quals.get() : nullptr, out.get(), cap, rec.get(), size, n_threads);
    if (rc == LEON_OK) {
        EXPECT(*size == need && rec[0] == 0 && rec[n] == need);
        uint64_t at = 0;
        for (uint64_t r = 0; r < n && at + 4 <= need; r++) {
            EXPECT(rec[r] == at);
            uint32_t block = 0;
            memcpy(&block, out.get() + at, 4);
            uint32_t l_seq = 0;
            memcpy(&l_seq, out.get() + at + 20, 4);
            EXPECT(l_seq == c.len[r]);
            at += 4 + (uint64_t)block;
        }
        EXPECT(at == need);
    }
    return rc;
}

}  // namespace

int main() {
    std::mt19937_64 rng(4190);
    uint8_t head[64];
    uint64_t n_head = 0;
    EXPECT(leon_bam_header(head, sizeof head, &n_head) == LEON_OK && n_head == 35 && memcmp(head, "BAM\1", 4) == 0);
    {
        std::unique_ptr<uint8_t[]> tight(new uint8_t[35]);
        EXPECT(leon_bam_header(tight.get(), 35, &n_head) == LEON_OK);
        EXPECT(leon_bam_header(tight.get(), 34, &n_head) == LEON_E_OVERFLOW && n_head == 35);
    }
    for (uint32_t draw_no = 0; draw_no < 60; draw_no++) {
        const bool with_hdr = draw_no % 3 != 0, with_quals = draw_no % 4 != 3;
        const uint32_t n = draw_no == 0 ? 0 : draw_no % 7 == 0 ? 9000 : 1 + (uint32_t)(rng() % 40);
        Call c = draw(rng, n, with_hdr, draw_no % 2 ? 99990 : 0);
        uint64_t size = 0;
        EXPECT(run(c, with_hdr, with_quals, 0, 1 + draw_no % 4, &size) == LEON_OK);
        if (n) {
            EXPECT(run(c, with_hdr, with_quals, ~0ull, 1, &size) == LEON_E_OVERFLOW);
            const uint64_t fewer = c.bases.size() + 1;
            EXPECT(run(c, with_hdr, with_quals, 0, 1, &size, nullptr, &fewer) == LEON_E_INVALID);
        }
        if (with_hdr && n >= 3) {
            std::vector<uint64_t> off = c.hdr_off;               // backwards, far past the bytes, below the first: nothing is read through them
            std::swap(off[1], off[2]);
            if (off[1] != off[2]) EXPECT(run(c, true, with_quals, 0, 1, &size, &off) == LEON_E_INVALID);
            off = c.hdr_off; off[n] += 1ull << 40;
            EXPECT(run(c, true, with_quals, 0, 1, &size, &off) == LEON_E_INVALID);
            off = c.hdr_off; off[0] += 1ull << 40;
            EXPECT(run(c, true, with_quals, 0, 1, &size, &off) == LEON_E_INVALID);
        }
        if (with_hdr && n) {                                     // a name of 255 bytes, and a quality byte 32 at the very last base
            Call d = c;
            const uint64_t r = rng() % n;
            std::vector<uint8_t> hdr(d.hdr.begin(), d.hdr.begin() + (d.hdr_off[r] - 77));
            hdr.insert(hdr.end(), 255, 'n');
            hdr.insert(hdr.end(), d.hdr.begin() + (d.hdr_off[r + 1] - 77), d.hdr.end());
            const int64_t grown = 255 - (int64_t)(d.hdr_off[r + 1] - d.hdr_off[r]);
            for (uint64_t i = r + 1; i <= n; i++) d.hdr_off[i] = (uint64_t)((int64_t)d.hdr_off[i] + grown);
            d.hdr = hdr; d.lay.hdr_bytes = hdr.size();
            EXPECT(run(d, true, with_quals, 0, 1, &size) == LEON_E_INVALID && strstr(leon_last_error(nullptr), "its name has 255 bytes") != nullptr);
        }
        if (with_quals && !c.quals.empty()) {
            Call d = c;
            d.quals.back() = 32;
            EXPECT(run(d, with_hdr, true, 0, 2, &size) == LEON_E_INVALID && strstr(leon_last_error(nullptr), "a quality byte below 33") != nullptr);
        }
    }
    if (failures) { printf("bam records: %d failure(s)\n", failures); return 1; }
    printf("bam records: ok\n");
    return 0;
}
