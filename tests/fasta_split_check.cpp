// fasta_split_check.cpp -- a stand-alone program for AddressSanitizer / UBSan (tests/test_fasta_split_cpu.py compiles and runs it): the
// serial FASTA split of leon_amd/csrc/host_fasta.h over the cases of tests/fasta_shapes.py, read from the file the test writes (argv[1]):
//     u64 n_cases, then per case: u64 n_text, last, max_records, wrap, the text;
//                                 u64 n_records, consumed, header_bytes, base_bytes, stop, reason, single_max, next_header;
//                                 the headers, header_off[n_records + 1], the bases, base_off[n_records + 1].
// Every buffer is allocated to its exact size (the text too), so that the sanitizer sees the first byte beyond; then the tables one entry
// and the blobs one byte too small: LEON_E_OVERFLOW, the same result fields.  Prints "fasta split: ok" and exits 0.
#include "../leon_amd/csrc/host_fasta.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "fasta split: case %llu, line %d: %s\n", (unsigned long long)g_case, __LINE__, #c); exit(1); } } while (0)
uint64_t g_case = 0;
FILE* g_in = nullptr;

uint64_t u64() { uint64_t v = 0; REQUIRE(fread(&v, 8, 1, g_in) == 1); return v; }
std::vector<uint8_t> blob(uint64_t n) { std::vector<uint8_t> b(n); REQUIRE(!n || fread(b.data(), 1, n, g_in) == n); return b; }
std::vector<uint64_t> table(uint64_t n) { std::vector<uint64_t> t(n); for (auto& x : t) x = u64(); return t; }

bool same(const leon_fasta_split_result& a, const leon_fasta_split_result& b) {
    return a.n_records == b.n_records && a.consumed == b.consumed && a.header_bytes == b.header_bytes && a.base_bytes == b.base_bytes && a.stop == b.stop &&
           a.reason == b.reason && a.single_max == b.single_max && a.next_header == b.next_header;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: fasta_split_check CASES\n"); return 2; }
    const uint64_t n_cases = u64();
    for (g_case = 0; g_case < n_cases; g_case++) {
        const uint64_t n_text = u64();
        const int last = (int)u64();
        const uint64_t max_records = u64(), wrap = u64();
        const std::vector<uint8_t> text = blob(n_text);
        leon_fasta_split_result want{};
        want.n_records = u64(); want.consumed = u64(); want.header_bytes = u64(); want.base_bytes = u64();
        want.stop = (uint32_t)u64(); want.reason = (uint32_t)u64(); want.single_max = u64(); want.next_header = u64();
        const std::vector<uint8_t> headers = blob(want.header_bytes);
        const std::vector<uint64_t> header_off = table(want.n_records + 1);
        const std::vector<uint8_t> bases = blob(want.base_bytes);
        const std::vector<uint64_t> base_off = table(want.n_records + 1);
        REQUIRE(!leon::fasta_split_refusal(text.data(), n_text, &want, &want, &want, &want, &want));
        const uint64_t cap = want.header_bytes > want.base_bytes ? want.header_bytes : want.base_bytes;
        {   // exactly enough room
            std::vector<uint8_t> h(cap), b(cap);
            std::vector<uint64_t> ho(want.n_records + 1), bo(want.n_records + 1);
            leon_fasta_split_result got{};
            REQUIRE(leon::fasta_split(text.data(), n_text, last, max_records, wrap, h.data(), ho.data(), b.data(), bo.data(), cap, want.n_records + 1, &got) == LEON_OK);
            REQUIRE(same(got, want));
            h.resize(want.header_bytes); b.resize(want.base_bytes);
            REQUIRE(h == headers && b == bases && ho == header_off && bo == base_off);
        }
        {   // the room a caller gives that does not want to think
            std::vector<uint8_t> h(n_text), b(n_text);
            std::vector<uint64_t> ho(n_text / 2 + 2), bo(n_text / 2 + 2);
            leon_fasta_split_result got{};
            REQUIRE(leon::fasta_split(text.data(), n_text, last, max_records, wrap, h.data(), ho.data(), b.data(), bo.data(), n_text, n_text / 2 + 2, &got) == LEON_OK);
            REQUIRE(same(got, want));
        }
        {   // one table entry too few
            std::vector<uint8_t> h(cap), b(cap);
            std::vector<uint64_t> ho(want.n_records), bo(want.n_records);
            leon_fasta_split_result got{};
            REQUIRE(leon::fasta_split(text.data(), n_text, last, max_records, wrap, h.data(), ho.data(), b.data(), bo.data(), cap, want.n_records, &got) == LEON_E_OVERFLOW);
            REQUIRE(same(got, want));
        }
        if (cap) {   // one byte too few
            std::vector<uint8_t> h(cap - 1), b(cap - 1);
            std::vector<uint64_t> ho(want.n_records + 1), bo(want.n_records + 1);
            leon_fasta_split_result got{};
            REQUIRE(leon::fasta_split(text.data(), n_text, last, max_records, wrap, h.data(), ho.data(), b.data(), bo.data(), cap - 1, want.n_records + 1, &got) == LEON_E_OVERFLOW);
            REQUIRE(same(got, want));
        }
    }
    REQUIRE(fgetc(g_in) == EOF);
    printf("fasta split: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
