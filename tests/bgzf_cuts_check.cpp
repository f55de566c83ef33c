// bgzf_cuts_check.cpp -- a stand-alone program for AddressSanitizer / UBSan (tests/test_bgzf_records_cpu.py compiles it together with
// leon_amd/csrc/host_streams.cpp): leon_host_bgzf_record_cuts over the shapes of tests/bgzf_records.py and fixed-seed random record
// lengths, with heads of 0, 1 and W bytes, with and without `last`.  The tables are allocated to their exact sizes (and one entry too
// small: LEON_E_OVERFLOW, nothing written past them), so that the sanitizer sees the first entry beyond; the members are set against a
// linear restatement of the rule.  Prints "bgzf cuts: ok" and exits 0.
#include "../include/leon_dna.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace leon { thread_local std::string g_error; void set_create_error(const std::string& m) { g_error = m; } }
extern "C" const char* leon_last_error(const leon_dna_ctx*) { return leon::g_error.c_str(); }

namespace {

constexpr uint64_t W = LEON_BGZF_MEMBER_TEXT;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "bgzf cuts: line %d: %s (%s)\n", __LINE__, #c, leon::g_error.c_str()); exit(1); } } while (0)

// the rule, one start at a time
std::vector<std::pair<uint64_t, uint64_t>> rule(const std::vector<uint64_t>& s, bool last, uint64_t* taken) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    size_t i = 0;
    while (i + 1 < s.size() && (last || s.back() - s[i] > W)) {
        if (s[i + 1] - s[i] > W) {
            for (uint64_t a = s[i]; a < s[i + 1]; a += W) out.push_back({a, s[i + 1] - a < W ? s[i + 1] - a : W});
            i++;
            continue;
        }
        size_t j = i + 1;
        while (j + 1 < s.size() && s[j + 1] <= s[i] + W) j++;
        out.push_back({s[i], s[j] - s[i]});
        i = j;
    }
    *taken = s.empty() ? 0 : s[i];
    return out;
}

void one(const std::vector<uint64_t>& lengths, uint64_t n_head, int last) {
    std::vector<uint64_t> off(lengths.size() + 1, 0), starts;
    for (size_t r = 0; r < lengths.size(); r++) off[r + 1] = off[r] + lengths[r];
    if (n_head) starts.push_back(0);
    for (uint64_t x : off) starts.push_back(n_head + x);
    uint64_t want_taken = 0;
    const auto want = rule(starts, last != 0, &want_taken);
    uint64_t n = 0, taken = 0;
    REQUIRE(leon_host_bgzf_record_cuts(off.data(), lengths.size(), n_head, last, nullptr, nullptr, 0, &n, &taken) == LEON_OK);
    REQUIRE(n == want.size() && taken == want_taken && n <= 3 * ((n_head + off.back()) / W) + 2);
    {
        std::vector<uint64_t> begin(n);                        // exactly as many entries as there are members
        std::vector<uint32_t> len(n);
        uint64_t n2 = 0;
        REQUIRE(leon_host_bgzf_record_cuts(off.data(), lengths.size(), n_head, last, begin.data(), len.data(), n, &n2, &taken) == LEON_OK);
        REQUIRE(n2 == n && taken == want_taken);
        for (uint64_t c = 0; c < n; c++) REQUIRE(begin[c] == want[c].first && len[c] == want[c].second);
    }
    if (n > 1) {
        std::vector<uint64_t> begin(n - 1);
        std::vector<uint32_t> len(n - 1);
        uint64_t n2 = 0;
        REQUIRE(leon_host_bgzf_record_cuts(off.data(), lengths.size(), n_head, last, begin.data(), len.data(), n - 1, &n2, &taken) == LEON_E_OVERFLOW);
        REQUIRE(n2 == n);
    }
}

}  // namespace

int main() {
    std::vector<std::vector<uint64_t>> shapes = {
        {}, {1}, std::vector<uint64_t>(128, 256), {16384, 16384, 16385, 16384}, {5, 32768, 5}, {5, 32769, 5}, {70000, 10, 20, 65536}, {7, 40000, 32769, 7},
        std::vector<uint64_t>(200000, 3), std::vector<uint64_t>(70000, 1)};
    shapes.push_back(std::vector<uint64_t>(127, 256)); shapes.back().push_back(257);
    shapes.push_back(std::vector<uint64_t>(10, 50)); shapes.back().push_back(100000); shapes.back().insert(shapes.back().end(), 10, 50);
    for (int draw = 0; draw < 300; draw++) {
        std::vector<uint64_t> l(1 + rnd() % 60);
        for (auto& x : l) x = draw % 3 ? 1 + rnd() % 40000 : (rnd() % 5 ? 1 + rnd() % 700 : 1 + rnd() % 40000);
        shapes.push_back(l);
    }
    uint64_t calls = 0;
    for (const auto& s : shapes)
        for (uint64_t n_head : {(uint64_t)0, (uint64_t)1, W, 1 + rnd() % W})
            for (int last = 0; last < 2; last++, calls++) one(s, n_head, last);
    // what the call refuses
    uint64_t n = 0, taken = 0;
    const uint64_t back[] = {0, 5, 5, 9}, late[] = {1, 5};
    REQUIRE(leon_host_bgzf_record_cuts(back, 3, 0, 1, nullptr, nullptr, 0, &n, &taken) == LEON_E_INVALID);
    REQUIRE(leon_host_bgzf_record_cuts(late, 1, 0, 1, nullptr, nullptr, 0, &n, &taken) == LEON_E_INVALID);
    REQUIRE(leon_host_bgzf_record_cuts(back, 1, W + 1, 1, nullptr, nullptr, 0, &n, &taken) == LEON_E_INVALID);
    REQUIRE(leon_host_bgzf_record_cuts(nullptr, 1, 0, 1, nullptr, nullptr, 0, &n, &taken) == LEON_E_INVALID);
    printf("bgzf cuts: ok (%llu calls)\n", (unsigned long long)calls);
    return 0;
}
