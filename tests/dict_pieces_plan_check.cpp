// dict_pieces_plan_check.cpp -- leon_plan.hpp's check of the piece table `leon -c -dict-pieces` writes (plan::check_dict_pieces): good
// tables pass, every rule is broken one at a time and refused with the words that begin "<file>: dictionary pieces: ".
// Stand-alone: g++ -std=c++17 -I include tests/dict_pieces_plan_check.cpp, nothing to link; tests/test_dict_pieces_cpu.py builds it plain and
// under AddressSanitizer + UBSan.
#include "../leon_amd/host/leon_plan.hpp"

#include <cstdio>

using namespace leon_host;
using namespace leon_host::layout;

static int g_checks = 0;
#define REQUIRE(cond) do { g_checks++; if (!(cond)) { fprintf(stderr, "dict_pieces_plan_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static const std::string kFile = "x.fastq.leon";

// "" when the table passes (or the file is of the single-stream form: *pieced says which), else the refusal
static std::string verdict(bool single, bool pieces, bool table, const std::vector<uint64_t>& t, uint64_t bytes, uint64_t n_anchors, bool* pieced = nullptr) {
    try {
        const bool r = plan::check_dict_pieces(kFile, single, pieces, table, t, bytes, n_anchors);
        if (pieced) *pieced = r;
        return "";
    } catch (const Exception& e) { return e.what(); }
}
static bool refused(const std::string& v, const std::string& with) {
    const std::string head = kFile + ": dictionary pieces: ";
    return v.compare(0, head.size(), head) == 0 && v.find(with) != std::string::npos;
}

static std::vector<uint64_t> good_table(uint64_t n_anchors, uint64_t P, uint64_t* bytes) {
    std::vector<uint64_t> t = {DICT_PIECES_ORDER0, P};
    *bytes = 0;
    for (uint64_t a = 0; a < n_anchors; a += P) { t.push_back(8 + (a * 7 + P) % 300); *bytes += t.back(); }
    return t;
}

int main() {
    bool pieced = true;
    // the single-stream form: neither dataset, with or without leon/anchors/dict -- not this check's business
    REQUIRE(verdict(true, false, false, {}, 0, 100, &pieced).empty() && !pieced);
    REQUIRE(verdict(false, false, false, {}, 0, 100, &pieced).empty() && !pieced);
    const uint64_t Ps[] = {1, 3, 64, 1024, 1ull << 20};
    for (uint64_t P : Ps) {
        const uint64_t ns[] = {0, 1, P - 1, P, P + 1, 5 * P + 2};
        for (uint64_t n : ns) {
            if (n > 6000) continue;
            uint64_t bytes = 0;
            const std::vector<uint64_t> t = good_table(n, P, &bytes);
            REQUIRE(t.size() - 2 == (n + P - 1) / P);
            REQUIRE(verdict(false, true, true, t, bytes, n, &pieced).empty() && pieced);
            // both datasets or neither; not both forms in one file
            REQUIRE(refused(verdict(false, true, false, {}, bytes, n), std::string(DS_ANCHOR_DICT_PIECE_TABLE) + " is missing"));
            REQUIRE(refused(verdict(false, false, true, t, 0, n), std::string(DS_ANCHOR_DICT_PIECES) + " is missing"));
            REQUIRE(refused(verdict(true, true, true, t, bytes, n), std::string("holds ") + DS_ANCHOR_DICT + " as well"));
            // the kind, the piece size
            std::vector<uint64_t> u = t;
            u[0] = 2;
            REQUIRE(refused(verdict(false, true, true, u, bytes, n), "unknown kind 2"));
            u = t; u[1] = 0;
            REQUIRE(refused(verdict(false, true, true, u, bytes, n), "0 anchors per piece"));
            u = t; u[1] = (1ull << 20) + 1;
            REQUIRE(refused(verdict(false, true, true, u, bytes, n), "anchors per piece"));
            // the count: one piece more, one fewer, another anchor count
            u = t; u.push_back(8);
            REQUIRE(refused(verdict(false, true, true, u, bytes + 8, n), "the table holds"));
            if (n) { u = t; u.pop_back(); REQUIRE(refused(verdict(false, true, true, u, bytes - t.back(), n), "the table holds")); }
            REQUIRE(refused(verdict(false, true, true, t, bytes, n + P), "the table holds"));
            // the sizes: every entry off by one either way, a piece below its flush bytes, the dataset a byte short or long
            for (size_t i = 2; i < t.size(); i++) {
                u = t; u[i]++;
                REQUIRE(refused(verdict(false, true, true, u, bytes, n), "add up to"));
                u = t; u[i]--;
                REQUIRE(refused(verdict(false, true, true, u, bytes, n), u[i] < 8 ? "flush bytes" : "add up to"));
                u = t; u[i] = 7;
                REQUIRE(refused(verdict(false, true, true, u, bytes, n), "has 7 bytes"));
                u = t; u[i] = ~0ull;                             // (the sum must not wrap)
                REQUIRE(refused(verdict(false, true, true, u, bytes, n), "add up to more than"));
            }
            if (n) {
                REQUIRE(refused(verdict(false, true, true, t, bytes + 1, n), "add up to"));
                REQUIRE(refused(verdict(false, true, true, t, bytes - 1, n), "add up to"));
            }
        }
    }
    REQUIRE(refused(verdict(false, true, true, {}, 0, 0), "too short"));
    REQUIRE(refused(verdict(false, true, true, {DICT_PIECES_ORDER0}, 0, 0), "too short"));
    printf("dict_pieces_plan_check: ok, %d checks\n", g_checks);
    return 0;
}
