// Stand-alone check of the host dictionary chain (leon_amd/csrc/host_rc.h), meant to be built with
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -pthread
// and run as a program of its own (tests/test_chain_selftest_cpu.py does both).  Random and skewed k-mers go through the
// worker -- ChainFeed's helpers, its ring, and the chain's record loop -- once per LEON_CHAIN_FORM and under several ring
// shapes; the bytes must equal those of the plain form (AnchorDictCoder::encode_kmers: one division per symbol, no
// records), and decode_anchor_dict must give the k-mers back.  Exit status 0 and a last line "chain selftest: ok".
#include "../leon_amd/csrc/host_rc.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>

using namespace leon;

static std::vector<uint64_t> make_kmers(const char* kind, uint32_t k, size_t n, uint64_t seed) {
    const uint32_t W = k >= 32 ? 2u : 1u;
    std::mt19937_64 rng(seed);
    std::vector<uint64_t> km(n * W);
    for (size_t a = 0; a < n; a++) {
        unsigned __int128 x = 0;
        for (uint32_t i = 0; i < k; i++) {
            uint32_t sy;
            const uint64_t u = rng();
            if (!strcmp(kind, "polyA")) sy = (u % 40000) == 0 ? 3u : 0u;
            else if (!strcmp(kind, "skewed")) sy = (u % 100) < 97 ? 0u : 1u + (uint32_t)((u >> 32) % 3);
            else if (!strcmp(kind, "two_letter")) sy = (uint32_t)(u & 1) * 2;
            else sy = (uint32_t)(u & 3);
            x = (x << 2) | sy;
        }
        km[a * W] = (uint64_t)x;
        if (W == 2) km[a * W + 1] = (uint64_t)(x >> 64);
    }
    return km;
}

static std::vector<uint8_t> through_worker(const std::vector<uint64_t>& km, uint32_t k, size_t pieces) {
    const uint32_t W = k >= 32 ? 2u : 1u;
    const size_t n = km.size() / W;
    AnchorDictWorker worker(k);
    const size_t step = std::max<size_t>(1, (n + pieces - 1) / pieces);
    for (size_t i = 0; i < n; i += step) {
        const size_t m = std::min(step, n - i);
        worker.push(std::vector<uint64_t>(km.begin() + i * W, km.begin() + (i + m) * W));
    }
    worker.drain();
    AnchorDictCoder& cd = worker.coder();
    cd.flush();
    return std::vector<uint8_t>(cd.data(), cd.data() + cd.size());
}

int main() {
    struct Case { const char* kind; uint32_t k; size_t n; };
    const Case cases[] = {
        {"uniform", 31, 1}, {"uniform", 31, 2}, {"uniform", 31, 1056}, {"uniform", 31, 1057}, {"uniform", 31, 1058}, {"uniform", 31, 30000},
        {"uniform", 63, 519}, {"uniform", 63, 520}, {"uniform", 63, 521}, {"uniform", 63, 8000}, {"uniform", 21, 3000}, {"uniform", 5, 2000},
        {"polyA", 31, 20000}, {"skewed", 31, 20000}, {"two_letter", 31, 20000}, {"skewed", 63, 6000},
    };
    struct Shape { const char* form; const char* ring; const char* helpers; const char* spares; size_t pieces; };
    const Shape shapes[] = {
        {"quotient", "512", "3", "3", 3}, {"carry", "512", "3", "3", 3}, {"carry", "4", "2", "6", 5}, {"carry", "8", "1", "0", 1}, {"quotient", "4", "2", "6", 5},
    };
    int bad = 0;
    uint64_t seed = 1;
    for (const Case& c : cases) {
        const std::vector<uint64_t> km = make_kmers(c.kind, c.k, c.n, seed++);
        AnchorDictCoder plain;
        plain.encode_kmers(km.data(), c.n, c.k);
        plain.flush();
        const std::vector<uint8_t> ref(plain.data(), plain.data() + plain.size());
        std::vector<uint64_t> back(km.size());
        if (!decode_anchor_dict(ref.data(), ref.size(), c.n, c.k, back.data()) || back != km) {
            printf("FAIL %s k=%u n=%zu: the plain form's stream does not decode to its k-mers\n", c.kind, c.k, c.n);
            bad++;
        }
        for (const Shape& s : shapes) {
            setenv("LEON_CHAIN_FORM", s.form, 1);
            setenv("LEON_CHAIN_RING", s.ring, 1);
            setenv("LEON_CHAIN_HELPERS", s.helpers, 1);
            setenv("LEON_CHAIN_SPARES", s.spares, 1);
            const std::vector<uint8_t> got = through_worker(km, c.k, s.pieces);
            if (got != ref) {
                printf("FAIL %s k=%u n=%zu form=%s ring=%s helpers=%s spares=%s: %zu bytes against %zu\n", c.kind, c.k, c.n, s.form, s.ring, s.helpers, s.spares, got.size(), ref.size());
                bad++;
            }
        }
    }
    if (bad) { printf("chain selftest: %d FAILED\n", bad); return 1; }
    printf("chain selftest: ok\n");
    return 0;
}
