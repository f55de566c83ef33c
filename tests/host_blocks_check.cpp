// host_blocks_check -- leon_amd/csrc/host_blocks.h on the CPU, stand-alone (tests/test_rc_edges_cpu.py builds it plain and with
// -fsanitize=address,undefined and runs it on the streams of tests/rc_edges.py).
//
//   host_blocks_check DIR one:NAME ... pair:NAME_A,NAME_B ...
//
// DIR/NAME.sym holds a stream as (model, value) byte pairs, DIR/NAME.pay the oracle's payload, DIR/sizes the models' alphabet sizes
// (one byte each; 0 stands for 256).  The 64-bit records (cumLow | freq << 22 | model << 44) are made HERE, from plain cumulative-count
// models -- not by k_rc_records --, so the chains are held to the oracle with nothing of the device in between.
//   one:NAME     HostBlockCoder::code, the stream cut into 1, 16 and 64 pieces of whole tiles as rc_blocks_on_host cuts it
//   pair:A,B     HostBlockCoder::code2 on the two streams (of unequal length), in 1 and 16 pieces
// Every payload must equal the oracle's in size and bytes.  Exit status 0 and a line "host_blocks_check: ok ..." when all do.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../leon_amd/csrc/host_blocks.h"

namespace {

std::vector<uint8_t> read_file(const std::string& path) {
    std::vector<uint8_t> out;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "host_blocks_check: cannot open %s\n", path.c_str()); exit(2); }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

// Order0Model: a count per value, and the counts' sums over 16 values so that a cumulative count is 30 additions at the most
struct Model {
    uint32_t n = 0, cnt[256], blk[16];
    void clear(uint32_t size) {
        n = size;
        memset(blk, 0, sizeof blk);
        for (uint32_t i = 0; i < 256; i++) { cnt[i] = i < n ? 1 : 0; blk[i >> 4] += cnt[i]; }
    }
    uint32_t below(uint32_t v) const {
        uint32_t s = 0;
        for (uint32_t b = 0; b < (v >> 4); b++) s += blk[b];
        for (uint32_t i = v & ~15u; i < v; i++) s += cnt[i];
        return s;
    }
    void update(uint32_t v) { cnt[v]++; blk[v >> 4]++; }
};

struct Stream {
    std::string name;
    std::vector<uint64_t> rec;
    std::vector<uint8_t> want;
};

std::vector<uint32_t> g_sizes;
uint32_t g_small_sizes = 0, g_n_small = 0;

Stream load(const std::string& dir, const std::string& name) {
    Stream s;
    s.name = name;
    const std::vector<uint8_t> sym = read_file(dir + "/" + name + ".sym");
    s.want = read_file(dir + "/" + name + ".pay");
    std::vector<Model> models(g_sizes.size());
    for (size_t m = 0; m < models.size(); m++) models[m].clear(g_sizes[m]);
    const size_t n = sym.size() / 2;
    s.rec.resize(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t m = sym[2 * i], v = sym[2 * i + 1];
        if (m >= models.size() || v >= models[m].n) { fprintf(stderr, "host_blocks_check: %s: bad symbol at %zu\n", name.c_str(), i); exit(2); }
        const uint64_t lo = models[m].below(v), fr = models[m].cnt[v];
        if (lo + fr > leon::HB_COUNT_MASK) { fprintf(stderr, "host_blocks_check: %s: counts beyond 22 bits at %zu\n", name.c_str(), i); exit(2); }
        s.rec[i] = lo | fr << leon::HB_COUNT_BITS | (uint64_t)m << (2 * leon::HB_COUNT_BITS);
        models[m].update(v);
    }
    return s;
}

int compare(const leon::HostBlockCoder& c, const Stream& s, const char* how, uint32_t pieces) {
    if (c.size() == s.want.size() && (c.size() == 0 || memcmp(c.data(), s.want.data(), c.size()) == 0)) return 0;
    size_t at = 0;
    while (at < c.size() && at < s.want.size() && c.data()[at] == s.want[at]) at++;
    fprintf(stderr, "host_blocks_check: %s, %s in %u pieces: %zu bytes against the oracle's %zu, the first difference at byte %zu\n",
            s.name.c_str(), how, pieces, c.size(), s.want.size(), at);
    return 1;
}

// rc_blocks_on_host's cut: `pieces` chunks of Tc whole tiles, Tc from the longest stream of the call
void cut(uint64_t longest, uint32_t pieces, uint32_t& n_chunks, uint64_t& per_chunk) {
    const uint64_t max_tiles = (longest + 63) / 64;
    n_chunks = (uint32_t)(pieces < max_tiles ? pieces : (max_tiles ? max_tiles : 1));
    per_chunk = 64 * ((max_tiles + n_chunks - 1) / n_chunks);
}

int run_one(const Stream& s) {
    int bad = 0;
    for (uint32_t pieces : {1u, 16u, 64u}) {
        leon::HostBlockCoder c;
        c.start(g_small_sizes, g_n_small);
        uint32_t n_chunks;
        uint64_t per;
        cut(s.rec.size(), pieces, n_chunks, per);
        for (uint32_t ch = 0; ch < n_chunks; ch++) {
            const uint64_t a0 = std::min<uint64_t>(s.rec.size(), ch * per), a1 = std::min<uint64_t>(s.rec.size(), (ch + 1) * per);
            c.code(s.rec.data() + a0, a1 - a0);
        }
        c.flush();
        bad += compare(c, s, "code", pieces);
    }
    return bad;
}

int run_pair(const Stream& a, const Stream& b) {
    int bad = 0;
    for (uint32_t pieces : {1u, 16u}) {
        leon::HostBlockCoder ca, cb;
        ca.start(g_small_sizes, g_n_small);
        cb.start(g_small_sizes, g_n_small);
        uint32_t n_chunks;
        uint64_t per;
        cut(std::max(a.rec.size(), b.rec.size()), pieces, n_chunks, per);
        for (uint32_t ch = 0; ch < n_chunks; ch++) {
            const uint64_t a0 = std::min<uint64_t>(a.rec.size(), ch * per), a1 = std::min<uint64_t>(a.rec.size(), (ch + 1) * per);
            const uint64_t b0 = std::min<uint64_t>(b.rec.size(), ch * per), b1 = std::min<uint64_t>(b.rec.size(), (ch + 1) * per);
            leon::HostBlockCoder::code2(ca, a.rec.data() + a0, a1 - a0, cb, b.rec.data() + b0, b1 - b0);
        }
        ca.flush();
        cb.flush();
        bad += compare(ca, a, "code2 (first)", pieces) + compare(cb, b, "code2 (second)", pieces);
    }
    return bad;
}

const Stream& get(std::vector<Stream>& all, const std::string& dir, const std::string& name) {
    for (const Stream& s : all) if (s.name == name) return s;
    all.push_back(load(dir, name));
    return all.back();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: host_blocks_check DIR one:NAME ... pair:A,B ...\n"); return 2; }
    const std::string dir = argv[1];
    for (uint8_t b : read_file(dir + "/sizes")) g_sizes.push_back(b ? b : 256u);
    while (g_n_small < g_sizes.size() && g_sizes[g_n_small] < 16) { g_small_sizes |= g_sizes[g_n_small] << (4 * g_n_small); g_n_small++; }
    if (g_n_small > 8 || g_sizes.size() > 128) { fprintf(stderr, "host_blocks_check: a model set the host chains do not take\n"); return 2; }
    std::vector<Stream> all;
    all.reserve(2 * (size_t)argc);                               // (references into it stay valid)
    int bad = 0, runs = 0;
    uint64_t symbols = 0;
    for (int i = 2; i < argc; i++) {
        const std::string arg = argv[i];
        if (arg.rfind("one:", 0) == 0) {
            const Stream& s = get(all, dir, arg.substr(4));
            bad += run_one(s);
            symbols += 3 * s.rec.size();
        } else if (arg.rfind("pair:", 0) == 0) {
            const size_t comma = arg.find(',');
            if (comma == std::string::npos) { fprintf(stderr, "host_blocks_check: %s\n", arg.c_str()); return 2; }
            const Stream& a = get(all, dir, arg.substr(5, comma - 5));
            const Stream& b = get(all, dir, arg.substr(comma + 1));
            bad += run_pair(a, b);
            symbols += 2 * (a.rec.size() + b.rec.size());
        } else { fprintf(stderr, "host_blocks_check: %s\n", arg.c_str()); return 2; }
        runs++;
    }
    if (bad) return 1;
    printf("host_blocks_check: ok, %d runs, %llu symbols coded\n", runs, (unsigned long long)symbols);
    return 0;
}
