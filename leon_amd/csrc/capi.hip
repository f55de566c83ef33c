// capi.hip -- the C-ABI of include/leon_dna.h: the context, its device memory, and the stage pipeline
//   pack -> anchor resolution (windows, fixpoint rounds) -> anchor sort -> walk -> symbols -> range coder -> D2H.
// Every other call lives beside its kernels, those that take a device_id (device_call.h) and the context's others (ctx.h): DESIGN.md 2.1.
#include "ctx.h"
#include "staging.h"
#include "host_dict_pieces.h"

#include "prim.h"

#include <atomic>
#include <cstring>
#include <mutex>
#include <thread>

using namespace leon;

namespace { thread_local std::string g_create_error; }
namespace leon {
void set_create_error(const std::string& msg) { g_create_error = msg; }
ReadsDev reads_view(leon_dna_ctx* c, const uint64_t* d_off, uint64_t n) {
    ReadsDev R{};
    R.packed = c->packed.as<uint32_t>(); R.nmask = c->nmask.as<uint32_t>(); R.slot_off = c->slot_off.as<uint64_t>();
    R.base_off = d_off; R.len = c->rlen.as<uint32_t>(); R.n_count = c->ncount.as<uint32_t>();
    R.n = n; R.k = c->cfg.kmer_size;
    return R;
}
// The batch buffers of a stage, sized by the stage and by leon_dna_reserve alike.
int ensure_pack_bufs(leon_dna_ctx* c, uint64_t n, uint64_t n_slots) {
    HIPCHK(c, c->packed.ensure((n_slots * 2 + 16) * 4)); HIPCHK(c, c->nmask.ensure((n_slots + 4) * 4));   // (wave loads reach 12 dwords past a pass start)
    HIPCHK(c, c->rlen.ensure(n * 4)); HIPCHK(c, c->ncount.ensure(n * 4));
    return LEON_OK;
}
int check_offsets(leon_dna_ctx* c, const uint64_t* d_off, uint64_t n, const char* too_long, uint64_t* n_slots, bool spin) {
    hipStream_t s = c->stream;
    uint64_t* const h_rb = c->rb(); uint32_t* const d_bad = c->counters.as<uint32_t>() + 4;
    HIPCHK(c, c->slot_off.ensure((n + 1) * 8));
    uint64_t* slot_off = c->slot_off.as<uint64_t>();
    HIPCHK(c, hipMemsetAsync(d_bad, 0, 4, s));
    launch_read_slots(s, d_off, n, slot_off, d_bad);
    if (n_slots) {
        if (int rc = run_prim(c, [&](void* t, size_t& b) { return prim::ExclusiveSum(t, b, slot_off, slot_off, n + 1, s); })) return rc;
        HIPCHK(c, hipMemcpyAsync(h_rb + 0, slot_off + n, 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipMemcpyAsync(h_rb + 1, d_bad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, spin ? spin_sync(s) : hipStreamSynchronize(s));
    if (n_slots) *n_slots = h_rb[0];
    if ((uint32_t)h_rb[1]) return fail(c, LEON_E_INVALID, std::string("offsets are not monotonic (or ") + too_long + ")");
    return LEON_OK;
}
}  // namespace leon
namespace {

uint64_t splitmix_rv(uint32_t idx) {     // built-in simplehash16 table, see DESIGN.md "recalled constants"
    uint64_t s = 0x4C454F4EULL + (uint64_t)(idx + 1) * 0x9E3779B97F4A7C15ULL;
    s = (s ^ (s >> 30)) * 0xBF58476D1CE4E5B9ULL;
    s = (s ^ (s >> 27)) * 0x94D049BB133111EBULL;
    return s ^ (s >> 31);
}
uint64_t hash_seed0() {                  // HashFunctors::generate_hash_seed, seed_tab[0], user_seed 0
    const uint64_t r0 = 0xAAAAAAAA55555555ULL, r3 = 0xB5B5B5B54B4B4B4BULL;
    return r0 * r3;
}

// a table of `cap` slots in M, D the kernels' view of it
int dict_alloc(leon_dna_ctx* c, DictMem& M, DictDev& D, uint64_t cap) {
    const uint32_t W = kmer_words(c->cfg.kmer_size);
    D = DictDev{};
    hipError_t e = M.slots.exactly(cap * 16 * W);
    if (e == hipSuccess && W == 1) e = M.tent.exactly(cap * 8);
    if (e == hipSuccess) e = M.addr.exactly(cap * 4);
    if (e != hipSuccess)                                      // nothing of a half-built table is kept: M goes with its owner
        return fail(c, LEON_E_HIP, std::string("anchor dictionary allocation: ") + hipGetErrorString(e));
    D.slots = M.slots.as<uint64_t>(); D.addr = M.addr.as<uint32_t>();
    if (W == 1) { D.tent = M.tent.as<uint64_t>(); D.tstride = 1; }
    else { D.tent = D.slots + 3; D.tstride = 4; }            // two-word keys keep tent inside the slots
    D.mask = cap - 1;
    D.n_keys = c->d_nkeys.as<unsigned long long>();
    D.wbits = c->wbits.as<uint32_t>();
    D.fbits = c->fbits.as<uint32_t>();
    D.pbits = c->pbits.as<uint32_t>();
    D.fwshift = 32 - (c->fbits_log2 - 6);
    minimizer_geometry(c->cfg.kmer_size, D.mm_m, D.mm_P, D.mm_c);
    D.err = c->errflag.as<int>() + 2;
    launch_dict_init(c->stream, D, cap, W);
    return LEON_OK;
}
// capacity >= 4 * keys: the look-up kernels are bound by chains of dependent loads, not by the table footprint
int dict_reserve(leon_dna_ctx* c, uint64_t keys) {
    uint64_t need = 1024;
    while (need < 4 * keys) need <<= 1;                   // load factor <= 1/4: a miss costs 1.2 dependent probes, not 2.5
    if (need <= c->dict_cap) return LEON_OK;
    if (need > (1ull << 32)) return fail(c, LEON_E_OVERFLOW, "anchor dictionary would exceed 2^32 slots");
    DictMem nm; DictDev nd{};
    HIPCHK(c, hipMemsetAsync(c->d_nkeys.p, 0, 8, c->stream));
    int rc = dict_alloc(c, nm, nd, need);
    if (rc) return rc;
    if (c->dict_cap) {
        launch_dict_rehash(c->stream, c->D, c->dict_cap, nd, c->cfg.kmer_size);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->dict_mem.swap(nm);                                     // nm holds the old table now and frees it, after the synchronise
    c->D = nd;
    c->dict_cap = need;
    return LEON_OK;
}

// leon_dna_encode_batch's upload of the caller's bases while the device already packs and resolves the groups that have
// arrived.  The caller's memory is pageable: one hipMemcpy from it runs at 11-12 GB/s here (the runtime stages it through
// ONE thread), a fifth of what PCIe carries.  So the staging is done here, by a few threads: each takes the next 16 MiB
// piece of the byte range, copies it into one of its two pinned buffers and sends that to the device on its own stream.
struct Upload {
    static constexpr uint64_t kPiece = kStagePiece;             // (staging.h; 3 threads reach PCIe's 52-56 GB/s, more only take CPU time from the dictionary
                                                                //  chain: 6 threads 1 079 ms per step, 3 threads 910)
    std::atomic<uint64_t> bytes_done{0};                       // bases [0, bytes_done) of the batch are in HBM
    std::atomic<int> failed{0};                                // 1: a copy failed
    std::atomic<int> cancel{0};                                // set by the caller when the batch has failed: stop copying
    std::atomic<uint64_t> next_piece{0};
    std::vector<std::atomic<uint8_t>> piece_done;
    std::mutex mu;
    uint64_t prefix = 0, n_bytes = 0;
    std::vector<std::thread> th;
    explicit Upload(uint64_t bytes) : piece_done((bytes + kPiece - 1) / kPiece), n_bytes(bytes) { for (auto& f : piece_done) f.store(0); }
    void publish(uint64_t piece) {
        piece_done[piece].store(1, std::memory_order_release);
        std::lock_guard<std::mutex> g(mu);
        while (prefix < piece_done.size() && piece_done[prefix].load(std::memory_order_acquire)) prefix++;
        bytes_done.store(std::min(n_bytes, prefix * kPiece), std::memory_order_release);
    }
    ~Upload() { for (auto& t : th) if (t.joinable()) t.join(); }
};
int ensure_resolve_bufs(leon_dna_ctx* c, uint64_t n, uint64_t W) {
    HIPCHK(c, c->status.ensure(n));
    HIPCHK(c, c->hit_pos.ensure(n * 4)); HIPCHK(c, c->hit_slot.ensure(n * 4));
    HIPCHK(c, c->cand_pos.ensure(n * 4)); HIPCHK(c, c->cand_slot.ensure(n * 4));
    HIPCHK(c, c->anchor_pos.ensure(n * 4)); HIPCHK(c, c->anchor_addr.ensure(n * 4));
    HIPCHK(c, c->flags.ensure(n)); HIPCHK(c, c->sort_key.ensure(n * 8));
    HIPCHK(c, c->ins_flag.ensure(W * 4)); HIPCHK(c, c->rank.ensure(W * 4));
    HIPCHK(c, c->ulist0.ensure(W * 4)); HIPCHK(c, c->ulist1.ensure(W * 4));
    return LEON_OK;
}
// The walk's path cache: a 64-byte bucket per ~8 solid k-mers (the bloom's size says how many), at most 2^27 = 8 GiB; 0: none.  Not for a job of
// three ranks or more: the walkers of one genome region are spread over all ranks' slices, a rank's cache would cost as much as it saves.
uint64_t walk_cache_buckets(const leon_dna_ctx* c) {
    uint64_t buckets = 1024;
    while (buckets < c->cfg.bloom_tai / 12 / 8 && buckets < (1ull << 27)) buckets <<= 1;
    return c->B.n_hash == 7 && c->shard_world <= 2 ? buckets : 0;
}

float ms_since(std::chrono::steady_clock::time_point t) { return (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
// the time inside event pairs [e0, e1)
float pairs_ms(const EventList& ev, uint32_t e0, uint32_t e1) {
    float t = 0;
    for (uint32_t e = e0; e < e1; e++) { float v = 0; (void)hipEventElapsedTime(&v, ev[2 * e], ev[2 * e + 1]); t += v; }
    return t;
}

}  // namespace

// the context's stream, events, bloom and first buffers (leon_dna_ctx_create; what fails here is reported as a call without a context)
static int ctx_init(leon_dna_ctx* c, const leon_dna_cfg* cfg) {
    DEVCHK(hipSetDevice(c->device));
    DEVCHK(hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking));
    DEVCHK(c->h_rb.ensure(4096, 4096));
    DEVCHK(c->ev.ensure(12));
    // BloomCacheCoherent / BloomContainer geometry
    uint64_t blk = 1ull << cfg->bloom_block_nbits;
    uint64_t tai = cfg->bloom_tai + 2 * blk;
    c->bloom_nchar = 1 + tai / 8;
    if ((tai & (tai - 1)) == 0) tai--;
    uint64_t reduced = tai - 2 * blk;
    DEVCHK(c->d_bloom.exactly(c->bloom_nchar + 16));
    DEVCHK(hipMemsetAsync(c->d_bloom.p, 0, c->bloom_nchar + 16, c->stream));
    uint16_t rv16[256];
    for (uint32_t i = 0; i < 256; i++) rv16[i] = (uint16_t)((cfg->random_values ? cfg->random_values[i] : splitmix_rv(i)) & 0xFFFF);
    DEVCHK(c->d_rv16.exactly(sizeof(rv16)));
    DEVCHK(hipMemcpy(c->d_rv16.p, rv16, sizeof(rv16), hipMemcpyHostToDevice));
    uint32_t k = cfg->kmer_size;
    c->B.bits = c->d_bloom.as<uint8_t>(); c->B.reduced_tai = reduced; c->B.mod_magic = ~0ull / reduced; c->B.seed0 = hash_seed0();
    c->B.k = k; c->B.n_hash = cfg->bloom_n_hash; c->B.block_mask = (uint32_t)(blk - 1);
    DEVCHK(c->d_nkeys.exactly(8));
    DEVCHK(hipMemset(c->d_nkeys.p, 0, 8));
    DEVCHK(c->counters.ensure(64));
    DEVCHK(c->errflag.ensure(16));
    DEVCHK(hipMemsetAsync(c->errflag.p, 0, 16, c->stream));
    DEVCHK(c->wbits.ensure((1ull << WBITS_LOG2) / 8));
    DEVCHK(c->pbits.ensure((1ull << WBITS_LOG2) / 8));
    if (const char* e = getenv("LEON_FBITS_LOG2")) {          // measurement override: size of the final-key filter
        const int v = atoi(e);
        if (v >= 12 && v <= (int)FBITS_LOG2_MAX) c->fbits_log2 = (uint32_t)v;
    }
    DEVCHK(c->fbits.ensure((1ull << c->fbits_log2) / 8));
    DEVCHK(hipMemsetAsync(c->fbits.p, 0, (1ull << c->fbits_log2) / 8, c->stream));
    DEVCHK(hipStreamSynchronize(c->stream));
    return LEON_OK;
}

extern "C" {
int leon_dna_abi_version(void) { return LEON_DNA_ABI_VERSION; }

const char* leon_last_error(const leon_dna_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int leon_dna_ctx_create(const leon_dna_cfg* cfg, leon_dna_ctx** out) {
    if (!cfg || !out) return dev_fail(LEON_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(leon_dna_cfg)) return dev_fail(LEON_E_INVALID, "leon_dna_cfg.struct_size mismatch");
    if (cfg->kmer_size < 3 || cfg->kmer_size > 63)
        return dev_fail(LEON_E_INVALID, "kmer_size must be in 3..63 (one 64-bit word below 32, two words from 32 to 63)");
    if (cfg->reads_per_block == 0) return dev_fail(LEON_E_INVALID, "reads_per_block must be > 0");
    if (cfg->bloom_n_hash < 1 || cfg->bloom_n_hash > 10) return dev_fail(LEON_E_INVALID, "bloom_n_hash must be in 1..10");
    if (cfg->bloom_block_nbits < 4 || cfg->bloom_block_nbits > 16)
        return dev_fail(LEON_E_INVALID, "bloom_block_nbits must be in 4..16");
    {   // BloomNeighborCoherent's modulus tai' - 2 * blk must stay positive (bloom_tai = 0 makes tai a power of two, tai' = tai - 1
        // < 2 * blk), and an absurd size is refused here rather than by hipMalloc
        const uint64_t blk0 = 1ull << cfg->bloom_block_nbits;
        uint64_t tai0 = cfg->bloom_tai + 2 * blk0;
        if ((tai0 & (tai0 - 1)) == 0) tai0--;
        if (tai0 <= 2 * blk0 || cfg->bloom_tai > (1ull << 46)) return dev_fail(LEON_E_INVALID, "bloom_tai out of range (1 .. 2^46 bits)");
    }
    if ((cfg->flags & LEON_F_DICT_PIECES) && (cfg->flags & LEON_F_DICT_ON_DEVICE))
        return dev_fail(LEON_E_INVALID, "LEON_F_DICT_PIECES and LEON_F_DICT_ON_DEVICE exclude each other");
    if (cfg->dict_piece_anchors && !(cfg->flags & LEON_F_DICT_PIECES)) return dev_fail(LEON_E_INVALID, "dict_piece_anchors needs LEON_F_DICT_PIECES");
    if (cfg->dict_piece_anchors > kDictPieceAnchorsMax) return dev_fail(LEON_E_INVALID, "dict_piece_anchors must be in 1..2^20 (0 = 1024)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return dev_fail(LEON_E_NO_DEVICE, "no HIP device: the DNA encode path has no CPU fallback");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return dev_fail(LEON_E_INVALID, "device_id out of range");
    leon_dna_ctx* c = new leon_dna_ctx();
    c->cfg = *cfg;
    c->cfg.random_values = nullptr;
    if (c->cfg.resolve_window == 0) c->cfg.resolve_window = 1ull << 21;     // (2^20 until the look-ups got cheaper: 174 -> 168 ms per 100 M reads, profiles/r4_minimizer_filter.txt)
    c->device = cfg->device_id;
    if (int rc = ctx_init(c, cfg)) { leon_dna_ctx_destroy(c); return rc; }
    c->anchor_worker.reset(new AnchorDictWorker(cfg->kmer_size));
    *out = c;
    return LEON_OK;
}

void leon_dna_ctx_destroy(leon_dna_ctx* c) {
    if (!c) return;
    c->anchor_worker.reset();                                 // the dictionary chain's thread stops first
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

// ------------------------------------------------------------------------------------------------ bloom
int leon_dna_bloom_nbytes(const leon_dna_ctx* c, uint64_t* n) {
    if (!c || !n) return LEON_E_INVALID;
    *n = c->bloom_nchar;
    return LEON_OK;
}
int leon_dna_bloom_upload(leon_dna_ctx* c, const uint8_t* bits, uint64_t n) {
    if (!c || !bits) return LEON_E_INVALID;
    if (n != c->bloom_nchar) return fail(c, LEON_E_INVALID, "bloom_upload: size differs from leon_dna_bloom_nbytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, staged_h2d(c->device, c->d_bloom.p, bits, n));
    return LEON_OK;
}
int leon_dna_bloom_download(leon_dna_ctx* c, uint8_t* bits, uint64_t n) {
    if (!c || !bits) return LEON_E_INVALID;
    if (n != c->bloom_nchar) return fail(c, LEON_E_INVALID, "bloom_download: size differs from leon_dna_bloom_nbytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, staged_d2h(c->device, bits, c->d_bloom.p, n));
    return LEON_OK;
}
int leon_dna_bloom_clear(leon_dna_ctx* c) {
    if (!c) return LEON_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->d_bloom.p, 0, c->bloom_nchar + 16, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LEON_OK;
}
int leon_dna_bloom_insert_device(leon_dna_ctx* c, const uint64_t* d_kmers, uint64_t n) {
    if (!c || (!d_kmers && n)) return LEON_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    launch_bloom_insert(c->stream, c->B, c->rv16(), d_kmers, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LEON_OK;
}
int leon_dna_bloom_insert(leon_dna_ctx* c, const uint64_t* kmers, uint64_t n) {
    if (!c || (!kmers && n)) return LEON_E_INVALID;
    if (!n) return LEON_OK;
    HIPCHK(c, hipSetDevice(c->device));
    OwnBuf tmp;
    const uint64_t bytes = n * 8 * kmer_words(c->cfg.kmer_size);
    HIPCHK(c, tmp.ensure(bytes));
    HIPCHK(c, hipMemcpy(tmp.p, kmers, bytes, hipMemcpyHostToDevice));
    return leon_dna_bloom_insert_device(c, tmp.as<uint64_t>(), n);
}
int leon_dna_bloom_device_ptr(leon_dna_ctx* c, void** p, uint64_t* n) {
    if (!c || !p || !n) return LEON_E_INVALID;
    *p = c->d_bloom.p; *n = c->bloom_nchar;
    return LEON_OK;
}
int leon_dna_bloom_upload_device(leon_dna_ctx* c, const uint8_t* d_bits, uint64_t n) {
    if (!c || !d_bits) return LEON_E_INVALID;
    if (n != c->bloom_nchar) return fail(c, LEON_E_INVALID, "bloom_upload_device: size differs from leon_dna_bloom_nbytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->d_bloom.p, d_bits, n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LEON_OK;
}
int leon_dna_bloom_download_device(leon_dna_ctx* c, uint8_t* d_bits, uint64_t n) {
    if (!c || !d_bits) return LEON_E_INVALID;
    if (n != c->bloom_nchar) return fail(c, LEON_E_INVALID, "bloom_download_device: size differs from leon_dna_bloom_nbytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(d_bits, c->d_bloom.p, n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LEON_OK;
}
static int bloom_query(leon_dna_ctx* c, const uint64_t* kmers, uint64_t n, int mode, uint8_t* out) {
    if (!c || ((!kmers || !out) && n)) return LEON_E_INVALID;
    if (!n) return LEON_OK;
    HIPCHK(c, hipSetDevice(c->device));
    OwnBuf dk, dout;
    const uint64_t bytes = n * 8 * kmer_words(c->cfg.kmer_size);
    HIPCHK(c, dk.ensure(bytes));
    HIPCHK(c, dout.ensure(n));
    HIPCHK(c, hipMemcpy(dk.p, kmers, bytes, hipMemcpyHostToDevice));
    launch_bloom_query(c->stream, c->B, c->rv16(), dk.as<uint64_t>(), n, mode, dout.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout.p, n, hipMemcpyDeviceToHost));
    return LEON_OK;
}
int leon_dna_bloom_contains4(leon_dna_ctx* c, const uint64_t* kmers, uint64_t n, int right, uint8_t* out) {
    return bloom_query(c, kmers, n, right ? 2 : 1, out);
}
int leon_dna_bloom_contains(leon_dna_ctx* c, const uint64_t* kmers, uint64_t n, uint8_t* out) {
    return bloom_query(c, kmers, n, 0, out);
}

// ------------------------------------------------------------------------------------------------ encode
// reads [0, group_end(a)) are packed (and, through the host entry point, uploaded) together: the first resolution window
// alone, so that the device and the dictionary chain start at once, then groups of 8 windows
// (the first window itself is short -- first_window() reads -- so that the first anchors reach the host chain, the longest
// single piece of a step, a few milliseconds after the call starts; the result does not depend on where windows end)
static uint64_t first_window(uint64_t window) { return std::min<uint64_t>(window, 1ull << 17); }
static uint64_t group_end(uint64_t a, uint64_t n, uint64_t window) {
    if (a == 0) return std::min(n, first_window(window));
    // (resident input used to pack everything that was left in one go: 9.6 ms at 100 M reads between the first window and the
    // second, during which the dictionary chain ran out of the first window's anchors and idled)
    return std::min(n, a + 8 * std::min<uint64_t>(window, 1ull << 20));
}

namespace {

// The encode path's knobs -- measurement aids and test hooks: any values give the same bytes --, read at the start of every batch
// (the tests change them inside one process).
struct EncodeKnobs {
    uint32_t rounds_ahead, rounds_max;   // LEON_RESOLVE_ROUNDS=a[:m]: fixpoint rounds launched ahead (1..32, default 3) / at most (..62, default 9)
    uint32_t chain_chunk;                // LEON_CHAIN_CHUNK: reads per k_chain_seq (<= 2^CHAIN_LOG2): the tests' way onto the chunk-by-chunk path
    bool xch_lookups, walk_cache;        // LEON_XCH_LOOKUPS=0: a job's window look-ups not shared out among its ranks; LEON_WALK_CACHE=0: no path cache
    long walk_cache_log2, walk_hop_log2; // LEON_WALK_CACHE_LOG2: log2 of the cache's buckets (10..31, else sized by the bloom); LEON_WALK_HOP_LOG2 (1..8, 4)
    bool trace_step, trace_resolve, trace_chain;   // LEON_TRACE_STEP / _RESOLVE / _CHAIN, on stderr: host time of a batch's first milestones /
                                                   //   what a read costs k_lookup_cand by its outcome / the sequential passes
};
long env_num(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
EncodeKnobs read_encode_knobs() {
    const char* rounds = getenv("LEON_RESOLVE_ROUNDS");
    const long ahead = env_num("LEON_RESOLVE_ROUNDS", 0), most = rounds && strchr(rounds, ':') ? atol(strchr(rounds, ':') + 1) : 0;
    const long chunk = env_num("LEON_CHAIN_CHUNK", 0), hop = env_num("LEON_WALK_HOP_LOG2", 4);
    EncodeKnobs K{};
    K.rounds_ahead = ahead >= 1 && ahead <= 32 ? (uint32_t)ahead : 3u;
    K.rounds_max = std::max<uint32_t>(K.rounds_ahead, most >= 1 && most <= 62 ? (uint32_t)most : 9u);
    K.chain_chunk = chunk >= 1 && chunk <= (1l << CHAIN_LOG2) ? (uint32_t)chunk : 1u << CHAIN_LOG2;
    K.xch_lookups = env_num("LEON_XCH_LOOKUPS", 1) != 0; K.walk_cache = env_num("LEON_WALK_CACHE", 1) != 0;
    K.walk_cache_log2 = env_num("LEON_WALK_CACHE_LOG2", 0); K.walk_hop_log2 = hop >= 1 && hop <= 8 ? hop : 4;
    K.trace_step = getenv("LEON_TRACE_STEP"); K.trace_resolve = getenv("LEON_TRACE_RESOLVE"); K.trace_chain = getenv("LEON_TRACE_CHAIN");
    return K;
}

// One call of leon_dna_encode_batch on its way through the stages (each returns LEON_OK or the batch's error), and what they hand one another.
struct EncodeBatch {
    leon_dna_ctx* const c;
    const uint8_t* const d_bases; const uint64_t* const d_off; const uint64_t n, first_read_index; const leon_block_sink sink; void* const user;
    Upload* const up; const uint64_t* const up_off;   // the host entry point's upload of the bases and the caller's offsets (nullptr: device input)
    const uint64_t* const walk_keys = c->walk_keys;   // leon_dna_debug_walk_order's: THIS batch only, whatever becomes of it
    const EncodeKnobs knobs = read_encode_knobs();
    const std::chrono::steady_clock::time_point t_enter = std::chrono::steady_clock::now();
    const hipStream_t s = c->stream;
    const uint32_t rpb = c->cfg.reads_per_block, k = c->cfg.kmer_size;
    uint64_t n_blocks = 0, off_first = 0, off_last = 0, n_slots = 0, W = 0, KW = 0;   // W: reads per resolution window, KW: words per anchor k-mer
    ReadsDev R{}; ResolveDev V{};
    uint64_t packed_upto = 0; uint32_t n_pack_ev = 0;   // the pack: reads [0, packed_upto), between n_pack_ev pairs of c->pack_ev
    // the anchor resolution: list counts ([0], [1]) and lists, the counts of a window's rounds, LEON_TRACE_RESOLVE's counts
    static constexpr uint32_t kRoundsMore = 2, kHist = 64;
    uint32_t* counters = nullptr; uint32_t* lists[2] = {nullptr, nullptr}; uint32_t* d_hist = nullptr; unsigned long long* d_trace = nullptr;
    size_t scan_tmp = 0;                     // work space of the window scans
    struct Pending { int buf = -1; uint64_t n = 0; } pending;      // a window's new anchors on their way to pinned memory
    int anchor_buf = 0; bool share_lookups = false;
    uint32_t hint = 0;                       // grid-size hint of a window's first round (any size is correct: grid-stride loops)
    uint32_t n_chain_ev = 0;                 // pairs of c->chain_ev around the sequential passes
    float lk_call_ms = 0, lk_emul_ms = 0;    // the shared look-ups' gathers / emulated runs
    // this rank's share and its walk; divided by anchor: where the slices begin, where each rank's reads begin, a slice's words by destination
    Share sh{}; uint64_t nl_bases = 0; bool by_anchor = false;
    WalkCache wc{nullptr, 0, 28, 0};
    std::vector<uint64_t> slice_at, rank_r0, send_counts, send_at; size_t scan_n = 0;
    void mark(const char* what) const {
        if (knobs.trace_step) fprintf(stderr, "[leon step] %-34s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enter).count());
    }
    float ms(int a, int b) const { float v = 0; (void)hipEventElapsedTime(&v, c->ev[a], c->ev[b]); return v; }
    // ---- everything that may fail before the stream changes: the offsets checked, the reads' 32-base slots counted and scanned,
    // the first window's reads packed, the resolution's buffers ----
    int start() {
        c->stats = leon_dna_stats{}; c->walk_keys = nullptr;
        HIPCHK(c, hipMemcpyAsync(c->rb() + 0, d_off, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(c->rb() + 1, d_off + n, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, spin_sync(s));
        off_first = c->rb()[0]; off_last = c->rb()[1];
        if (off_last < off_first) return fail(c, LEON_E_INVALID, "offsets are not monotonic");
        n_blocks = (n + rpb - 1) / rpb;
        HIPCHK(c, hipEventRecord(c->ev[0], s));
        // ---- pack ----
        if (int rc = check_offsets(c, d_off, n, "a read is longer than 2^31 bases", &n_slots, true)) return rc;
        mark("offsets checked, slots scanned");
        if (int rc = ensure_pack_bufs(c, n, n_slots)) return rc;
        HIPCHK(c, hipMemsetAsync(c->packed.as<uint32_t>() + n_slots * 2, 0, 64, s));
        if (int rc = pack_next_group()) return rc;               // the first window's reads
        HIPCHK(c, hipEventRecord(c->ev[1], s));
        // ---- anchor resolution: its buffers ----
        R = reads_view(c, d_off, n);
        W = std::min<uint64_t>(c->cfg.resolve_window, n);
        if (int rc = ensure_resolve_bufs(c, n, W)) return rc;
        V.status = c->status.as<uint8_t>(); V.hit_pos = c->hit_pos.as<uint32_t>(); V.hit_slot = c->hit_slot.as<uint32_t>();
        V.cand_pos = c->cand_pos.as<uint32_t>(); V.cand_slot = c->cand_slot.as<uint32_t>();
        V.anchor_pos = c->anchor_pos.as<int32_t>(); V.anchor_addr = c->anchor_addr.as<uint32_t>(); V.flags = c->flags.as<uint8_t>();
        V.sort_key = c->sort_key.as<uint64_t>(); V.ins_flag = c->ins_flag.as<uint32_t>();
        counters = c->counters.as<uint32_t>(); lists[0] = c->ulist0.as<uint32_t>(); lists[1] = c->ulist1.as<uint32_t>();
        HIPCHK(c, prim::ExclusiveSum(nullptr, scan_tmp, V.ins_flag, c->rank.as<uint32_t>(), W, s));
        return ensure_cub(c, scan_tmp);
    }
    // The first resolution window's reads are packed first, later groups right before their first window: the host thread that codes the
    // dictionary stream (the longest single piece of a step) gets its first anchors ~25 ms earlier, and with host input the upload of a
    // group overlaps the resolution of the groups before it.
    int pack_next_group() {
        const uint64_t a = packed_upto, b = group_end(a, n, c->cfg.resolve_window);
        if (up) {
            // the group's last base, from the caller's offsets: checked before it is waited for (whatever the entries between
            // the group boundaries are, the device checks them one by one and refuses the batch)
            const uint64_t want = up_off[b];
            if (want < up_off[0] || want > up_off[n] || want < up_off[a]) return fail(c, LEON_E_INVALID, "offsets are not monotonic");
            while (up->bytes_done.load(std::memory_order_acquire) < want - up_off[0] && !up->failed.load()) std::this_thread::yield();
            if (up->failed.load()) return fail(c, LEON_E_HIP, "upload of the read bases failed");
        }
        HIPCHK(c, c->pack_ev.ensure(2 * (size_t)(n_pack_ev + 1)));
        HIPCHK(c, hipEventRecord(c->pack_ev[2 * n_pack_ev], s));
        launch_pack(s, d_bases, d_off + a, c->slot_off.as<uint64_t>() + a, b - a, c->packed.as<uint32_t>(), c->nmask.as<uint32_t>(),
                    c->rlen.as<uint32_t>() + a, c->ncount.as<uint32_t>() + a);
        HIPCHK(c, hipEventRecord(c->pack_ev[2 * n_pack_ev + 1], s));
        n_pack_ev++;
        packed_upto = b;
        return LEON_OK;
    }
    // Host round trips: a wait costs 20-40 us and the stage used to make ~6 per window (580 per 100 M reads: the window's first count,
    // one per fixpoint round, the insert count, the new anchors' copy).  Now two: the rounds are launched AHEAD of their counts -- the
    // kernels take the list lengths from device memory, an empty list costs a launch that finds nothing to do -- three at once, then two
    // at a time for the few windows that need more, with every round's count copied to a small history that comes back with the
    // next wait; and a window's new anchors travel to pinned memory behind the kernels and are handed to the dictionary chain at
    // the NEXT window's first wait (the first window's at once: the chain, the longest piece of a step, starts with them).
    int resolve() {
        KW = kmer_words(k);
        HIPCHK(c, c->round_hist.ensure(kHist * 4)); d_hist = c->round_hist.as<uint32_t>();
        for (auto& b : c->h_anchor) HIPCHK(c, b.ensure(W * 8 * KW + 64, W * 8 * KW + 64));
        if (knobs.trace_resolve) { HIPCHK(c, c->resolve_trace.ensure(12 * 8)); d_trace = c->resolve_trace.as<unsigned long long>(); HIPCHK(c, hipMemsetAsync(d_trace, 0, 12 * 8, s)); }
        // the look-ups shared out among the ranks of a job (leon_dna_set_gather; LEON_XCH_EMULATE plays the other ranks)
        share_lookups = c->shard_world > 1 && knobs.xch_lookups && ((c->xch_mode == LEON_XCH_BY_ANCHOR && c->gather_fn) || c->xch_mode == LEON_XCH_EMULATE);
        hint = (uint32_t)std::min<uint64_t>(W, 1u << 20);
        for (uint64_t w0 = 0, w1 = 0; w0 < n; w0 = w1) {
            w1 = std::min(n, w0 + (w0 == 0 ? first_window(W) : W));
            if (int rc = resolve_window(w0, w1)) return rc;
            while (w1 < n && packed_upto < std::min(n, w1 + W)) { if (int rc = pack_next_group()) return rc; }   // the next window's reads
            c->stats.resolve_windows++;
        }
        if (pending.buf >= 0) { HIPCHK(c, spin_sync(s)); hand_over(); }
        if (knobs.trace_resolve) {
            unsigned long long t[12];
            HIPCHK(c, hipMemcpy(t, d_trace, sizeof t, hipMemcpyDeviceToHost));
            const char* cls[3] = {"found an anchor of the dictionary", "went on to propose its own", "no anchor at all"};
            for (int j = 0; j < 3; j++)
                if (t[4 * j]) fprintf(stderr, "[leon resolve] k_lookup_cand, reads that %-34s: %10llu reads, per read %.1f filter probes, %.1f dictionary probes behind a filter maybe, %.1f k-mers through the bloom\n",
                                      cls[j], t[4 * j], (double)t[4 * j + 1] / t[4 * j], (double)t[4 * j + 2] / t[4 * j], (double)t[4 * j + 3] / t[4 * j]);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev[2], s));
        mark("resolution launched to its end");
        return LEON_OK;
    }
    // one window [w0, w1): look-ups, fixpoint rounds (and the sequential pass behind them), the settled anchors to the dictionary
    int resolve_window(uint64_t w0, uint64_t w1) {
        if (int rc = dict_reserve(c, c->n_keys + (w1 - w0))) return rc;
        HIPCHK(c, hipMemsetAsync(counters, 0, 8, s));
        HIPCHK(c, hipMemsetAsync(c->wbits.p, 0, (1ull << WBITS_LOG2) / 8, s));
        HIPCHK(c, hipMemsetAsync(c->pbits.p, 0, (1ull << WBITS_LOG2) / 8, s));
        if (!share_lookups) launch_lookup_cand(s, R, c->B, c->rv16(), c->D, V, w0, w1, first_read_index, lists[0], counters, d_trace);
        else if (int rc = look_up_shared(w0, w1)) return rc;
        HIPCHK(c, hipMemcpyAsync(d_hist, counters, 4, hipMemcpyDeviceToDevice, s));         // hist[0]: the window's unresolved reads
        uint32_t cnt0 = 0;
        if (int rc = fixpoint_rounds(w0, w1, cnt0)) return rc;
        hint = std::max<uint32_t>(2 * cnt0, 4096);
        if (cnt0 > 0) { if (int rc = settle(w0, w1)) return rc; }
        launch_finalize_reads(s, R, c->D, V, w0, w1);
        return LEON_OK;
    }
    // The window's look-ups divided among the ranks (leon_dna_set_gather): rank r takes the r-th run of P reads, everybody learns what
    // everybody found from ONE all-gather of a word per read -- the caller's -- and makes the other runs' results its own (k_lookup_apply):
    // every rank's dictionary goes on holding every proposal, as if it had looked everything up.
    int look_up_shared(uint64_t w0, uint64_t w1) {
        const uint32_t Wn = c->shard_world; const uint64_t P = (w1 - w0 + Wn - 1) / Wn;
        auto run_of = [&](uint32_t r, uint64_t& a, uint64_t& b) { a = std::min(w1, w0 + (uint64_t)r * P); b = std::min(w1, a + P); };
        HIPCHK(c, c->xch_res.ensure((uint64_t)Wn * P * 8)); uint64_t* xres = c->xch_res.as<uint64_t>();
        uint64_t s0 = 0, s1 = 0; run_of(c->shard_rank, s0, s1);
        launch_lookup_cand(s, R, c->B, c->rv16(), c->D, V, s0, s1, first_read_index, lists[0], counters, d_trace, xres, w0, false);
        HIPCHK(c, hipStreamSynchronize(s));
        const auto t_l0 = std::chrono::steady_clock::now();
        if (c->xch_mode == LEON_XCH_BY_ANCHOR) {
            if (c->gather_fn(c->gather_user, xres, P * 8, Wn)) return fail(c, LEON_E_STATE, "the gather callback returned non-zero");
            HIPCHK(c, hipSetDevice(c->device));               // (the callback may have changed the thread's device)
            lk_call_ms += ms_since(t_l0);
        } else {                                              // no other rank present: their runs computed here, leaving nothing but their words
            for (uint32_t r = 0; r < Wn; r++) {
                if (r == c->shard_rank) continue;
                uint64_t a = 0, b = 0; run_of(r, a, b);
                launch_lookup_cand(s, R, c->B, c->rv16(), c->D, V, a, b, first_read_index, lists[0], counters, nullptr, xres, w0, true);
            }
            HIPCHK(c, hipStreamSynchronize(s));
            lk_emul_ms += ms_since(t_l0);
        }
        launch_lookup_apply(s, R, c->D, V, w0, w1, s0, s1, first_read_index, xres, lists[0], counters);
        return LEON_OK;
    }
    // The rounds are NOT asked to finish: their count is the longest chain of reads each waiting for the one before it, which no valid
    // input bounds (reads in genome-position order make one chain of a whole window).  After knobs.rounds_ahead rounds -- more while the
    // list keeps halving, knobs.rounds_max at most -- what is left goes, in read order, through the exact sequential pass (chain_tail).
    // cnt0: the reads the window's look-ups left unresolved.
    int fixpoint_rounds(uint64_t w0, uint64_t w1, uint32_t& cnt0) {
        int cur = 0;
        uint32_t n_hist = 1;
        bool first_wait = true;
        // (Fewer rounds ahead for a file whose last window left the sequential pass most of its list -- position-sorted reads -- were
        // measured and are slower: rounds 2 and 3 settle the reads that contain round 1's inserters, 15 M of a sorted 100 M-read
        // file's, in 180 ms; the sequential pass takes 18 ns for each of them.  1 929 ms against 1 838 for the stage.)
        for (uint32_t ahead = knobs.rounds_ahead;; ahead = kRoundsMore) {
            for (uint32_t r = 0; r < ahead && n_hist < kHist; r++) {
                const int nxt = cur ^ 1;
                const uint32_t h = std::max<uint32_t>(hint >> (2 * (n_hist - 1) < 31 ? 2 * (n_hist - 1) : 31), 4096);
                HIPCHK(c, hipMemsetAsync(counters + nxt, 0, 4, s));
                launch_check(s, R, c->D, V, first_read_index, lists[cur], counters + cur, h, lists[nxt], counters + nxt);
                HIPCHK(c, hipMemcpyAsync(d_hist + n_hist, counters + nxt, 4, hipMemcpyDeviceToDevice, s));
                launch_reset_tent(s, c->D, V, lists[cur], counters + cur, h);
                launch_propose(s, c->D, V, first_read_index, lists[nxt], counters + nxt, h);
                cur = nxt; n_hist++;
            }
            HIPCHK(c, hipMemcpyAsync(c->rb() + 8, d_hist, n_hist * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(c->rb() + 1, c->D.err, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, spin_sync(s));
            if (first_wait) { hand_over(); first_wait = false; }
            if (const int derr = (int)(uint32_t)c->rb()[1]) {
                HIPCHK(c, hipMemsetAsync(c->D.err, 0, 4, s));
                return fail(c, LEON_E_STATE, derr == 2 ? "the look-ups gathered from the other ranks do not fit this rank's reads or dictionary (were all ranks fed the same batches?)"
                                                       : "anchor dictionary: a two-word key stayed half-written (a stalled wave); batch abandoned");
            }
            const uint32_t* hist = reinterpret_cast<const uint32_t*>(c->rb() + 8);
            cnt0 = hist[0];
            for (uint32_t r = 1; r < n_hist; r++)
                if (hist[r - 1] > 0 && hist[r] >= hist[r - 1]) return fail(c, LEON_E_STATE, "anchor resolution made no progress (internal error)");
            const uint32_t cnt = hist[n_hist - 1];
            // more rounds only while they pay: the list at least halved in the last round and the budget is not spent
            const bool halving = n_hist >= 2 && 2ull * hist[n_hist - 1] <= hist[n_hist - 2];
            if (cnt == 0 || !halving || n_hist - 1 >= knobs.rounds_max || n_hist + kRoundsMore > kHist) {
                for (uint32_t r = 1; r < n_hist; r++) if (hist[r - 1] > 0) c->stats.resolve_rounds++;
                return cnt ? chain_tail(cnt, w0, w1, lists[cur ^ 1]) : LEON_OK;
            }
        }
    }
    // ---- the exact sequential pass behind the rounds (dna_kernels.hip, k_chain_*): the `left` reads the rounds did not settle ----
    int chain_tail(uint32_t left, uint64_t w0, uint64_t w1, uint32_t* clist) {
        HIPCHK(c, c->chain_ev.ensure(2 * (size_t)(n_chain_ev + 1)));
        HIPCHK(c, hipEventRecord(c->chain_ev[2 * n_chain_ev], s));
        // in read order: flags over the window, their ranks (a read's chain index), the compacted list
        uint32_t* rank = c->rank.as<uint32_t>();
        launch_chain_flags(s, V, w0, w1, V.ins_flag);
        HIPCHK(c, prim::ExclusiveSum(c->cub_tmp.p, scan_tmp, V.ins_flag, rank, w1 - w0, s));
        launch_chain_compact(s, V, w0, w1, rank, clist);
        const uint32_t CH = knobs.chain_chunk;
        unsigned long long* d_ctrace = nullptr;
        if (knobs.trace_chain) { HIPCHK(c, c->chain_trace.ensure(8 * 8)); d_ctrace = c->chain_trace.as<unsigned long long>(); HIPCHK(c, hipMemsetAsync(d_ctrace, 0, 8 * 8, s)); }
        for (uint32_t c0 = 0; c0 < left; c0 += CH) {
            const uint32_t nc = std::min(CH, left - c0), nG = (nc + 63) / 64;
            // a later chunk: tent still names reads of the chunk before (settled now) -- cleared, and what is left proposes again
            if (c0) launch_chain_repropose(s, c->D, V, first_read_index, clist + (c0 - CH), left - (c0 - CH), clist + c0, left - c0);
            HIPCHK(c, c->chain_cnt.ensure((uint64_t)nc * 4)); HIPCHK(c, c->chain_own.ensure((uint64_t)nc * 4));
            HIPCHK(c, c->chain_ins.ensure(((uint64_t)nG + 1) * 8)); HIPCHK(c, c->chain_rows.ensure(((uint64_t)nG + 1) * 8));
            HIPCHK(c, c->chain_dep.ensure((uint64_t)nc * 8)); HIPCHK(c, c->chain_xdep.ensure((uint64_t)nc * 8));
            HIPCHK(c, c->chain_om.ensure((uint64_t)nG * 64 * 8)); HIPCHK(c, c->chain_late.ensure((uint64_t)nG * 8));
            uint64_t* rows = c->chain_rows.as<uint64_t>();
            uint32_t* cnt = c->chain_cnt.as<uint32_t>(); uint32_t* own = c->chain_own.as<uint32_t>();
            unsigned long long* om = c->chain_om.as<unsigned long long>(); unsigned long long* late = c->chain_late.as<unsigned long long>();
            unsigned long long* dep = c->chain_dep.as<unsigned long long>(); unsigned long long* xdep = c->chain_xdep.as<unsigned long long>();
            size_t rows_tmp = 0;
            HIPCHK(c, prim::ExclusiveSum(nullptr, rows_tmp, rows, rows, nG + 1, s));
            if (rows_tmp > c->cub_tmp.cap) { HIPCHK(c, hipStreamSynchronize(s)); if (int rc = ensure_cub(c, std::max(rows_tmp, scan_tmp))) return rc; }
            launch_chain_prep(s, false, R, c->D, V, first_read_index, w0, clist + c0, nc, c0, rank, cnt, own, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            launch_chain_tables(s, cnt, own, nc, rows, om, late);
            HIPCHK(c, prim::ExclusiveSum(c->cub_tmp.p, rows_tmp, rows, rows, nG + 1, s));
            HIPCHK(c, hipMemcpyAsync(c->rb() + 0, rows + nG, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(c, spin_sync(s));
            const uint64_t total_rows = c->rb()[0];
            HIPCHK(c, c->chain_ent.ensure(std::max<uint64_t>(total_rows, 1) * 64 * 4)); uint32_t* ent = c->chain_ent.as<uint32_t>();
            launch_chain_prep(s, true, R, c->D, V, first_read_index, w0, clist + c0, nc, c0, rank, cnt, own, rows, ent, om, late, dep, xdep);
            if (launch_chain_seq(s, nc, cnt, own, dep, xdep, rows, ent, c->chain_ins.as<unsigned long long>(), d_ctrace))
                return fail(c, LEON_E_HIP, "the sequential resolution pass could not be launched (its LDS request was refused)");
            launch_chain_apply(s, c->D, V, first_read_index, clist + c0, nc, c->chain_ins.as<unsigned long long>(), k);
            HIPCHK(c, hipGetLastError());
        }
        // (the rounds end with every tent they touched cleared; so must this: a tent that still named a settled read would block whoever
        // proposes the key in a later window)
        { const uint32_t c_last = (left - 1) / CH * CH; launch_chain_repropose(s, c->D, V, first_read_index, clist + c_last, left - c_last, nullptr, 0); }
        HIPCHK(c, hipEventRecord(c->chain_ev[2 * n_chain_ev + 1], s));
        n_chain_ev++;
        c->stats.resolve_chain_reads += left; c->stats.resolve_chain_windows++;
        if (knobs.trace_chain) {
            unsigned long long t[8];
            HIPCHK(c, hipStreamSynchronize(s));
            HIPCHK(c, hipMemcpy(t, d_ctrace, sizeof t, hipMemcpyDeviceToHost));
            float cms = 0; (void)hipEventElapsedTime(&cms, c->chain_ev[2 * n_chain_ev - 2], c->chain_ev[2 * n_chain_ev - 1]);
            fprintf(stderr, "[leon chain] window [%llu, %llu): %u reads left by the rounds; %llu steps of 64, %.2f ballot iterations and %.1f entry rows per step, %llu inserters; %.2f ms; per step the settler waited %.0f (tester: %.0f), settled + published %.0f ticks of s_memtime\n",
                    (unsigned long long)w0, (unsigned long long)w1, left, t[0], t[0] ? (double)t[1] / t[0] : 0.0, t[0] ? (double)t[2] / t[0] : 0.0, t[3], cms,
                    t[0] ? (double)t[4] / t[0] : 0.0, t[0] ? (double)t[5] / t[0] : 0.0, t[0] ? (double)t[6] / t[0] : 0.0);
        }
        return LEON_OK;
    }
    // the window's settled reads: their final positions, the new anchors' addresses and k-mers, and those k-mers on their way to the
    // host thread coding the dictionary stream
    int settle(uint64_t w0, uint64_t w1) {
        launch_final_pos(s, R, c->D, V, w0, w1, first_read_index);
        launch_ins_flags(s, V, w0, w1);
        HIPCHK(c, prim::ExclusiveSum(c->cub_tmp.p, scan_tmp, V.ins_flag, c->rank.as<uint32_t>(), w1 - w0, s));
        HIPCHK(c, hipMemcpyAsync(c->rb() + 0, c->rank.as<uint32_t>() + (w1 - w0 - 1), 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(c->rb() + 1, V.ins_flag + (w1 - w0 - 1), 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(c->rb() + 2, c->d_nkeys.p, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, spin_sync(s));
        const uint64_t n_new = (uint64_t)(uint32_t)c->rb()[0] + (uint32_t)c->rb()[1];   // the window's last read's rank + its flag
        c->n_keys = c->rb()[2];
        if (c->n_anchors + n_new > 0xFFFFFFFFull) return fail(c, LEON_E_OVERFLOW, "more than 2^32 anchors");
        if ((c->n_anchors + n_new) * 8 * KW > c->anchor_kmers.cap) {      // grow, keeping what is there
            OwnBuf nb;
            HIPCHK(c, nb.ensure(std::max<uint64_t>((c->n_anchors + n_new) * 2, 1024) * 8 * KW));
            if (c->n_anchors) HIPCHK(c, hipMemcpyAsync(nb.p, c->anchor_kmers.p, c->n_anchors * 8 * KW, hipMemcpyDeviceToDevice, s));
            HIPCHK(c, hipStreamSynchronize(s));
            c->anchor_kmers.swap(nb);                                // nb now holds the old buffer and releases it
        }
        launch_assign_addr(s, c->D, V, w0, w1, c->rank.as<uint32_t>(), c->n_anchors, c->anchor_kmers.as<uint64_t>(), k);
        if (n_new && c->shard_rank == 0 && !(c->cfg.flags & (LEON_F_DICT_ON_DEVICE | LEON_F_DICT_PIECES))) {   // the window's new anchors, for the host thread coding the dictionary stream
            HIPCHK(c, hipMemcpyAsync(c->h_anchor[anchor_buf].p, c->anchor_kmers.as<uint64_t>() + c->n_anchors * KW, n_new * 8 * KW, hipMemcpyDeviceToHost, s));
            pending.buf = anchor_buf; pending.n = n_new;
            anchor_buf ^= 1;
            if (w0 == 0) {
                HIPCHK(c, spin_sync(s));
                hand_over();
                mark("first window's anchors to the chain");
            }
        }
        c->n_anchors += n_new;
        return LEON_OK;
    }
    void hand_over() {                              // (called right after a wait: the copy has landed)
        if (pending.buf < 0) return;
        const uint64_t* const landed = c->h_anchor[pending.buf].as<uint64_t>();
        std::vector<uint64_t> fresh(landed, landed + pending.n * KW);
        c->anchor_worker->push(std::move(fresh));
        pending.buf = -1;
    }
    // ---- this rank's share of the batch: a contiguous range of whole blocks (all of it when not sharded) ----
    int take_share() {
        sh = share_of(c, n);
        uint64_t off_r0 = off_first, off_r1 = off_last;
        if (c->shard_world > 1) {
            HIPCHK(c, hipMemcpy(&off_r0, d_off + sh.r0, 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(&off_r1, d_off + sh.r0 + sh.nl, 8, hipMemcpyDeviceToHost));
        }
        nl_bases = off_r1 - off_r0;
        R.ev_origin = sh.r0;
        c->stats.n_reads = sh.nl; c->stats.n_bases = nl_bases; c->stats.n_blocks = sh.nbl; c->stats.n_anchors = c->n_anchors;
        c->last_n = n; c->last_bases = nl_bases; c->last_d_bases = d_bases; c->last_d_off = d_off;
        by_anchor = c->shard_world > 1 && c->xch_mode != LEON_XCH_OFF;
        return LEON_OK;
    }
    // ---- walk: the events of the share's reads, walked here (walk_share) or divided among the ranks by anchor (walk_by_anchor) ----
    int walk() {
        HIPCHK(c, c->events.ensure(nl_bases + 16));
        HIPCHK(c, hipMemsetAsync(c->events.p, 0, nl_bases + 16, s));
        start_walk_cache();
        HIPCHK(c, c->perm.ensure(n * 4));
        launch_iota(s, c->perm.as<uint32_t>(), n);
        return by_anchor ? walk_by_anchor() : walk_share();
    }
    // the walk's path cache (walk_cache_buckets), at most an eighth of the free device memory; EMPTY again at every batch -- what a batch's
    // walkers learn from the bloom is shared among THEM, a later batch (or a bench step) starts cold
    void start_walk_cache() {
        uint64_t buckets = knobs.walk_cache ? walk_cache_buckets(c) : 0;
        if (!buckets) return;
        if (knobs.walk_cache_log2 >= 10 && knobs.walk_cache_log2 <= 31) buckets = 1ull << knobs.walk_cache_log2;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) while (buckets > 1024 && buckets * 64 > c->wcache.cap && buckets * 64 > free_b / 8) buckets >>= 1;
        if (c->wcache.ensure(buckets * 64) != hipSuccess) { (void)hipGetLastError(); return; }
        wc.slots = c->wcache.as<uint64_t>(); wc.bucket_mask = buckets - 1; wc.hop_shift = 32 - knobs.walk_hop_log2;
        launch_walk_cache_init(s, wc, k);
    }
    int walk_share() {
        // ---- sort the share's reads by (anchor address, strand) ----
        const uint64_t r0 = sh.r0, nl = sh.nl;
        HIPCHK(c, c->sort_key2.ensure(nl * 8)); HIPCHK(c, c->perm2.ensure(nl * 4));
        // (measurement hook: another order of the reads in the walk changes which lanes share bloom sectors, never the bytes --
        // events are indexed by read position)
        const uint64_t* walk_key = walk_keys ? walk_keys + r0 : V.sort_key + r0;
        const unsigned key_bits = walk_keys ? 48u : 33u;
        auto sort = [&](void* t, size_t& b) { return prim::SortPairs(t, b, walk_key, c->sort_key2.as<uint64_t>(), c->perm.as<uint32_t>() + r0, c->perm2.as<uint32_t>(), nl, 0, key_bits, s); };
        if (int rc = run_prim(c, sort)) return rc;
        HIPCHK(c, hipEventRecord(c->ev[3], s));
        // ---- walk ----
        HIPCHK(c, hipEventRecord(c->ev[4], s));
        launch_walk(s, R, c->B, c->rv16(), V.anchor_pos, V.flags, c->perm2.as<uint32_t>(), nl, c->events.as<uint8_t>(), nullptr, wc);
        HIPCHK(c, hipEventRecord(c->ev[5], s));
        c->stats.walk_launches = 1; c->stats.walk_reads = nl;
        return LEON_OK;
    }
    // ---- the walk divided by anchor (leon_dna_set_exchange): ALL of the batch's reads sorted by anchor address, cut into `world` slices of
    // equal size; this rank walks its slice into a buffer of its own and what it found goes to the ranks that code the reads' blocks, as
    // (place in that rank's event buffer, byte) words grouped by destination ----
    int walk_by_anchor() {
        const uint32_t Wd = c->shard_world, me = c->shard_rank;
        if (Wd + 2 > 4096 / 8) return fail(c, LEON_E_INVALID, "set_exchange: world too large");
        if (int rc = cut_slices()) return rc;
        HIPCHK(c, hipMemsetAsync(c->errflag.as<int>() + 1, 0, 4, s));
        const auto t_x0 = std::chrono::steady_clock::now();     // (ms_exchange: everything of the division that is not the slice's walk itself)
        if (int rc = walk_slice(me, true)) return rc;
        HIPCHK(c, hipStreamSynchronize(s));
        float walk_own = 0; (void)hipEventElapsedTime(&walk_own, c->ev[4], c->ev[5]);
        c->stats.xch_words_sent = send_at[Wd];
        if (c->xch_mode == LEON_XCH_BY_ANCHOR) {
            const uint64_t* d_recv = nullptr; uint64_t recv_total = 0;
            const auto t_call = std::chrono::steady_clock::now();
            if (c->xch_fn(c->xch_user, c->xch_send.as<uint64_t>(), send_counts.data(), Wd, &d_recv, &recv_total))
                return fail(c, LEON_E_STATE, "the exchange callback returned non-zero");
            c->stats.ms_exchange_call = ms_since(t_call);
            if (recv_total && !d_recv) return fail(c, LEON_E_STATE, "the exchange callback returned no buffer");
            c->stats.xch_words_received = recv_total;
            HIPCHK(c, hipSetDevice(c->device));                   // (the callback may have changed the thread's device)
            launch_ev_scatter(s, d_recv, recv_total, c->events.as<uint8_t>(), nl_bases, c->errflag.as<int>() + 1);
            HIPCHK(c, hipStreamSynchronize(s));                   // the caller's buffer is free again when this call returns
            c->stats.ms_exchange = ms_since(t_x0) - walk_own;
        } else {
            // no other rank present: this context plays them all, one slice after the other, and keeps what is meant for its own rank
            auto keep_own = [&] { launch_ev_scatter(s, c->xch_send.as<uint64_t>() + send_at[me], send_counts[me], c->events.as<uint8_t>(), nl_bases, c->errflag.as<int>() + 1);
                                  c->stats.xch_words_received += send_counts[me]; };
            keep_own();
            HIPCHK(c, hipStreamSynchronize(s));
            c->stats.ms_exchange = ms_since(t_x0) - walk_own;
            const auto t_e0 = std::chrono::steady_clock::now();
            for (uint32_t sl = 0; sl < Wd; sl++) {
                if (sl == me) continue;
                if (int rc = walk_slice(sl, false)) return rc;
                keep_own();
            }
            HIPCHK(c, hipStreamSynchronize(s));
            c->stats.ms_emulated = ms_since(t_e0);
        }
        // (the window look-ups shared out among the ranks, earlier in this call: their gathers and, emulated, the other ranks' runs)
        c->stats.ms_exchange_call += lk_call_ms; c->stats.ms_exchange += lk_call_ms; c->stats.ms_gather_call = lk_call_ms;
        c->stats.ms_emulated += lk_emul_ms; c->stats.ms_emulated_lookups = lk_emul_ms;
        HIPCHK(c, hipEventRecord(c->ev[9], s));                  // the symbols stage begins here
        int xerr = 0;
        HIPCHK(c, hipMemcpy(&xerr, c->errflag.as<int>() + 1, 4, hipMemcpyDeviceToHost));
        if (xerr) return fail(c, LEON_E_STATE, "the exchange delivered a word that lies outside this rank's blocks");
        return LEON_OK;
    }
    // the batch's reads sorted by anchor and cut into slices: slice_at, rank_r0, and the work space of the slices' scans
    int cut_slices() {
        const uint32_t Wd = c->shard_world;
        HIPCHK(c, c->sort_key2.ensure(n * 8)); HIPCHK(c, c->perm2.ensure(n * 4));
        auto sort = [&](void* t, size_t& b) { return prim::SortPairs(t, b, V.sort_key, c->sort_key2.as<uint64_t>(), c->perm.as<uint32_t>(), c->perm2.as<uint32_t>(), n, 0, 33, s); };
        if (int rc = run_prim(c, sort)) return rc;
        unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(c->counters.as<uint32_t>() + 10);
        launch_lower_bound(s, c->sort_key2.as<uint64_t>(), n, 1ull << 32, d_cnt);            // reads without an anchor sort last: nothing to walk
        HIPCHK(c, hipMemcpyAsync(c->rb() + 0, d_cnt, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, spin_sync(s));
        const uint64_t n_anch = c->rb()[0];
        // the slices: equal WEIGHT (a read 1, an anchor group's first read SLICE_GROUP_WEIGHT more), the same cuts on every rank
        HIPCHK(c, c->xch_slot.ensure(n * 4)); HIPCHK(c, c->xch_off.ensure((n + 1) * 8));
        HIPCHK(c, prim::ExclusiveSum(nullptr, scan_n, c->xch_off.as<uint64_t>(), c->xch_off.as<uint64_t>(), n + 1, s));
        if (int rc = ensure_cub(c, scan_n)) return rc;
        HIPCHK(c, c->xch_split.ensure((Wd + 1) * 8));
        launch_slice_weights(s, c->sort_key2.as<uint64_t>(), n_anch, c->xch_off.as<uint64_t>());
        HIPCHK(c, prim::ExclusiveSum(c->cub_tmp.p, scan_n, c->xch_off.as<uint64_t>(), c->xch_off.as<uint64_t>(), n_anch + 1, s));
        launch_slice_splits(s, c->xch_off.as<uint64_t>(), n_anch, Wd, c->xch_split.as<unsigned long long>());
        HIPCHK(c, hipMemcpyAsync(c->rb() + 0, c->xch_split.p, (Wd + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->ev[3], s));
        HIPCHK(c, spin_sync(s));
        slice_at.assign(c->rb(), c->rb() + Wd + 1);
        // where each rank's reads begin in file order, for the words' grouping
        rank_r0.resize(Wd + 1);
        for (uint32_t d = 0; d <= Wd; d++) rank_r0[d] = std::min<uint64_t>(n, block_start(n_blocks, d, Wd) * rpb);
        send_counts.assign(Wd, 0);
        send_at.assign(Wd + 1, 0);
        return LEON_OK;
    }
    // one slice: walked into xch_events, its words formed in xch_send (grouped by destination; send_at[d] = where rank d's begin)
    int walk_slice(uint32_t sl, bool timed) {
        const uint32_t Wd = c->shard_world;
        const uint64_t s0 = slice_at[sl], s1 = slice_at[sl + 1], ns = s1 - s0;
        const uint32_t* slice = c->perm2.as<uint32_t>() + s0;
        HIPCHK(c, c->xch_evoff.ensure((ns + 1) * 8));
        uint64_t* evoff = c->xch_evoff.as<uint64_t>();
        HIPCHK(c, hipMemsetAsync(c->xch_slot.p, 0xFF, n * 4, s));
        launch_slice_reads(s, R, slice, ns, evoff, c->xch_slot.as<uint32_t>());
        if (int rc = run_prim(c, [&](void* t, size_t& b) { return prim::ExclusiveSum(t, b, evoff, evoff, ns + 1, s); })) return rc;
        HIPCHK(c, hipMemcpyAsync(c->rb() + 0, evoff + ns, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, spin_sync(s));
        const uint64_t slice_bases = c->rb()[0];
        HIPCHK(c, c->xch_events.ensure(slice_bases + 16));
        HIPCHK(c, hipMemsetAsync(c->xch_events.p, 0, slice_bases + 16, s));
        if (timed) HIPCHK(c, hipEventRecord(c->ev[4], s));
        launch_walk(s, R, c->B, c->rv16(), V.anchor_pos, V.flags, slice, ns, c->xch_events.as<uint8_t>(), evoff, wc);
        if (timed) { HIPCHK(c, hipEventRecord(c->ev[5], s)); c->stats.walk_launches = 1; c->stats.walk_reads = ns; }
        launch_ev_words(s, R, c->xch_slot.as<uint32_t>(), evoff, c->xch_events.as<uint8_t>(), n, rpb, n_blocks, Wd, c->xch_off.as<uint64_t>(), nullptr);
        HIPCHK(c, prim::ExclusiveSum(c->cub_tmp.p, scan_n, c->xch_off.as<uint64_t>(), c->xch_off.as<uint64_t>(), n + 1, s));
        for (uint32_t d = 0; d <= Wd; d++) HIPCHK(c, hipMemcpyAsync(c->rb() + 1 + d, c->xch_off.as<uint64_t>() + rank_r0[d], 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, spin_sync(s));
        for (uint32_t d = 0; d <= Wd; d++) send_at[d] = c->rb()[1 + d];
        for (uint32_t d = 0; d < Wd; d++) send_counts[d] = send_at[d + 1] - send_at[d];
        HIPCHK(c, c->xch_send.ensure(send_at[Wd] * 8 + 64));
        launch_ev_words(s, R, c->xch_slot.as<uint32_t>(), evoff, c->xch_events.as<uint8_t>(), n, rpb, n_blocks, Wd, c->xch_off.as<uint64_t>(),
                        c->xch_send.as<uint64_t>());
        HIPCHK(c, hipGetLastError());
        return LEON_OK;
    }
    // ---- symbols, range coder, D2H: the share's blocks ----
    int code(CodedBlocks& out) {
        HIPCHK(c, c->prev.ensure(n * 8));
        HIPCHK(c, c->nerr.ensure(sh.nl * 8));                      // (two words per read: error positions, chunks that hold events)
        launch_prev_anchored(s, V.anchor_pos, n, rpb, sh.lb0, sh.nbl, c->prev.as<int64_t>());
        auto symbols = [&](uint8_t* syms) {
            launch_symbols(s, R, V.anchor_pos, V.anchor_addr, V.flags, c->prev.as<int64_t>(), c->events.as<uint8_t>(), sh.r0, sh.nl,
                           c->sym_off.as<uint64_t>(), c->nerr.as<uint32_t>(), syms);
        };
        return code_blocks(c, sh, symbols, SMALL_SIZES_DNA, true, "read", out);
    }
    // The batch's end, on each of its three ways out: the stats up to event last_ev -- 2: nothing of the batch is this rank's to walk or code;
    // 5: the rank's slice walked and delivered, none of the blocks is its own; 8: `out` coded --, the blocks to the sink, the stream moved on.
    int finish(int last_ev, const CodedBlocks* out = nullptr) {
        leon_dna_stats& st = c->stats;
        const float pack2 = pairs_ms(c->pack_ev, 1, n_pack_ev);   // the part of the pack stage that ran inside the resolution loop
        st.ms_pack = ms(0, 1) + pack2; st.ms_resolve = ms(1, 2) - pack2; st.ms_resolve_chain = pairs_ms(c->chain_ev, 0, n_chain_ev);
        if (last_ev >= 5) { st.ms_sort = ms(2, 3); st.ms_walk = ms(4, 5); }
        if (out) {
            st.n_symbols = out->n_syms; st.payload_bytes = out->payload_bytes;
            st.ms_symbols = by_anchor ? ms(9, 6) : ms(5, 6); st.ms_rangecoder = ms(6, 7); st.ms_d2h = ms(7, 8);
        }
        st.ms_total = ms(0, last_ev);
        if (out) { if (int rc = deliver_blocks(c, *out, sh, n, c->dna.next_block, sink, user)) return rc; }
        c->dna.advance(n, rpb);
        c->poisoned = false;
        return LEON_OK;
    }
};

}  // namespace

static int encode_batch_impl(leon_dna_ctx* c, const uint8_t* d_bases, const uint64_t* d_off, uint64_t n,
                             uint64_t first_read_index, leon_block_sink sink, void* user, Upload* up, const uint64_t* up_off) {
    if (!c) return LEON_E_INVALID;
    if (c->finished) return fail(c, LEON_E_STATE, "encode_batch after finish");
    if (int rc = c->dna.follows(c, first_read_index, n, "stream")) return rc;
    if (n == 0) return LEON_OK;
    if (!d_bases || !d_off || !sink) return fail(c, LEON_E_INVALID, "null argument");
    if (n > 0xFFFFFFF0ull) return fail(c, LEON_E_INVALID, "more than 2^32 reads in one batch");
    HIPCHK(c, hipSetDevice(c->device));
    EncodeBatch B{c, d_bases, d_off, n, first_read_index, sink, user, up, up_off};
    if (int rc = B.start()) return rc;
    c->poisoned = true;             // from here on the dictionary and the dictionary stream change: cleared on success
    if (int rc = B.resolve()) return rc;
    if (int rc = B.take_share()) return rc;
    if (B.sh.nl == 0 && !(B.by_anchor && c->xch_mode == LEON_XCH_BY_ANCHOR)) {   // nothing of this batch is ours to encode (and nobody waits for our slice)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return B.finish(2);
    }
    if (int rc = B.walk()) return rc;
    if (B.sh.nl == 0) return B.finish(5);                        // our slice is delivered; no block of the batch is ours to code
    CodedBlocks out;                                             // (the share's blocks: symbols, range coder, D2H)
    if (int rc = B.code(out)) return rc;
    return B.finish(8, &out);
}

// A batch that fails before it has touched the stream (bad arguments, bad offsets, call order) leaves the context as it was.
// One that fails later -- a HIP error, an internal bound, the sink -- leaves the dictionary, the dictionary-stream thread
// and the caller's block sequence part-way through the batch: the context is poisoned and every call on the stream
// returns LEON_E_STATE until leon_dna_reset_stream starts a new one.
static int encode_batch_guarded(leon_dna_ctx* c, const uint8_t* d_bases, const uint64_t* d_off, uint64_t n,
                                uint64_t first_read_index, leon_block_sink sink, void* user, Upload* up, const uint64_t* up_off = nullptr) {
    if (!c) return LEON_E_INVALID;
    if (c->poisoned) return refuse_poisoned(c);
    if (c->dc.pc.slots) (void)hipStreamSynchronize(c->stream);   // a context that goes back to encoding gives the decoder's table (up to 40 % of the HBM) back first,
    c->dc.release();                                          // and the decode calls' buffers
    return note_poisoned(c, encode_batch_impl(c, d_bases, d_off, n, first_read_index, sink, user, up, up_off));
}

int leon_dna_encode_batch_device(leon_dna_ctx* c, const uint8_t* d_bases, const uint64_t* d_off, uint64_t n,
                                 uint64_t first_read_index, leon_block_sink sink, void* user) {
    return encode_batch_guarded(c, d_bases, d_off, n, first_read_index, sink, user, nullptr);
}

int leon_dna_encode_batch(leon_dna_ctx* c, const uint8_t* bases, const uint64_t* off, uint64_t n, uint64_t first_read_index,
                          leon_block_sink sink, void* user) {
    if (!c) return LEON_E_INVALID;
    if (n == 0) return leon_dna_encode_batch_device(c, nullptr, nullptr, 0, first_read_index, sink, user);
    if (!bases || !off) return fail(c, LEON_E_INVALID, "null argument");
    if (off[n] < off[0]) return fail(c, LEON_E_INVALID, "offsets are not monotonic");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t nb = off[n] - off[0];
    HIPCHK(c, c->in_bases.ensure(nb + 64));
    HIPCHK(c, c->in_off.ensure((n + 1) * 8));
    // offsets first (rebased on the device so that they index the device copy of the bases), then the bases group by
    // group on an uploader thread while the device already works on the groups that have arrived
    HIPCHK(c, staged_h2d(c->device, c->in_off.p, off, (n + 1) * 8));      // (800 MB at 100 M reads: 73 ms as one hipMemcpy from pageable memory, 15 staged)
    if (off[0]) {
        launch_rebase_offsets(c->stream, c->in_off.as<uint64_t>(), n + 1, off[0]);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    Upload up(nb);
    const int dev = c->device;
    uint8_t* dst = c->in_bases.as<uint8_t>();
    const uint8_t* src = bases + off[0];
    const uint32_t n_workers = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(stage_threads(), up.piece_done.size()));
    for (uint32_t w = 0; w < n_workers; w++)
        up.th.emplace_back([&up, dev, dst, src, nb] {
            StageLane L(dev);
            uint64_t held[2] = {~0ull, ~0ull};                  // the piece a buffer's copy in flight belongs to
            bool ok = L.ok;
            for (uint32_t turn = 0; ok && !up.cancel.load(); turn ^= 1) {
                if (held[turn] != ~0ull) {                     // the buffer's previous piece has landed: publish it before refilling
                    if (hipEventSynchronize(L.ev[turn]) != hipSuccess) { ok = false; break; }
                    up.publish(held[turn]); held[turn] = ~0ull;
                }
                const uint64_t piece = up.next_piece.fetch_add(1);
                if (piece >= up.piece_done.size()) break;
                const uint64_t a = piece * Upload::kPiece, m = std::min<uint64_t>(Upload::kPiece, nb - a);
                memcpy(L.buf[turn], src + a, m);
                if (hipMemcpyAsync(dst + a, L.buf[turn], m, hipMemcpyHostToDevice, L.st) != hipSuccess || hipEventRecord(L.ev[turn], L.st) != hipSuccess) { ok = false; break; }
                held[turn] = piece;
            }
            for (int t = 0; t < 2 && ok; t++)
                if (held[t] != ~0ull) { if (hipEventSynchronize(L.ev[t]) != hipSuccess) ok = false; else up.publish(held[t]); }
            if (!ok && !up.cancel.load()) up.failed.store(1);
        });
    static const bool trace_up = getenv("LEON_TRACE_UPLOAD") != nullptr;      // measurement aid: when the last base reached HBM
    const auto t_up0 = std::chrono::steady_clock::now();
    std::thread watcher;
    if (trace_up) watcher = std::thread([&up, nb, t_up0] {
        while (up.bytes_done.load() < nb && !up.failed.load() && !up.cancel.load()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up0).count();
        fprintf(stderr, "[leon upload] %.1f MB in %.1f ms = %.1f GB/s\n", nb / 1e6, ms, nb / 1e6 / ms);
    });
    const int rc = encode_batch_guarded(c, dst, c->in_off.as<uint64_t>(), n, first_read_index, sink, user, &up, off);
    if (rc != LEON_OK) up.cancel.store(1);
    for (auto& t : up.th) t.join();
    if (watcher.joinable()) watcher.join();
    return rc;
}

// Sizes every per-batch device buffer for a batch of up to max_reads reads / max_bases bases before the first batch arrives
// (a host calls it while it is still parsing): the first leon_dna_encode_batch of a process then allocates nothing large, and
// does not wait for the driver to wipe memory another stage has just returned.  Symbol counts are an
// estimate (40 per read); whatever turns out larger is grown on demand as before.
int leon_dna_reserve(leon_dna_ctx* c, uint64_t max_reads, uint64_t max_bases) {
    if (!c) return LEON_E_INVALID;
    if (max_reads == 0) return LEON_OK;
    if (max_reads > 0xFFFFFFF0ull) return fail(c, LEON_E_INVALID, "more than 2^32 reads in one batch");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = max_reads, rpb = c->cfg.reads_per_block, nbl = (n + rpb - 1) / rpb;
    const uint64_t n_slots = max_bases / 32 + n, W = std::min<uint64_t>(c->cfg.resolve_window, n), est_syms = 40 * n;
    HIPCHK(c, c->slot_off.ensure((n + 1) * 8));
    if (int rc = ensure_pack_bufs(c, n, n_slots)) return rc;
    if (int rc = ensure_resolve_bufs(c, n, W)) return rc;
    HIPCHK(c, c->sort_key2.ensure(n * 8)); HIPCHK(c, c->perm.ensure(n * 4)); HIPCHK(c, c->perm2.ensure(n * 4));
    HIPCHK(c, c->events.ensure(max_bases + 16));
    HIPCHK(c, c->prev.ensure(n * 8)); HIPCHK(c, c->sym_off.ensure((n + 1) * 8)); HIPCHK(c, c->nerr.ensure(n * 8));
    HIPCHK(c, c->syms.ensure(est_syms * 2 + 256));
    if (int rc = ensure_block_bufs(c, nbl)) return rc;
    if (int rc = ensure_rc_bufs(c, nbl, est_syms)) return rc;
    HIPCHK(c, c->payload.ensure(max_bases / 12 + 4096));
    size_t t1 = 0, t2 = 0, t3 = 0;                               // the scans' and the sort's work space
    HIPCHK(c, prim::ExclusiveSum(nullptr, t1, c->slot_off.as<uint64_t>(), c->slot_off.as<uint64_t>(), n + 1, c->stream));
    HIPCHK(c, prim::SortPairs(nullptr, t2, c->sort_key.as<uint64_t>(), c->sort_key2.as<uint64_t>(), c->perm.as<uint32_t>(), c->perm2.as<uint32_t>(),
                                                 n, 0, 33, c->stream));
    HIPCHK(c, prim::ExclusiveSum(nullptr, t3, c->ins_flag.as<uint32_t>(), c->rank.as<uint32_t>(), W, c->stream));
    if (int rc = ensure_cub(c, std::max(t1, std::max(t2, t3)))) return rc;
    HIPCHK(c, c->h_payload.ensure(max_bases / 12 + 4096, max_bases / 12 + 4096));
    // the walk's path cache (as a batch sizes it: walk_cache_buckets; best effort)
    size_t free_b = 0, total_b = 0;
    if (const uint64_t buckets = walk_cache_buckets(c))
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && buckets * 64 <= free_b / 8 && c->wcache.ensure(buckets * 64) != hipSuccess) (void)hipGetLastError();
    // the dictionary: one anchor per ~6 reads of a 30x read set; it grows (rehash) if the data want more
    if (int rc = dict_reserve(c, c->n_keys + n / 6 + 1024)) return rc;
    if ((n / 6) * 8 * kmer_words(c->cfg.kmer_size) > c->anchor_kmers.cap && c->n_anchors == 0) HIPCHK(c, c->anchor_kmers.ensure((n / 6) * 8 * kmer_words(c->cfg.kmer_size)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    leon_device_trim();                                          // (the k-mer counter's parked buffers go back now that this context's exist: kmer_kernels.hip)
    return LEON_OK;
}

// ---- the anchor dictionary in independently coded pieces (dict_pieces_code and the device calls: dict_kernels.hip) ----
int leon_dna_dict_pieces(leon_dna_ctx* c, const uint64_t** piece_off, uint64_t* n_pieces, uint32_t* piece_anchors) {
    if (!c || !piece_off || !n_pieces || !piece_anchors) return LEON_E_INVALID;
    if (!(c->cfg.flags & LEON_F_DICT_PIECES)) return fail(c, LEON_E_STATE, "leon_dna_dict_pieces: the context was created without LEON_F_DICT_PIECES");
    if (!c->finished || c->dict_piece_off.empty()) return fail(c, LEON_E_STATE, "leon_dna_dict_pieces must follow leon_dna_finish");
    *piece_off = c->dict_piece_off.data();
    *n_pieces = c->dict_piece_off.size() - 1;
    *piece_anchors = dict_piece_anchors(c->cfg.dict_piece_anchors);
    return LEON_OK;
}

// the dictionary stream coded on the device, into c->dict_device_out: in independent pieces (LEON_F_DICT_PIECES) ...
static int finish_in_pieces(leon_dna_ctx* c) {
    c->dict_piece_off.assign(1, 0);
    if (c->shard_rank != 0 || !c->n_anchors) return LEON_OK;    // the dictionary stream is rank 0's to write
    const uint32_t P = dict_piece_anchors(c->cfg.dict_piece_anchors);
    c->dict_piece_off.assign(dict_piece_count(c->n_anchors, P) + 1, 0);
    OwnBuf d_dst; std::string why;
    if (int rc = dict_pieces_code(c->stream, c->anchor_kmers.as<uint64_t>(), c->n_anchors, c->cfg.kmer_size, P, c->dict_piece_off.data(), d_dst, why)) {
        c->dict_piece_off.clear();
        return fail(c, rc, why);
    }
    c->dict_device_out.resize(c->dict_piece_off.back());
    if (!c->dict_device_out.empty()) HIPCHK(c, hipMemcpy(c->dict_device_out.data(), d_dst.p, c->dict_device_out.size(), hipMemcpyDeviceToHost));
    return LEON_OK;
}
// ... or as the one stream the host chain would have written, by k_rc_encode (LEON_F_DICT_ON_DEVICE)
static int finish_on_device(leon_dna_ctx* c) {
    if (c->shard_rank != 0) return LEON_OK;
    const uint64_t nsym = c->n_anchors * c->cfg.kmer_size, begin[2] = { 0, nsym };
    OwnBuf dsyms; RcStreamsDev D;
    HIPCHK(c, dsyms.ensure(nsym * 2 + 256));
    launch_anchor_symbols(c->stream, c->anchor_kmers.as<uint64_t>(), c->n_anchors, c->cfg.kmer_size, dsyms.as<uint8_t>());
    uint64_t sz = 0;
    if (int rc = D.code(c, dsyms.as<uint8_t>(), begin, 1, nsym, "dictionary stream: device range coder bound hit", &sz)) return rc;
    c->dict_device_out.resize(sz);
    if (sz) HIPCHK(c, hipMemcpy(c->dict_device_out.data(), D.out.p, sz, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_dna_finish(leon_dna_ctx* c, const uint8_t** payload, uint64_t* size, uint64_t* n_anchors) {
    if (!c || !payload || !size || !n_anchors) return LEON_E_INVALID;
    if (c->poisoned) return refuse_poisoned(c);
    auto t0 = std::chrono::steady_clock::now();
    const bool on_device = c->cfg.flags & (LEON_F_DICT_PIECES | LEON_F_DICT_ON_DEVICE);
    if (!on_device) c->anchor_worker->drain();
    else if (!c->finished) {
        c->dict_device_out.clear();
        HIPCHK(c, hipSetDevice(c->device));
        if (int rc = (c->cfg.flags & LEON_F_DICT_PIECES) ? finish_in_pieces(c) : finish_on_device(c)) return rc;
    }
    c->anchor_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!on_device) {
        if (getenv("LEON_TRACE_STEP")) fprintf(stderr, "[leon step] dictionary chain busy %.1f ms, of which %.1f ms waiting for its helpers' records\n",
                                               c->anchor_worker->busy_ms(), c->anchor_worker->starved_ms());
        if (!c->finished && c->shard_rank == 0) c->anchor_worker->coder().flush();
    }
    c->finished = true;
    *payload = on_device ? c->dict_device_out.data() : c->anchor_worker->coder().data();
    *size = on_device ? c->dict_device_out.size() : c->shard_rank == 0 ? c->anchor_worker->coder().size() : 0;   // the dictionary stream is rank 0's to write
    *n_anchors = c->n_anchors;
    return LEON_OK;
}

int leon_dna_debug_walk_order(leon_dna_ctx* c, const uint64_t* d_keys) {
    if (!c) return LEON_E_INVALID;
    c->walk_keys = d_keys;
    return LEON_OK;
}

int leon_dna_set_shard(leon_dna_ctx* c, uint32_t rank, uint32_t world) {
    if (!c) return LEON_E_INVALID;
    if (world == 0 || rank >= world) return fail(c, LEON_E_INVALID, "set_shard: need rank < world");
    if (c->dna.next_read) return fail(c, LEON_E_STATE, "set_shard must precede the first batch of a stream");
    c->shard_rank = rank; c->shard_world = world;
    return LEON_OK;
}

int leon_dna_set_exchange(leon_dna_ctx* c, uint32_t mode, leon_exchange_fn fn, void* user) {
    if (!c) return LEON_E_INVALID;
    if (mode > LEON_XCH_EMULATE) return fail(c, LEON_E_INVALID, "set_exchange: unknown mode");
    if (mode == LEON_XCH_BY_ANCHOR && !fn) return fail(c, LEON_E_INVALID, "set_exchange: LEON_XCH_BY_ANCHOR needs the exchange callback");
    if (c->dna.next_read) return fail(c, LEON_E_STATE, "set_exchange must precede the first batch of a stream");
    c->xch_mode = mode; c->xch_fn = fn; c->xch_user = user;
    return LEON_OK;
}

int leon_dna_set_gather(leon_dna_ctx* c, leon_gather_fn fn, void* user) {
    if (!c) return LEON_E_INVALID;
    if (c->dna.next_read) return fail(c, LEON_E_STATE, "set_gather must precede the first batch of a stream");
    c->gather_fn = fn; c->gather_user = user;
    return LEON_OK;
}

int leon_dna_reset_stream(leon_dna_ctx* c) {
    if (!c) return LEON_E_INVALID;
    static const bool trace_step = getenv("LEON_TRACE_STEP") != nullptr;
    const auto t_enter = std::chrono::steady_clock::now();
    struct Done { bool on; std::chrono::steady_clock::time_point t0; ~Done() { if (on) fprintf(stderr, "[leon step] %-34s %8.2f ms\n", "reset_stream", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); } } done{trace_step, t_enter};
    c->anchor_worker->reset();
    c->dict_piece_off.clear();
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, spin_sync(c->stream));
    HIPCHK(c, hipMemsetAsync(c->fbits.p, 0, (1ull << c->fbits_log2) / 8, c->stream));
    if (c->dict_cap) {
        HIPCHK(c, hipMemsetAsync(c->d_nkeys.p, 0, 8, c->stream));
        launch_dict_init(c->stream, c->D, c->dict_cap, kmer_words(c->cfg.kmer_size));
        HIPCHK(c, spin_sync(c->stream));
    }
    c->n_keys = 0; c->n_anchors = 0;
    c->dna = StreamCursor{}; c->hdr = StreamCursor{};
    c->finished = false; c->poisoned = false;
    c->last_n = 0; c->last_bases = 0; c->last_d_bases = c->last_d_off = nullptr;
    return LEON_OK;
}

int leon_dna_get_stats(const leon_dna_ctx* c, leon_dna_stats* out) {
    if (!c || !out) return LEON_E_INVALID;
    *out = c->stats;
    out->n_anchors = c->n_anchors;
    out->ms_anchor_wait = (float)c->anchor_wait_ms;
    out->ms_chain_busy = c->finished ? (float)c->anchor_worker->busy_ms() : 0.f;
    return LEON_OK;
}

// ------------------------------------------------------------------------------------------------ traces
int leon_dna_trace_anchors(leon_dna_ctx* c, int32_t* pos, uint32_t* addr, uint8_t* flags, uint64_t n) {
    if (!c) return LEON_E_INVALID;
    if (n != c->last_n) return fail(c, LEON_E_INVALID, "trace size differs from the last batch");
    HIPCHK(c, hipSetDevice(c->device));
    if (pos) HIPCHK(c, hipMemcpy(pos, c->anchor_pos.p, n * 4, hipMemcpyDeviceToHost));
    if (addr) HIPCHK(c, hipMemcpy(addr, c->anchor_addr.p, n * 4, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(c, hipMemcpy(flags, c->flags.p, n, hipMemcpyDeviceToHost));
    return LEON_OK;
}
int leon_dna_trace_events(leon_dna_ctx* c, uint8_t* events, uint64_t n_bases) {
    if (!c || !events) return LEON_E_INVALID;
    if (n_bases != c->last_bases) return fail(c, LEON_E_INVALID, "trace size differs from the last batch");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(events, c->events.p, n_bases, hipMemcpyDeviceToHost));
    return LEON_OK;
}
int leon_dna_anchor_kmers(leon_dna_ctx* c, uint64_t* kmers, uint64_t n) {
    if (!c || (!kmers && n)) return LEON_E_INVALID;
    if (n > c->n_anchors) return fail(c, LEON_E_INVALID, "more anchors requested than exist");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(kmers, c->anchor_kmers.p, n * 8 * kmer_words(c->cfg.kmer_size), hipMemcpyDeviceToHost));
    return LEON_OK;
}
}  // extern "C"
