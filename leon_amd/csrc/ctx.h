// ctx.h -- the context behind include/leon_dna.h's leon_dna_ctx and what the calls that take one share.  Each such call lives in the
// file of its kernels, like the stateless calls (device_call.h); capi.hip keeps the context's life and the encode path.
// Every member of the context that owns something releases it in its own destructor: leon_dna_ctx_destroy has no list to keep.
#pragma once
#include "../../include/leon_dna.h"
#include "kernels.h"
#include "host_rc.h"
#include "host_blocks.h"
#include "device_call.h"
#include <algorithm>
#include <functional>
#include <memory>
#include <vector>

namespace leon {
// pinned host memory: `want` bytes when it holds fewer than `need`
struct PinnedBuf : NoCopy {
    void* p = nullptr; size_t cap = 0;
    hipError_t release() { const hipError_t e = p ? hipHostFree(p) : hipSuccess; p = nullptr; cap = 0; return e; }
    hipError_t ensure(size_t need, size_t want) {
        if (need <= cap) return hipSuccess;
        if (const hipError_t e = release()) return e;
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    template <typename T> T* as() const { return (T*)p; }
    ~PinnedBuf() { (void)release(); }
};
// a list of events that grows on demand (pairs around the launches of a batch, a fixed set made at create)
struct EventList : NoCopy {
    std::vector<hipEvent_t> ev; const unsigned flags;
    explicit EventList(unsigned f = hipEventDefault) : flags(f) {}
    hipError_t ensure(size_t n) {
        for (hipEvent_t e; ev.size() < n; ev.push_back(e)) if (const hipError_t err = hipEventCreateWithFlags(&e, flags)) return err;
        return hipSuccess;
    }
    hipEvent_t operator[](size_t i) const { return ev[i]; }
    ~EventList() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
// the anchor dictionary's allocations; the kernels' view of them is a DictDev (two-word keys keep tent inside the slots: `tent` stays empty)
struct DictMem {
    OwnBuf slots, tent, addr;
    void swap(DictMem& o) { slots.swap(o.slots); tent.swap(o.tent); addr.swap(o.addr); }
};
// where an ordered stream of batches stands (the DNA stream, the header stream)
struct StreamCursor {
    uint64_t next_read = 0, next_block = 0; bool partial_seen = false;
    // LEON_OK when a batch of n reads that begins at first_read_index goes on from here; `stream`: "stream" / "header stream"
    int follows(leon_dna_ctx* c, uint64_t first_read_index, uint64_t n, const char* stream) const;
    void advance(uint64_t n, uint64_t rpb) { next_read += n; next_block += (n + rpb - 1) / rpb; if (n % rpb) partial_seen = true; }
};
// small launches: the blocks' chains on host cores (host_blocks.h, rc_kernels.hip), fed by the device's modelers chunk by chunk
struct HostChains {
    OwnBuf recs[2], recoff, state;
    PinnedBuf h_recs;                                            // the records of a launch
    CallStream copy_stream;
    EventList ev{hipEventDisableTiming};                         // per chunk: modelled, copied
    std::vector<HostBlockCoder> coders;
};
// the decoder (decode_kernels.hip): its path cache lives as long as the bloom it was learnt from, a call's large buffers from call
// to call (a fresh 15 GB allocation waits 0.3 s for the driver to wipe it)
struct DecoderState {
    OwnBuf cache, out, pay, len, pool, scr;
    PathCache pc{}; bool filled = false;
    uint64_t bloom_fp = 0;                                       // fingerprint of the bloom bits the cache's entries were derived from
    void drop_cache() { cache.release(); pc = PathCache{}; filled = false; }
    void release() { drop_cache(); out.release(); pay.release(); len.release(); pool.release(); scr.release(); }
};
}  // namespace leon

// Members are destroyed in reverse order of declaration: the stream first, so that it goes last.
struct leon_dna_ctx {
    leon::CallStream stream;
    leon_dna_cfg cfg{};
    int device = 0;
    leon::PinnedBuf h_rb;                                        // pinned host words the short read-backs of a batch land in (spin_sync)
    std::string err;
    // bloom
    leon::OwnBuf d_bloom;
    uint64_t bloom_nchar = 0;
    leon::BloomDev B{};
    leon::OwnBuf d_rv16;
    // dictionary
    leon::DictMem dict_mem;
    leon::DictDev D{};
    uint64_t dict_cap = 0;
    uint64_t n_keys = 0;
    leon::OwnBuf d_nkeys;
    uint64_t n_anchors = 0;
    leon::OwnBuf anchor_kmers;
    std::unique_ptr<leon::AnchorDictWorker> anchor_worker;       // host thread coding the dictionary stream, fed per window
    double anchor_wait_ms = 0;
    std::vector<uint8_t> dict_device_out;        // LEON_F_DICT_ON_DEVICE: the stream coded by k_rc_encode; LEON_F_DICT_PIECES: the pieces back to back
    std::vector<uint64_t> dict_piece_off;        // LEON_F_DICT_PIECES: where each piece begins (n_pieces + 1 entries), from leon_dna_finish on
    // stream state
    leon::StreamCursor dna, hdr;                 // the DNA stream's and the header stream's own counters
    bool finished = false, poisoned = false;     // poisoned: a batch failed after it had started to change the stream: LEON_E_STATE until reset_stream
    uint32_t shard_rank = 0, shard_world = 1;    // leon_dna_set_shard
    uint32_t xch_mode = LEON_XCH_OFF;            // leon_dna_set_exchange: how the walk is divided among the ranks
    leon_exchange_fn xch_fn = nullptr; void* xch_user = nullptr;
    leon_gather_fn gather_fn = nullptr; void* gather_user = nullptr;   // leon_dna_set_gather: the look-ups of a window divided as well
    leon::OwnBuf xch_slot, xch_off, xch_evoff, xch_events, xch_send, xch_split, xch_res;
    leon::OwnBuf resolve_trace;
    leon::OwnBuf round_hist;                     // the counts of a window's fixpoint rounds, read back together
    leon::OwnBuf wcache;                         // the walk's path cache (dna_kernels.hip): cleared at every batch
    leon::OwnBuf chain_cnt, chain_own, chain_ins, chain_rows, chain_ent, chain_trace, chain_dep, chain_xdep, chain_om, chain_late;   // the sequential pass behind the rounds (k_chain_*)
    leon::EventList chain_ev;                    // pairs around the sequential passes of a batch
    leon::HostChains hb;
    leon::PinnedBuf h_anchor[2];                 // a window's new anchors on their way to the dictionary chain
    leon::OwnBuf hdr_first;
    const uint64_t* walk_keys = nullptr;         // leon_dna_debug_walk_order: the next batch's walk order (measurement hook)
    uint32_t fbits_log2 = leon::FBITS_LOG2_DEFAULT;
    // batch buffers
    leon::OwnBuf in_bases, in_off, slot_off, packed, nmask, rlen, ncount;
    leon::OwnBuf status, hit_pos, hit_slot, cand_pos, cand_slot, anchor_pos, anchor_addr, flags, sort_key, ins_flag, rank;
    leon::OwnBuf ulist0, ulist1, counters, cub_tmp, sort_key2, perm, perm2, events, prev, sym_off, syms;
    leon::OwnBuf blk_begin, out_off, out_size, rc_out, rc_scratch, dst_off, payload, errflag, nerr, wbits, fbits, pbits;
    leon::PinnedBuf h_payload;                   // the payloads of a launch cross to it
    uint64_t last_n = 0, last_bases = 0;
    const void* last_d_bases = nullptr; const void* last_d_off = nullptr;      // the last encoded batch: its anchors can serve the smoothing of the same reads
    leon::DecoderState dc;
    leon_dna_stats stats{};
    leon::EventList ev;                          // twelve, made at create: a batch's stage boundaries
    leon::EventList pack_ev;                     // pairs around the pack launches of a batch
    uint64_t* rb() const { return h_rb.as<uint64_t>(); }
    const uint16_t* rv16() const { return d_rv16.as<uint16_t>(); }
};

namespace leon {
// a context call's failure: its words stay with the context (device_call.h has the forms for calls without one)
inline int fail(leon_dna_ctx* c, int code, const std::string& msg) { if (!c) return dev_fail(code, msg); c->err = msg; return code; }
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return leon::fail((c), LEON_E_HIP, leon::hip_failure(#call, e_)); } while (0)
// The short waits of a batch -- a counter read back after a kernel of a millisecond, hundreds of them in the anchor resolution, and
// the ones before the first anchors reach the dictionary chain -- POLL the stream instead of calling hipStreamSynchronize: a wait
// that goes to sleep comes back on the host's 10 ms tick here (steps of chain + 30-40 ms, leon_dna_reset_stream taking 17 ms instead
// of 0.4), and the read-backs land in pinned host words so that the copies themselves do not wait inside the runtime.  Long waits
// (the walk, the range coder) keep sleeping: a spinning core would only take clock from the chain's.
// LEON_SPIN_SYNC=0: always sleep in the runtime instead (hosts with few cores, or many contexts whose spinning waits would compete
// with one another and with the chain thread the spinning was meant to help).
inline hipError_t spin_sync(hipStream_t s) {
    static const bool spin = [] { const char* e = getenv("LEON_SPIN_SYNC"); return !(e && e[0] == '0'); }();
    if (!spin) return hipStreamSynchronize(s);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0;; i++) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        for (int k = 0; k < 32; k++) __builtin_ia32_pause();
        if ((i & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    (void)hipGetLastError();
    return hipStreamSynchronize(s);
}
inline int ensure_cub(leon_dna_ctx* c, size_t bytes) { HIPCHK(c, c->cub_tmp.ensure(bytes)); return LEON_OK; }
// a rocPRIM call in its two steps: asked for the work space it needs, then run in c->cub_tmp grown to that
template <typename F> int run_prim(leon_dna_ctx* c, F&& call) {
    size_t bytes = 0;
    HIPCHK(c, call(nullptr, bytes));
    if (int rc = ensure_cub(c, bytes)) return rc;
    HIPCHK(c, call(c->cub_tmp.p, bytes));
    return LEON_OK;
}
inline int StreamCursor::follows(leon_dna_ctx* c, uint64_t first_read_index, uint64_t n, const char* stream) const {
    if (first_read_index != next_read) return fail(c, LEON_E_STATE, std::string("first_read_index does not continue the ") + stream);
    if (partial_seen && n) return fail(c, LEON_E_STATE, "a batch with a partial block must be the last one");
    return LEON_OK;
}
// A batch that failed after it had begun to change the stream poisons it: every call on the stream is refused until
// leon_dna_reset_stream, and the failure that did it says so.
inline int refuse_poisoned(leon_dna_ctx* c) { return fail(c, LEON_E_STATE, "an earlier batch failed part-way: the stream is unusable until leon_dna_reset_stream"); }
inline int note_poisoned(leon_dna_ctx* c, int rc) { if (rc != LEON_OK && c->poisoned) c->err += " (stream poisoned: leon_dna_reset_stream to go on)"; return rc; }// Where rank `rank` of `world` begins its share of a batch of n_blocks blocks: the share is the contiguous range of whole blocks
// [block_start(rank), block_start(rank + 1)), all of them when world is 1.
inline uint64_t block_start(uint64_t n_blocks, uint64_t rank, uint64_t world) { return rank * (n_blocks / world) + std::min(rank, n_blocks % world); }
// this context's rank's share of a batch of n reads: blocks [lb0, lb0 + nbl), reads [r0, r0 + nl)
struct Share { uint64_t lb0, nbl, r0, nl; };
inline Share share_of(const leon_dna_ctx* c, uint64_t n) {
    const uint64_t rpb = c->cfg.reads_per_block, n_blocks = (n + rpb - 1) / rpb;
    const uint64_t lb0 = block_start(n_blocks, c->shard_rank, c->shard_world), lb1 = block_start(n_blocks, c->shard_rank + 1, c->shard_world);
    const uint64_t r0 = std::min(n, lb0 * rpb), r1 = std::min(n, lb1 * rpb);
    return {lb0, lb1 - lb0, r0, r1 - r0};
}

// ---- capi.hip: the pack stage's front, shared with the quality smoothing and the header stream ----
ReadsDev reads_view(leon_dna_ctx* c, const uint64_t* d_off, uint64_t n);
int ensure_pack_bufs(leon_dna_ctx* c, uint64_t n, uint64_t n_slots);
// d_off[0 .. n] is an offsets array (else LEON_E_INVALID "offsets are not monotonic (or <too_long>)"), its reads' 32-base slots counted into
// c->slot_off.  n_slots: nullptr, or the counts scanned and their sum.  spin: the wait polls (spin_sync: the encode path) or sleeps.
int check_offsets(leon_dna_ctx* c, const uint64_t* d_off, uint64_t n, const char* too_long, uint64_t* n_slots, bool spin);

// ---- rc_kernels.hip: the block-coding tail of a stream ----
// A share's coded blocks, in block order: block b's sizes[b] bytes are hb.coders[b]'s (host chains) or at h_payload + dst[b].
struct CodedBlocks { bool host_chains = false; uint64_t n_syms = 0, payload_bytes = 0; std::vector<uint64_t> sizes, dst; };
int code_blocks(leon_dna_ctx* c, const Share& sh, const std::function<void(uint8_t* syms)>& symbols, uint32_t small_sizes, bool counts_apart,
                const char* unit, CodedBlocks& out);
int ensure_block_bufs(leon_dna_ctx* c, uint64_t nbl);                 // (sized by leon_dna_reserve too)
int ensure_rc_bufs(leon_dna_ctx* c, uint64_t nbl, uint64_t n_syms);
int deliver_blocks(leon_dna_ctx* c, const CodedBlocks& out, const Share& sh, uint64_t n, uint64_t first_block, leon_block_sink sink, void* user);
// Symbols in device memory -> k_rc_encode -> sizes and bytes (leon_rc_encode_streams, leon_dna_finish): n_streams streams of begin_host[b + 1] -
// begin_host[b] symbols of d_syms, the longest of `longest` (`overflow`: the LEON_E_OVERFLOW text); stream b's sizes[b] bytes then lie at out + off[b].
struct RcStreamsDev {
    OwnBuf begin, d_off, size, out, scr; std::vector<uint64_t> off;
    int code(leon_dna_ctx* c, const uint8_t* d_syms, const uint64_t* begin_host, uint64_t n_streams, uint64_t longest, const char* overflow, uint64_t* sizes);
};

// ---- decode_kernels.hip: a block table on the device, the DNA decoder's and the header decoders' ----
// payload_off must be monotonic (LEON_E_INVALID); then the payloads, 1024 zero bytes behind them (the payload window reads up to
// 256 + 3 bytes past a block's end), in `pay`, and the table -- offsets from the first payload's first byte, reads per block -- in T
struct BlockTableDev { OwnBuf off, nreads; };
int block_table_to_device(leon_dna_ctx* c, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads, uint64_t n_blocks,
                          DevBuf& pay, BlockTableDev& T, uint64_t* ordered = nullptr /* the blocks before the first offender */);
}  // namespace leon
