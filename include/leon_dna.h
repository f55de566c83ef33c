/*
 * leon_dna.h -- C-ABI of the MI355X-native Leon DNA encode path (libleon_dna.so).
 *
 * This is the drop-in boundary for the one hot path SURVEY.md section 8 scopes: what gatb-core's
 * Leon::startDnaCompression does by running Dispatcher::iterate(bank, DnaEncoder(this)) on pthreads
 * (call shape verified at /root/reference/src/main.cpp:44 `Leon().run(argc, argv)`; everything below
 * it lives in the un-vendored gatb-core submodule, /root/reference/.gitmodules:1-3, so the upstream
 * names cited per entry point are [RECALLED] names, not file:line -- SURVEY.md section 0).
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; every call returns 0 on success or a
 * negative LEON_E_* code and never throws; leon_last_error() gives the message.  One ctx = one ordered
 * read stream (one output file); calls on a ctx are serialised by the caller; HIP streams are private.
 * There is NO CPU fallback: without a HIP device ctx_create fails with LEON_E_NO_DEVICE.
 */
#ifndef LEON_DNA_H
#define LEON_DNA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LEON_DNA_ABI_VERSION 5

enum {
    LEON_OK = 0,
    LEON_E_INVALID = -1,     /* bad argument / configuration */
    LEON_E_NO_DEVICE = -2,   /* no usable HIP device (the product has no CPU path) */
    LEON_E_HIP = -3,         /* HIP runtime error, message carries hipGetErrorString */
    LEON_E_STATE = -4,       /* call order violated (e.g. encode after finish), or the stream is poisoned: a batch that
                                failed after it had begun to change the stream (HIP error, internal bound, sink) leaves the
                                dictionary and the caller's block sequence part-way through; every later call on the stream
                                returns this code until leon_dna_reset_stream.  Batches refused for their arguments
                                (LEON_E_INVALID, call order) leave the context untouched. */
    LEON_E_OVERFLOW = -5,    /* an internal device buffer bound was hit (reported, never silently truncated) */
    LEON_E_SINK = -6         /* the block sink returned non-zero */
};

typedef struct leon_dna_ctx leon_dna_ctx;

/* Replaces the state a DnaEncoder copies from its owning Leon*: _kmerSize, Leon::READ_PER_BLOCK and the
 * shared IBloom<kmer_type>* created by Leon::createBloom (BloomFactory BLOOM_NEIGHBOR, 7 hashes). */
typedef struct leon_dna_cfg {
    uint32_t struct_size;        /* sizeof(leon_dna_cfg) */
    uint32_t kmer_size;          /* 3..63.  k-mers cross this ABI as W 64-bit words each, low word first:
                                    W = 1 below 32 (upstream LargeInt<1>), W = 2 from 32 to 63 (LargeInt<2>) */
    uint32_t reads_per_block;    /* Leon::READ_PER_BLOCK, 50000 */
    uint32_t bloom_n_hash;       /* 7 */
    uint32_t bloom_block_nbits;  /* BloomCacheCoherent block_nbits, 12 */
    int32_t  device_id;          /* HIP device ordinal */
    uint64_t bloom_tai;          /* tai_bloom as handed to BloomNeighborCoherent (bits, before its padding) */
    const uint64_t* random_values; /* optional 256-entry simplehash16 table; NULL = built-in */
    uint64_t resolve_window;     /* reads per anchor-resolution window; 0 = default (1<<21) */
    uint32_t flags;              /* LEON_F_* */
    uint32_t dict_piece_anchors; /* with LEON_F_DICT_PIECES: anchors per piece, 0 = 1024, otherwise 1 .. 2^20; must be 0 without the flag */
} leon_dna_cfg;

#define LEON_F_KEEP_TRACE 1u     /* keep per-read anchors / events of the last batch for leon_dna_trace_* */
#define LEON_F_DICT_ON_DEVICE 2u /* code the anchor-dictionary stream with the device range coder (one serial chain on one
                                    workgroup, ~50x slower than the default host thread: DESIGN.md 4.4) instead of the host thread */
#define LEON_F_DICT_PIECES 4u    /* write the anchor dictionary as independently coded PIECES of dict_piece_anchors anchors (a different
                                    stream: leon_dna_dict_pieces below), coded on the device by leon_dna_finish; the host
                                    chain is not fed.  Not together with LEON_F_DICT_ON_DEVICE. */

/* Replaces Leon::writeBlock(buffer, size, nReads, blockId): called on the calling thread, in increasing
 * block_id; payload is owned by the library and valid until the sink returns.  Non-zero aborts. */
typedef int (*leon_block_sink)(void* user, uint64_t block_id, const uint8_t* payload, uint64_t size,
                               uint32_t n_reads);

typedef struct leon_dna_stats {
    uint64_t n_reads, n_bases, n_blocks, n_anchors, n_no_anchor, n_symbols, payload_bytes;
    uint64_t resolve_rounds, resolve_windows;
    /* HIP-event milliseconds of the last batch, measured on the library's own stream */
    float ms_pack, ms_resolve, ms_sort, ms_walk, ms_symbols, ms_rangecoder, ms_d2h, ms_total;
    uint32_t walk_launches, reserved;
    float ms_anchor_wait, ms_chain_busy;   /* host ms leon_dna_finish waited for the dictionary-stream thread; ms that thread spent coding */
    /* the walk divided by anchor (leon_dna_set_exchange), last batch: ms_walk above is then this rank's SLICE; ms_exchange = forming the
       words + the caller's exchange + scattering what came back (host wall-clock, the call waits for the device around it);
       ms_emulated = LEON_XCH_EMULATE only: the other ranks' slices walked here in their stead (not part of a real rank's time) */
    float ms_exchange, ms_exchange_call, ms_emulated, ms_emulated_lookups;   /* ms_emulated_lookups: the part of ms_emulated (and of ms_resolve) spent on the other ranks' window look-ups */
    uint64_t xch_words_sent, xch_words_received, walk_reads;
    /* anchor resolution, last batch: resolve_rounds above counts the parallel rounds; what they left unsettled (reads each waiting for the
       one before it: files in genome-position order) went through the exact sequential pass -- that many reads, in that many windows,
       ms_resolve_chain of ms_resolve (ABI 5) */
    uint64_t resolve_chain_reads, resolve_chain_windows;
    float ms_resolve_chain, ms_gather_call;   /* ms_gather_call: host ms inside the caller's gather callback (leon_dna_set_gather), part of ms_exchange_call */
} leon_dna_stats;

/* -- lifecycle (DnaEncoder ctor / dtor bracket one thread's work upstream) -- */
int  leon_dna_ctx_create(const leon_dna_cfg* cfg, leon_dna_ctx** out);
void leon_dna_ctx_destroy(leon_dna_ctx* ctx);
const char* leon_last_error(const leon_dna_ctx* ctx);      /* ctx may be NULL: last create error */
int  leon_dna_abi_version(void);

/* -- bloom (probe side is on the path; build side: Leon::createBloom's insert loop) -- */
int leon_dna_bloom_nbytes(const leon_dna_ctx* ctx, uint64_t* nbytes);          /* Bloom::getSize, nchar */
int leon_dna_bloom_upload(leon_dna_ctx* ctx, const uint8_t* bits, uint64_t nbytes);   /* StorageTools::loadBloom */
int leon_dna_bloom_download(leon_dna_ctx* ctx, uint8_t* bits, uint64_t nbytes);       /* StorageTools::saveBloom */
int leon_dna_bloom_clear(leon_dna_ctx* ctx);
int leon_dna_bloom_insert(leon_dna_ctx* ctx, const uint64_t* kmers, uint64_t n);      /* n host k-mers (n*W words), IBloom::insert */
int leon_dna_bloom_insert_device(leon_dna_ctx* ctx, const uint64_t* d_kmers, uint64_t n);
int leon_dna_bloom_device_ptr(leon_dna_ctx* ctx, void** d_bits, uint64_t* nbytes);    /* for an RCCL broadcast */
/* device-to-device forms of upload/download: the bloom travels between GPUs over xGMI, never via the host */
int leon_dna_bloom_upload_device(leon_dna_ctx* ctx, const uint8_t* d_bits, uint64_t nbytes);
int leon_dna_bloom_download_device(leon_dna_ctx* ctx, uint8_t* d_bits, uint64_t nbytes);
/* BloomNeighborCoherent::contains4 / contains over a list of k-mers (host in, host out) */
int leon_dna_bloom_contains4(leon_dna_ctx* ctx, const uint64_t* kmers, uint64_t n, int right, uint8_t* out);
int leon_dna_bloom_contains(leon_dna_ctx* ctx, const uint64_t* kmers, uint64_t n, uint8_t* out);

/* -- the hot path: DnaEncoder::operator()(Sequence&) over a batch of reads in file order --
 * bases: concatenated ASCII read data (A,C,G,T; any other byte is an N); offsets[n_reads+1].
 * first_read_index must continue the stream; every batch but the last must hold a whole number of
 * blocks (n_reads % reads_per_block == 0).  Blocks go to `sink` in increasing block_id. */
int leon_dna_encode_batch(leon_dna_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                          uint64_t first_read_index, leon_block_sink sink, void* user);
/* same with bases/offsets already resident in device memory (HBM) */
int leon_dna_encode_batch_device(leon_dna_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets,
                                 uint64_t n_reads, uint64_t first_read_index, leon_block_sink sink, void* user);

/* Optional: size every per-batch device buffer for batches of up to max_reads reads / max_bases bases ahead of the first
 * batch (a host calls it while it is still parsing the input), so that the first encode of a process allocates nothing
 * large.  Estimates only: whatever a batch needs beyond them is grown on demand. */
int leon_dna_reserve(leon_dna_ctx* ctx, uint64_t max_reads, uint64_t max_bases);

/* N contexts, one per GPU, working on ONE output file: every rank is fed the SAME batches; each resolves the
 * anchors of all reads (replicated, so the dictionary and every read's anchor are file-order exact on every rank
 * without any exchange), then walks and codes only its contiguous share of each batch's blocks, which its sink
 * receives with their global block ids.  Rank 0 alone produces the dictionary stream.  Default: rank 0 of 1. */
int leon_dna_set_shard(leon_dna_ctx* ctx, uint32_t rank, uint32_t world);

/* How a batch's WALK is divided among the ranks of leon_dna_set_shard(rank, world > 1).
 * LEON_XCH_OFF (default): every rank walks the reads of its own block range.  The reads of one anchor are spread over all block
 * ranges, so every rank fetches nearly every anchor group's bloom sectors: the eight ranks' walks of a 100 M-read file add up to
 * 2.8 x the one-GPU walk.
 * LEON_XCH_BY_ANCHOR: the batch's reads, sorted by anchor address, are cut into `world` contiguous slices and rank r walks slice r --
 * whole anchor groups, the sharing that makes the one-GPU walk cheap -- whatever block the reads belong to; what the walk found then
 * travels to the rank that codes each read's block in ONE exchange per batch, which the CALLER performs (the library stays free of
 * RCCL): `fn` is called once per batch, on the calling thread, with this rank's 64-bit words in DEVICE memory grouped by
 * destination rank (send_counts[d] words for rank d, in rank order) and must return, in device memory that stays valid until the
 * next call on this context, the words the other ranks (and this one) hold for this rank, concatenated in any order, with their
 * total in *recv_total -- an all-to-all (ncclAllToAllv / all_to_all_single).  Every rank must call it for every batch, also a rank
 * that codes no block of the batch.  Non-zero return = the batch fails (LEON_E_SINK-like: LEON_E_STATE, stream poisoned).
 * LEON_XCH_EMULATE: the same division with NO other rank present: the context walks every slice itself, one after the other, and
 * keeps the words meant for its own rank -- the bytes of a real run (one-process tests of an N-rank job, timing one seat of it:
 * stats.ms_walk is the own slice, stats.ms_emulated the rest).  fn is ignored.
 * The blocks' bytes are the same in all three modes. */
enum { LEON_XCH_OFF = 0, LEON_XCH_BY_ANCHOR = 1, LEON_XCH_EMULATE = 2 };
typedef int (*leon_exchange_fn)(void* user, const uint64_t* d_send, const uint64_t* send_counts, uint32_t world,
                                const uint64_t** d_recv, uint64_t* recv_total);
int leon_dna_set_exchange(leon_dna_ctx* ctx, uint32_t mode, leon_exchange_fn fn, void* user);

/* The anchor resolution's look-ups (a good half of the stage every rank otherwise repeats for ALL reads) divided among the ranks as
 * well: of every resolution window rank r looks up the r-th run of ceil(window / world) reads, and ONE all-gather per window --
 * again the caller's -- tells every rank what every read's pass found: `fn` is called on the calling thread with a device buffer of
 * world * part_bytes bytes whose part r (at d_buf + r * part_bytes) this rank has filled for r == its own rank, and must return with
 * every part filled by its rank (ncclAllGather / all_gather_into_tensor, in place or through a copy).  Each rank then makes the
 * other runs' results its own (the found key's slot, the proposals' entries in its dictionary), so the dictionaries stay identical.
 * Takes effect with LEON_XCH_BY_ANCHOR and world > 1; LEON_XCH_EMULATE computes the other ranks' runs itself
 * (stats.ms_emulated_lookups).  ~50 calls per 100 M reads, 16 MB each at the default window.  fn == NULL: every rank looks
 * everything up (the default).  Must precede the first batch of a stream.  Non-zero return of fn = the batch fails. */
typedef int (*leon_gather_fn)(void* user, void* d_buf, uint64_t part_bytes, uint32_t world);
int leon_dna_set_gather(leon_dna_ctx* ctx, leon_gather_fn fn, void* user);
/* FAILURE WITH CALLBACKS SET -- a rule for the caller.  The two callbacks put the caller's collectives INSIDE leon_dna_encode_batch*: one
 * all-gather per resolution window, one all-to-all per batch.  A rank whose call fails for a reason of its own (no memory for a buffer,
 * a HIP error, its sink, input the other ranks did not get) returns at once with its error code and does NOT enter the collectives it
 * has not reached: the library cannot "meet" them with empty parts, it does not know the caller's communicator.  The other ranks are
 * then waiting in theirs.  So a caller that sets a callback MUST treat a non-zero return of leon_dna_encode_batch* on any rank as the
 * end of the job on all of them: abort the communicator (ncclCommAbort), or run with a collective timeout and end the process non-zero
 * so that the launcher tears the job down -- bench.py does the latter: `Watch` names the collective that did not complete within
 * LEON_BENCH_COLL_TIMEOUT seconds and exits, a failed rank exits at once.  The context itself is poisoned (LEON_E_STATE) like after any
 * failure part-way through a batch; leon_dna_reset_stream starts a new stream once the communicator is whole again. */

/* Leon::endDnaCompression: flush the anchor-dictionary range coder (Leon::encodeInsertedAnchor stream).
 * payload stays owned by ctx until destroy. */
int leon_dna_finish(leon_dna_ctx* ctx, const uint8_t** dict_payload, uint64_t* dict_size, uint64_t* n_anchors);

/* -- the step BEFORE the path: solid k-mers of the reads, the set Leon::createBloom inserts (upstream DSK,
 * SortingCountAlgorithm).  Canonical k-mers occurring at least min_abundance times (0 = automatic threshold, see leon_kmer_auto_cutoff); k-mers containing an N are skipped.
 * Output: W words per k-mer (unordered across hash partitions).  histogram (optional, 256 entries): number of distinct
 * k-mers by abundance, clipped at 255.  max_keys_per_pass: k-mers sorted at once (0 = sized from the free device memory).  Errors: leon_last_error(NULL). */
int leon_kmer_solid_device(int device_id, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads,
                           uint32_t kmer_size, uint32_t min_abundance, uint64_t max_keys_per_pass,
                           uint64_t** d_solid, uint64_t* n_solid, uint64_t* histogram);   /* *d_solid: leon_device_free */
int leon_kmer_solid(int device_id, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t kmer_size,
                    uint32_t min_abundance, uint64_t max_keys_per_pass, uint64_t* out, uint64_t out_cap, uint64_t* n_solid,
                    uint64_t* histogram);
void leon_device_free(void* d_ptr);
/* leon_kmer_solid_device keeps its large work buffers for its next call instead of freeing them (freed device memory is wiped by the
 * driver before it is handed out again, at the expense of whoever allocates next); leon_dna_reserve returns them once the context's
 * own buffers exist, and so does this. */
void leon_device_trim(void);
/* min_abundance = 0 in the two calls above means "automatic" (Leon's default, /root/reference/README.md:54): the threshold
 * this function derives from the abundance spectrum (first local minimum, never below 2; 2 when there is no valley).
 * histogram: 256 entries as returned above.  Host-only. */
int leon_kmer_auto_cutoff(const uint64_t* histogram, uint32_t* cutoff);
/* plain device memory for callers that keep their reads resident in HBM (the host mirror's -c does): errors through
 * leon_last_error(NULL) */
int leon_device_count(int* n_devices);
int leon_device_alloc(int device_id, uint64_t bytes, void** d_ptr);
int leon_device_upload(int device_id, void* d_dst, const void* src, uint64_t bytes);
int leon_device_copy(int device_id, void* d_dst, const void* d_src, uint64_t bytes);   /* device to device; complete on return */
int leon_device_download(int device_id, void* dst, const void* d_src, uint64_t bytes);

/* Host-only helper (no GPU, no ctx): the dictionary stream leon_dna_finish returns for a given anchor list, i.e.
 * Leon::encodeInsertedAnchor over `kmers` in address order followed by the flush.  Used by the CPU tests. */
int leon_host_anchor_dict_encode(const uint64_t* kmers, uint64_t n_anchors, uint32_t kmer_size, uint8_t* out,
                                 uint64_t out_cap, uint64_t* size);

/* -- the anchor dictionary in independently coded pieces --
 * Anchors in address order are cut into pieces of P = piece_anchors anchors (0 = 1024, at most 2^20; the last piece holds the rest),
 * n_pieces = ceil(n_anchors / P).  Piece p is exactly the bytes leon_host_anchor_dict_encode returns for anchors [p * P, min((p + 1) * P,
 * n_anchors)): a fresh model, a fresh coder, the 8 flush bytes.  The stream is the pieces back to back; piece_off (n_pieces + 1 entries,
 * piece_off[0] = 0) says where each begins.
 * leon_dna_dict_pieces: after leon_dna_finish on a context created with LEON_F_DICT_PIECES -- whose dict_payload is then this stream --
 * its table; *piece_off is the context's until leon_dna_reset_stream or destroy.  LEON_E_STATE before leon_dna_finish or without the flag.
 * The context-free calls work on a stream of their own beside calls on any context and are complete on return.
 * encode: d_kmers (n_anchors * W words) in DEVICE memory, out / piece_off in host memory; *size = the stream's bytes, LEON_E_OVERFLOW when
 * out_cap is smaller (piece_off is filled, out is not written).  k_dict_encode_pieces, lane = piece.
 * decode: everything in host memory; out_kmers (n_anchors * W words) is written only when every piece has decoded, else LEON_E_INVALID
 * "anchor dictionary piece N does not decode" names the SMALLEST piece that fails.  k_dict_decode_pieces, lane = piece.
 * The leon_host_ twins do the same without a device (the encode twin takes the k-mers in host memory), one piece per task on n_threads
 * host threads (0 = all this process may use).  They are the verdict for the device calls: the same arguments are refused, before a
 * device is touched, with the same code and words -- null pointers, kmer_size outside 1..63, piece_anchors above 2^20, "piece table does
 * not match the anchor count" (n_pieces != ceil(n_anchors / P)), "piece offsets run backwards".  Errors: leon_last_error(NULL). */
int leon_dna_dict_pieces(leon_dna_ctx* ctx, const uint64_t** piece_off, uint64_t* n_pieces, uint32_t* piece_anchors);
int leon_anchor_dict_encode_pieces_device(int device_id, const uint64_t* d_kmers, uint64_t n_anchors, uint32_t kmer_size, uint32_t piece_anchors,
                                          uint8_t* out, uint64_t out_cap, uint64_t* piece_off, uint64_t* size);
int leon_anchor_dict_decode_pieces_device(int device_id, const uint8_t* payload, const uint64_t* piece_off, uint64_t n_pieces, uint64_t n_anchors,
                                          uint32_t kmer_size, uint32_t piece_anchors, uint64_t* out_kmers);
int leon_host_anchor_dict_encode_pieces(const uint64_t* kmers, uint64_t n_anchors, uint32_t kmer_size, uint32_t piece_anchors, uint8_t* out,
                                        uint64_t out_cap, uint64_t* piece_off, uint64_t* size, uint32_t n_threads);
int leon_host_anchor_dict_decode_pieces(const uint8_t* payload, const uint64_t* piece_off, uint64_t n_pieces, uint64_t n_anchors,
                                        uint32_t kmer_size, uint32_t piece_anchors, uint64_t* out_kmers, uint32_t n_threads);

/* -- the inverse path: DnaDecoder::execute over read blocks, blocks in parallel on the device --
 * Needs the bloom of the compressed file in ctx (leon_dna_bloom_upload).  anchors: the dictionary (n_anchors * W words,
 * from leon_host_anchor_dict_decode).  payloads: the blocks' payloads back to back, payload_off[n_blocks + 1];
 * block_n_reads / block_n_bases: reads and bases per block (the container's block table).  Output: the reads' bases back
 * to back in block order (out_cap >= the sum of block_n_bases) and every read's length (sum of block_n_reads entries).
 * LEON_E_INVALID with a message when a payload does not decode against this bloom / dictionary; out_bases and out_len are then
 * as the caller left them (the call writes them only once every block has decoded).  "block N does not decode: <reason>" names the
 * SMALLEST block that fails, with that block's own reason, however many fail.
 * Memory: the context keeps a table of what the decoding waves have learnt from the bloom (16 or 32 bytes x 4 per solid
 * k-mer the bloom was sized for, at most 40 % of the device's free memory; LEON_DC_CACHE_MB in the environment overrides,
 * 0 = none) from call to call, for as long as the bloom's bits do not change and the context does not encode (an encode
 * call returns the table's memory first); it makes the call faster, never different.
 * n_threads of the host functions below: 0 = the CPUs this process may use (its cgroup's quota). */
int leon_dna_decode_blocks(leon_dna_ctx* ctx, const uint64_t* anchors, uint64_t n_anchors, const uint8_t* payloads,
                           const uint64_t* payload_off, const uint32_t* block_n_reads, const uint64_t* block_n_bases,
                           uint64_t n_blocks, uint8_t* out_bases, uint64_t out_cap, uint32_t* out_len);
/* The same with the bases and lengths left in CALLER-OWNED device buffers (leon_device_alloc): d_out_bases (out_cap >= the sum of
 * block_n_bases) and d_out_len (one uint32 per read), complete on return and untouched when the call fails; out_len (may be NULL): a host
 * copy of the lengths as well.  Caller-owned, because a caller that works on one call's reads on the device while the next call decodes
 * cannot have them in the context's own buffers.  Same validation, errors and messages as leon_dna_decode_blocks. */
int leon_dna_decode_blocks_device(leon_dna_ctx* ctx, const uint64_t* anchors, uint64_t n_anchors, const uint8_t* payloads,
                                  const uint64_t* payload_off, const uint32_t* block_n_reads, const uint64_t* block_n_bases,
                                  uint64_t n_blocks, uint8_t* d_out_bases, uint64_t out_cap, uint32_t* d_out_len, uint32_t* out_len);
/* Host-only (no GPU, no ctx): Leon::decodeAnchorDict, the inverse of the stream leon_dna_finish returns.
 * out_kmers: n_anchors * W words. */
int leon_host_anchor_dict_decode(const uint8_t* payload, uint64_t size, uint64_t n_anchors, uint32_t kmer_size,
                                 uint64_t* out_kmers);

/* -- the streams either side of the DNA stream --------------------------------------------------
 * Header stream, Leon::startHeaderCompression's Dispatcher::iterate(bank, HeaderEncoder(this)) [RECALLED]: headers
 * (text after '>' / '@', no newline) back to back with offsets[n_reads + 1], in file order; first_header: the file's
 * first header, which every block starts from (AbstractHeaderCoder::startBlock; upstream stores it in the metadata).
 * Same batching rules and sink contract as leon_dna_encode_batch; the header stream keeps its own read / block
 * counters on the context and follows leon_dna_set_shard.  Record layout: DESIGN.md section 1.3. */
int leon_header_encode_batch(leon_dna_ctx* ctx, const uint8_t* headers, const uint64_t* offsets, uint64_t n_reads,
                             uint64_t first_read_index, const uint8_t* first_header, uint64_t first_header_len,
                             leon_block_sink sink, void* user);
int leon_header_encode_batch_device(leon_dna_ctx* ctx, const uint8_t* d_headers, const uint64_t* d_offsets, uint64_t n_reads,
                                    uint64_t first_read_index, const uint8_t* first_header, uint64_t first_header_len,
                                    leon_block_sink sink, void* user);
/* Host-only (no GPU, no ctx): HeaderDecoder over read blocks, blocks in parallel on n_threads host threads (0 = all).
 * out: the headers back to back in block order, out_off[total reads + 1]; *out_size = bytes needed (LEON_E_OVERFLOW when
 * out_cap is smaller: call again with that capacity).  Errors: leon_last_error(NULL). */
int leon_host_header_decode_blocks(const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                                   uint64_t n_blocks, const uint8_t* first_header, uint64_t first_header_len, uint8_t* out,
                                   uint64_t out_cap, uint64_t* out_off, uint64_t* out_size, uint32_t n_threads);
/* The same with the arithmetic decoding on the device (one wave per block, every block at once; the header TEXT is rebuilt from
 * the decoded symbols on n_threads host threads): same arguments, same results and errors as leon_host_header_decode_blocks.
 * A block with more symbols than the device buffer gives it (free text in every header) sends the call to the host decoder. */
int leon_header_decode_blocks(leon_dna_ctx* ctx, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                              uint64_t n_blocks, const uint8_t* first_header, uint64_t first_header_len, uint8_t* out,
                              uint64_t out_cap, uint64_t* out_off, uint64_t* out_size, uint32_t n_threads);
/* leon_header_decode_blocks in its two halves, for callers that decode a file in rounds: the symbols of ALL header blocks in one device
 * call (a block is one serial chain on one wave, ~1.5 s whether the call holds 200 blocks or 2 000: a call per round pays that every
 * round), then the text of any run of blocks on host threads.  The set is the library's until leon_header_symbols_free.
 * leon_header_text_from_symbols: blocks [first_block, first_block + n_blocks) of the set, block_n_reads = THOSE blocks' read counts; outputs
 * and errors as leon_host_header_decode_blocks; LEON_E_STATE when the set's symbols did not fit the device buffer (free text in every
 * header): the caller then decodes the payloads with leon_host_header_decode_blocks. */
typedef struct leon_header_symbols leon_header_symbols;
int leon_header_decode_symbols(leon_dna_ctx* ctx, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                               uint64_t n_blocks, leon_header_symbols** set);
int leon_header_text_from_symbols(const leon_header_symbols* set, uint64_t first_block, uint64_t n_blocks, const uint32_t* block_n_reads,
                                  const uint8_t* first_header, uint64_t first_header_len, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                  uint64_t* out_size, uint32_t n_threads);
void leon_header_symbols_free(leon_header_symbols* set);
/* The header TEXT on the device as well (k_hdr_text, one wave per block: the device form of the host's text builder): same arguments,
 * results and errors as leon_header_decode_blocks, but the text comes back from the device as it is.  A block the kernel declines
 * -- a header longer than 4096 bytes, or more symbols than the block's share of the device buffer -- is decoded by the host
 * decoder from its payload on n_threads threads; *n_blocks_on_host (may be NULL) counts those blocks. */
int leon_header_decode_blocks_device(leon_dna_ctx* ctx, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                                     uint64_t n_blocks, const uint8_t* first_header, uint64_t first_header_len, uint8_t* out,
                                     uint64_t out_cap, uint64_t* out_off, uint64_t* out_size, uint32_t n_threads,
                                     uint64_t* n_blocks_on_host);
/* ... and its two halves, for callers that decode a file in rounds (as leon_header_decode_symbols / leon_header_text_from_symbols).
 * leon_header_decode_text: the symbols and the text of ALL header blocks in one device call (both kernels on the context's stream); the
 * text and one offset per header STAY IN DEVICE MEMORY until leon_header_text_free -- the text + 8 bytes per header, about 7 GB for
 * 100 M SRA-style headers --, the symbol buffer is released before the call returns.  block_text_bytes: every block's text size where
 * the caller knows it (the container's header table), or NULL: a sizing pass of the kernel counts them first.  A payload that does not
 * decode gives LEON_E_INVALID.  The set belongs to the context's device; free it before the context is destroyed.
 * leon_header_text_fetch: blocks [first_block, first_block + n_blocks) of the set to the host, outputs and LEON_E_OVERFLOW as
 * leon_host_header_decode_blocks; LEON_E_STATE when the kernel declined a block of the run (see above, or a block_text_bytes entry
 * that is not the block's size): the caller then decodes the run's payloads with leon_host_header_decode_blocks.
 * leon_header_text_device_ptr: the same run where it lies: *d_text its first byte, d_off[0 .. reads of the run] the headers' bounds
 * counted from the SET's first byte (d_off[i] - d_off[0] is header i's offset in the run), *size its bytes; same errors. */
typedef struct leon_header_text leon_header_text;
int leon_header_decode_text(leon_dna_ctx* ctx, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                            const uint64_t* block_text_bytes, uint64_t n_blocks, const uint8_t* first_header, uint64_t first_header_len,
                            leon_header_text** set);
int leon_header_text_fetch(const leon_header_text* set, uint64_t first_block, uint64_t n_blocks, uint8_t* out, uint64_t out_cap,
                           uint64_t* out_off, uint64_t* out_size);
int leon_header_text_device_ptr(const leon_header_text* set, uint64_t first_block, uint64_t n_blocks, const uint8_t** d_text,
                                const uint64_t** d_off, uint64_t* size);
void leon_header_text_free(leon_header_text* set);
/* -- the decoder's last step: the reads' FASTA / FASTQ text, formatted on the device (k_fmt_sizes, k_fmt_records: DESIGN.md 4.9) --
 * Record r of a call, as the host mirror's -d writes it:
 *     lead  header r | decimal(first_read_index + r)  '\n'
 *     the sequence: its len bytes and '\n' when wrap == 0 or len <= wrap, else ceil(len / wrap) lines of at most wrap bytes, each + '\n'
 *     fastq only:  '+'  [header r again when plus_kind == 1]  '\n'  len quality bytes  '\n'
 * Everything lies in device memory: d_bases (n_bases bytes, the reads back to back) and d_len[n_reads] as leon_dna_decode_blocks_device
 * leaves them; d_hdr_text / d_hdr_off[n_reads + 1] as leon_header_text_device_ptr hands them out (header r is d_hdr_text[d_hdr_off[r] -
 * d_hdr_off[0] .. d_hdr_off[r + 1] - d_hdr_off[0]), hdr_bytes of the layout = d_hdr_off[n_reads] - d_hdr_off[0]); d_hdr_text == NULL: the
 * read index stands in for the header; d_quals: one byte per base, indexed like d_bases (fastq only).  d_text needs no alignment.
 * d_rec_off (may be NULL): every record's offset in the text, n_reads + 1 entries.  *text_size: the text's bytes.
 * LEON_E_OVERFLOW when text_cap is smaller (or d_text NULL): *text_size = the bytes needed, nothing written.  LEON_E_INVALID, nothing
 * written: lengths that do not add up to n_bases or header offsets that run backwards or do not end at hdr_bytes (checked on the device
 * before anything is indexed with them), fastq without d_quals, plus_kind == 1 without headers, an unknown struct_size.
 * The call works on a stream of its own and may run beside calls on any context.  Errors: leon_last_error(NULL). */
typedef struct leon_record_layout {
    uint32_t struct_size;        /* sizeof(leon_record_layout) */
    uint8_t  lead;               /* '@' or '>' */
    uint8_t  fastq;              /* 1: '+' line and qualities */
    uint8_t  plus_kind;          /* 0: bare '+' lines, 1: every '+' line repeats its header */
    uint8_t  reserved;
    uint32_t wrap;               /* sequence line width, 0 = one line */
    uint32_t reserved2;
    uint64_t first_read_index;   /* the index of record 0 (what stands in for a header) */
    uint64_t hdr_bytes;          /* bytes of d_hdr_text the offsets must end at (ignored without headers) */
} leon_record_layout;
int leon_records_format_device(int device_id, const leon_record_layout* lay, const uint8_t* d_bases, const uint32_t* d_len, uint64_t n_reads,
                               uint64_t n_bases, const uint8_t* d_hdr_text, const uint64_t* d_hdr_off, const uint8_t* d_quals, uint8_t* d_text,
                               uint64_t text_cap, uint64_t* d_rec_off, uint64_t* text_size);
/* -- the same reads as unaligned BAM records (k_bam_sizes, k_bam_records: DESIGN.md 4.19) --
 * The uncompressed content of a BAM file is leon_bam_header's bytes ("BAM\1", l_text, the text "@HD\tVN:1.6\tSO:unsorted\n", n_ref = 0)
 * and then one record per read, little-endian:
 *     block_size (the bytes that follow)  refID -1  pos -1  l_read_name (counting its NUL)  mapq 0  bin 4680  n_cigar_op 0  flag 4
 *     l_seq  next_refID -1  next_pos -1  tlen 0  |  the name, NUL  |  (l_seq + 1) / 2 bytes, two bases a byte, the first in the high
 *     nybble, codes from "=ACMGRSVTWYHKDBN" whatever the case, any other byte 15  |  l_seq quality bytes, the FASTQ byte - 33  |
 *     'C' 'O' 'Z' the comment, NUL -- when there is a comment
 * The name is header r up to its first space or tab ("*" when empty; the decimal read index without a header stream), the comment what
 * follows that one byte.  [RECALLED from the SAM/BAM specification; parity with htslib's reader is unpinned.]
 * Arguments as leon_records_format_device's; lead, wrap and plus_kind of the layout are ignored; fastq == 0 or d_quals == NULL: every
 * quality byte is 0xFF.  d_out needs no alignment.  d_rec_off (may be NULL): n_reads + 1 record offsets ([0] = 0 also with no read).
 * LEON_E_OVERFLOW when out_cap is smaller (or d_out NULL): *out_size = the bytes needed, nothing written.  LEON_E_INVALID, nothing
 * written: lengths that do not add up to n_bases, header offsets that run backwards or do not end at hdr_bytes, an unknown struct_size,
 * a name of more than 254 bytes ("read N: its name has M bytes, BAM allows 254").  LEON_E_INVALID after the records were written (they
 * are to be discarded): "read N: a quality byte below 33".  N is the smallest such read of the call, counted from first_read_index.
 * leon_host_records_bam: the same bytes and verdicts from host memory, on n_threads threads (0: all usable), no GPU.
 * leon_bam_header: *size = the header's bytes; LEON_E_OVERFLOW when cap is smaller (or out NULL).  A file is these bytes and the records
 * through leon_text_bgzf_device (or _records_device / _ex, the header as the first call's head) with its EOF marker. */
int leon_records_bam_device(int device_id, const leon_record_layout* lay, const uint8_t* d_bases, const uint32_t* d_len, uint64_t n_reads,
                            uint64_t n_bases, const uint8_t* d_hdr_text, const uint64_t* d_hdr_off, const uint8_t* d_quals, uint8_t* d_out,
                            uint64_t out_cap, uint64_t* d_rec_off, uint64_t* out_size);
int leon_host_records_bam(const leon_record_layout* lay, const uint8_t* bases, const uint32_t* len, uint64_t n_reads, uint64_t n_bases,
                          const uint8_t* hdr_text, const uint64_t* hdr_off, const uint8_t* quals, uint8_t* out, uint64_t out_cap,
                          uint64_t* rec_off, uint64_t* out_size, uint32_t n_threads);
int leon_bam_header(uint8_t* out, uint64_t cap, uint64_t* size);
/* Device memory to a sink, in the pinned pieces the copy lands in (no second copy into pageable memory): the sink receives pieces of at
 * most 16 MiB, every byte of [0, bytes) exactly once, disjoint, IN NO PARTICULAR ORDER AND FROM UP TO LEON_UPLOAD_THREADS (default 3)
 * THREADS AT ONCE; a piece is valid until the sink returns.  Non-zero from the sink stops the call with LEON_E_SINK (pieces already
 * under way on other threads may still arrive).  Copies below four pieces come one piece at a time on the calling thread, from a pinned
 * buffer as well.  Errors: leon_last_error(NULL). */
typedef int (*leon_piece_sink)(void* user, uint64_t offset, const void* bytes, uint64_t size);
int leon_device_download_pieces(int device_id, const void* d_src, uint64_t bytes, leon_piece_sink sink, void* user);

/* Quality stream, lossy form (Leon's default, /root/reference/README.md:55): DnaEncoder::storeSolidCoverageInfo + smoothQuals
 * [RECALLED]: a quality becomes '@' where at least two of the read's solid k-mers (in the bloom of ctx) span the position, or
 * where it is above '@'; reads shorter than k are left alone.  quals: one byte per base, same offsets as the bases, rewritten
 * in place; what comes out then goes through leon_host_qual_encode_blocks like the lossless form. */
int leon_qual_smooth_batch(leon_dna_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint8_t* quals);
int leon_qual_smooth_batch_device(leon_dna_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads,
                                  uint8_t* d_quals);   /* d_quals[j] belongs to base d_bases[d_offsets[0] + j] */
/* Quality stream, lossless form (`-lossless`): per read block the quality lines, each followed by '\n', through zlib
 * (upstream deflates the block's buffered quality lines, Leon::writeBlockLena [RECALLED]).  Host-only, blocks in parallel
 * on n_threads threads; blocks go to the sink in increasing id starting at first_block_id.  zlib_level: -1 = zlib default. */
int leon_host_qual_encode_blocks(const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads, uint32_t reads_per_block,
                                 int zlib_level, uint32_t n_threads, leon_block_sink sink, void* user, uint64_t first_block_id);
/* The same blocks written on the device: d_quals = the qualities in device memory (d_quals[j] is the byte at offsets[0] + j of the
 * concatenation, as leon_qual_smooth_batch_device leaves them), offsets in HOST memory.  Each block is a zlib stream that inflates
 * to the block's quality lines, each followed by '\n' -- what leon_host_qual_decode_blocks (or upstream's inflate) reads -- but
 * not the bytes zlib's default strategy would write: deflate with matches at distance 1 only (zlib's Z_RLE) and dynamic Huffman
 * codes per 32 KB of text (deflate_kernels.hip).  Errors: leon_last_error(NULL). */
int leon_qual_deflate_blocks_device(int device_id, const uint8_t* d_quals, const uint64_t* offsets, uint64_t n_reads,
                                    uint32_t reads_per_block, leon_block_sink sink, void* user, uint64_t first_block_id);
/* It keeps its device buffers (about 1.5 GB after a large call) for the next call: this returns them. */
void leon_qual_deflate_release(void);
/* Any text in DEVICE memory written as BGZF, the blocked gzip of SAM / htslib: a series of independent gzip members
 * of LEON_BGZF_MEMBER_TEXT bytes of text each (the last one what is left), every one a block of the same encoder as above with its own
 * CRC-32 and ISIZE, and -- with `last` -- the 28-byte BGZF EOF marker behind them; any gzip reader reads the concatenation.
 * The call compresses *n_taken = last ? n_text : n_text - n_text % LEON_BGZF_MEMBER_TEXT bytes; the caller carries the rest in front of
 * the text of its next call, so the output is a function of the whole text alone, however it was split into calls.  d_text needs no
 * alignment and is never written.  The sink follows leon_device_download_pieces' contract: pieces of at most 16 MiB, every byte of
 * [0, *out_bytes) exactly once, in no particular order, from up to LEON_UPLOAD_THREADS threads at once; offsets count from this
 * call's first output byte.  Non-zero from the sink: LEON_E_SINK; after any failure the caller discards what it has received.
 * n_text == 0 (or below one member) without `last`: LEON_OK, nothing delivered; n_text == 0 with `last`: the EOF marker alone.
 * *n_members (may be NULL): the members written, the EOF marker not counted.
 * Refused before a device is touched, LEON_E_INVALID: d_text NULL with n_text != 0, a NULL sink, n_taken or out_bytes, a `last` other
 * than 0 or 1.  The text goes through in slices of 512 MiB (LEON_BGZF_SLICE in the environment: bytes, rounded down to whole
 * members), one after the other; the temporaries of a slice (about 2 bytes per byte of its text) are kept per device for the next call
 * and go with leon_qual_deflate_release.  The call works on a stream of its own.  Errors: leon_last_error(NULL). */
#define LEON_BGZF_MEMBER_TEXT 32768u
int leon_text_bgzf_device(int device_id, const uint8_t* d_text, uint64_t n_text, int last, leon_piece_sink sink, void* user,
                          uint64_t* n_taken, uint64_t* out_bytes, uint64_t* n_members);
/* The same stream with its members cut at RECORD STARTS, and a table of where every member lies.
 * d_text: n_head bytes of head, then n_body bytes whose records start at d_rec_off[0 .. n_records] -- DEVICE memory, relative to the
 * body, [0] = 0, [n_records] = n_body, strictly ascending: what leon_records_format_device writes into its d_rec_off.  The head is what
 * the call before did not take (n_head <= W = LEON_BGZF_MEMBER_TEXT): whole records from a record start; the records inside it need not
 * be known again.  The cut rule, from a cut p = s_i of the record starts s_0 = 0 < s_1 < ... < s_R = n_text:
 *   s_{i+1} - s_i > W (an oversized record): floor(len / W) members of W bytes and one of len % W when that is not 0; next cut s_{i+1};
 *   otherwise the next cut is the largest record start s_j <= p + W, j > i (as many whole records as fit; ending exactly at p + W fits).
 * Without `last` members are cut from p while n_text - p > W; the rest (at most W bytes of whole records) is not taken: *n_taken (head
 * included) says where it begins, and the caller puts it in front of its next call as that call's head.  With `last` the rest is the
 * final member when it is not empty, and the EOF marker follows.  The output is a function of the whole text and its record starts
 * alone, however they are split into calls and slices (LEON_BGZF_SLICE: a slice ends at a cut).
 * Every member has 1 .. W bytes of text; a call writes at most 3 * (n_text / W) + 2 of them, n_text = n_head + n_body: two neighbours
 * hold more than W bytes together unless the first is an oversized record's remainder, of which there are at most n_text / W; so
 * members <= 2 * (n_text / W) + 1 + n_text / W.
 * d_rec_off == NULL with n_records == 0 and n_head == 0: the fixed cuts and the bytes of leon_text_bgzf_device on (d_text, n_body).
 * member_out_off / member_text_off (HOST memory, members_cap entries each; both NULL with members_cap == 0: no table): per data member
 * its offset in this call's output and in this call's text.  *n_members is always the count; a table that is too small: LEON_E_OVERFLOW,
 * *n_members = the entries needed, nothing delivered to the sink.
 * Refused before a device is touched, LEON_E_INVALID: leon_text_bgzf_device's list (n_members must not be NULL here), n_head > W,
 * records given with d_rec_off NULL, a body without records in record mode (d_rec_off given, or a head), a half-given member table.
 * Refused on the device (k_bgzf_check_recs) before a byte is compressed or delivered, LEON_E_INVALID: offsets that are not strictly
 * ascending, do not start at 0 or do not end at n_body.  Sink, stream and temporaries: as leon_text_bgzf_device. */
int leon_text_bgzf_records_device(int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body,
                                  const uint64_t* d_rec_off, uint64_t n_records, int last,
                                  leon_piece_sink sink, void* user,
                                  uint64_t* n_taken, uint64_t* out_bytes,
                                  uint64_t* member_out_off, uint64_t* member_text_off, uint64_t members_cap, uint64_t* n_members);
/* leon_text_bgzf_records_device with a choice of encoder.  flags == 0: its bytes on the same arguments.
 * LEON_BGZF_F_MATCHES: every member's block comes from k_deflate_lz_chunks -- an LZ77 search inside the member (a hash of four bytes,
 * one candidate a position, greedy selection) with a distance code of its own, beside the runs and Huffman codes of the encoder above;
 * what record text wants, where a header line repeats most of the one before.  A member's block is a function of its text alone.
 * Cuts, member layout, member bound, sink, slices, carry rule and refusals are those of leon_text_bgzf_records_device; a bit of flags
 * that is not defined here is refused with them, LEON_E_INVALID, before a device is touched.  The kernel keeps 16 MiB more per device. */
#define LEON_BGZF_F_MATCHES 1u
int leon_text_bgzf_device_ex(int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body,
                             const uint64_t* d_rec_off, uint64_t n_records, int last,
                             leon_piece_sink sink, void* user,
                             uint64_t* n_taken, uint64_t* out_bytes,
                             uint64_t* member_out_off, uint64_t* member_text_off, uint64_t members_cap, uint64_t* n_members, uint32_t flags);
/* The same cut rule on HOST memory (no GPU): rec_off[0 .. n_records] as above (NULL with n_records == 0: a head alone), n_body =
 * rec_off[n_records].  begin / len (cap entries each; both NULL with cap == 0: count only): every member's offset in the call's text
 * (head included) and its bytes.  *n_members = the count, *n_taken as above.  LEON_E_OVERFLOW when a given table is too small
 * (*n_members = the need); LEON_E_INVALID in the device call's words for what both refuse. */
int leon_host_bgzf_record_cuts(const uint64_t* rec_off, uint64_t n_records, uint64_t n_head, int last, uint64_t* begin, uint32_t* len,
                               uint64_t cap, uint64_t* n_members, uint64_t* n_taken);
/* inverse: block_n_bytes = quality bytes per block without the newlines; out_off[total reads + 1] */
int leon_host_qual_decode_blocks(const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                                 const uint64_t* block_n_bytes, uint64_t n_blocks, uint8_t* out, uint64_t out_cap,
                                 uint64_t* out_off, uint32_t n_threads);
/* The same inverse into DEVICE memory, the blocks inflated by the device (inflate_kernels.hip: k_qual_inflate, one wave per block, and
 * a device-wide line pass).  payloads / payload_off[n_blocks + 1] / block_n_reads / block_n_bytes: HOST memory, as
 * leon_host_qual_decode_blocks takes them.  d_quals (device, quals_cap bytes): the blocks' quality bytes back to back WITHOUT the
 * newlines -- what leon_records_format_device takes as d_quals.  d_qual_off (device, may be NULL): total reads + 1 offsets into
 * d_quals, [0] = 0.  d_len (device, may be NULL): when given, read r's line must have exactly d_len[r] bytes.  n_symbols (host, may
 * be NULL): the literal/length symbols the call decoded (measurement).
 * One decoder for every RFC 1950 / 1951 stream -- who wrote the blocks is not asked.  The verdict is the host function's on the
 * same arguments: zlib's uncompress (header, code-length sets, codes, distances, stored lengths, a stream that ends early, the
 * Adler-32; bytes behind the stream's end are ignored) and the line rules (exactly block_n_bytes[b] + block_n_reads[b] bytes of
 * text, block_n_reads[b] newlines, the last byte one of them); LEON_E_INVALID "quality block N does not decode" names the smallest
 * block that fails.  Arguments are refused before a device is touched, with the host function's words.  The call works on a stream of
 * its own, beside a context's decode calls; its temporaries (the payloads, the text with its newlines) live for the call and are
 * bounded by working through the blocks in launches of at most 1 024 blocks and 8 GiB of text.  Errors: leon_last_error(NULL). */
int leon_qual_inflate_blocks_device(int device_id, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* block_n_reads,
                                    const uint64_t* block_n_bytes, uint64_t n_blocks, const uint32_t* d_len, uint8_t* d_quals,
                                    uint64_t quals_cap, uint64_t* d_qual_off, uint64_t* n_symbols);

/* -- block checksums: zlib's CRC-32 of segments of one buffer --
 * Segment s is bytes[seg_off[s] .. seg_off[s + 1]); crc[s] = what zlib's crc32() gives for it (reflected polynomial 0xEDB88320,
 * initial value and final XOR 0xFFFFFFFF; an empty segment gives 0).  seg_off (n_seg + 1 entries) and crc (n_seg) are HOST memory in
 * both forms.  Bytes outside [seg_off[0], seg_off[n_seg]) are never read.  Both forms refuse, before anything is touched, with
 * LEON_E_INVALID and the same words: null pointers with non-zero counts, offsets that run backwards, seg_off[n_seg] > n_bytes.
 * n_seg == 0 and segments that are all empty are LEON_OK.  Errors: leon_last_error(NULL).
 * The device form takes d_bytes in DEVICE memory (no alignment asked), works on a stream of its own beside calls on any context and
 * is complete on return; its temporaries (the offsets, 4 bytes per segment) live for the call (crc_kernels.hip: k_crc32_tiles). */
int leon_crc32_segments_device(int device_id, const uint8_t* d_bytes, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, uint32_t* crc);
/* zlib's crc32 on n_threads host threads (0 = all this process may use); needs no GPU */
int leon_host_crc32_segments(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, uint32_t n_threads, uint32_t* crc);

/* -- BGZF input inflated on the device --
 * A BGZF file is a series of gzip members of at most 64 KiB, each with an extra subfield B C 02 00 BSIZE (the member's size - 1) and,
 * behind its raw deflate stream, CRC-32 and ISIZE of its text; an empty member (ISIZE 0) is the EOF marker and may stand anywhere.
 *
 * leon_host_bgzf_members walks the members of bytes[0, n_bytes) (no GPU).  A member must begin 1f 8b 08 with FLG exactly 4; the XLEN
 * bytes of subfields are walked for B C 02 00 BSIZE, others in front of it are skipped; the deflate stream begins at 12 + XLEN and
 * BSIZE + 1 must hold the header and the 8-byte trailer.  member_off (off_cap entries) receives the members' first bytes and, as entry
 * *n_members, the end of the last whole one, which is also *consumed; *n_text = the sum of their ISIZE (a member whose ISIZE is above
 * 65 536 counts none: the inflate refuses it).  *stop says why the walk ended:
 *   LEON_BGZF_WHOLE      the range ends with a member's last byte (or is empty);
 *   LEON_BGZF_PARTIAL    last == 0: the member at *consumed is cut short by the end of the range, in its header, its payload or its
 *                        trailer -- "not consumed": the caller puts those bytes in front of the next range.  LEON_OK;
 *   LEON_BGZF_TRUNCATED  the same with last == 1 (the range ends the file): LEON_E_INVALID "BGZF member N (at byte X) is truncated";
 *   LEON_BGZF_FOREIGN    the bytes at *consumed are no BGZF member (a gzip member without the subfield, a BSIZE too small for its own
 *                        header, anything else): LEON_E_INVALID "no BGZF member at byte X (member N)".
 * The outputs are filled in every one of these cases.  LEON_E_OVERFLOW when the table needs more than off_cap entries (*n_members + 1).
 *
 * leon_host_bgzf_inflate (no GPU) inflates members [member_off[i], member_off[i + 1]) of bytes into text, back to back: zlib's inflate
 * on a raw stream, one member per thread (n_threads, 0 = all this process may use).  A member decodes when it is a BGZF member of
 * exactly its span, its stream ends with the last byte in front of the trailer, gives exactly ISIZE <= 65 536 bytes, and their CRC-32
 * is the trailer's.  *n_text = the bytes of text; LEON_E_OVERFLOW "the text needs N bytes" when text_cap is smaller, nothing decoded.
 * LEON_E_INVALID "BGZF member N (at byte X) does not decode" names the smallest member that fails.
 *
 * leon_bgzf_inflate_device does the same into DEVICE memory (inflate_kernels.hip: k_bgzf_inflate, one wave per member, into 16-byte
 * aligned shares of a temporary; crc_kernels.hip over them; k_bgzf_gather to d_text, which needs no alignment).  bytes and member_off
 * are HOST memory.  The verdict -- code and message -- is the host function's on the same arguments; arguments are refused before a
 * device is touched.  The members go through in launches of at most max_members_per_launch (0 = 4 096) members; a launch writes to
 * d_text only when every member of it has passed, so after a refusal of member N no byte of a member behind N's launch is written.
 * The kernels and the small copies run on a stream of the call's own; a launch's bytes go up in one blocking copy (through pinned
 * pieces from 64 MiB on, staging.h), complete before its kernel is launched; the temporaries live for the call and are bounded by
 * the launch size (at most 64 KiB of text and of payload per member).  n_symbols (host, may be NULL): the literal/length symbols
 * decoded (measurement).  Errors: leon_last_error(NULL). */
#define LEON_BGZF_WHOLE 0u
#define LEON_BGZF_PARTIAL 1u
#define LEON_BGZF_TRUNCATED 2u
#define LEON_BGZF_FOREIGN 3u
int leon_host_bgzf_members(const uint8_t* bytes, uint64_t n_bytes, int last, uint64_t* member_off, uint64_t off_cap, uint64_t* n_members,
                           uint64_t* n_text, uint64_t* consumed, uint32_t* stop);
int leon_host_bgzf_inflate(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* member_off, uint64_t n_members, uint8_t* text, uint64_t text_cap,
                           uint64_t* n_text, uint32_t n_threads);
int leon_bgzf_inflate_device(int device_id, const uint8_t* bytes, uint64_t n_bytes, const uint64_t* member_off, uint64_t n_members, uint8_t* d_text,
                             uint64_t text_cap, uint64_t* n_text, uint32_t max_members_per_launch, uint64_t* n_symbols);
/* Page-locked host memory for a caller that downloads into the same buffers again and again (the reader of `leon -c -input-inflate
 * device`): leon_device_download into it is one direct copy.  Freed with leon_host_pinned_free (NULL is allowed). */
int leon_host_pinned_alloc(int device_id, uint64_t bytes, void** ptr);
void leon_host_pinned_free(void* ptr);

/* -- FASTQ text split into records --
 * The text begins at a record start.  Lines end at '\n'; one '\r' directly in front of the '\n' is dropped, a '\r' anywhere else is
 * kept; with last != 0 the end of the text ends a line that has no '\n' (that line keeps a '\r' at its end).  Lines are taken in fours
 * from the start of the text: record r is lines 4r .. 4r + 3, and WHOLE when all four are there.  A whole record is REGULAR when
 *   its first line is non-empty and begins with '@'                                   (else LEON_FASTQ_R_HEADER),
 *   its third line begins with '+'                                                    (else LEON_FASTQ_R_PLUS),
 *   its second and fourth lines have the same length, 0 allowed                       (else LEON_FASTQ_R_LENGTH),
 *   its '+' line agrees with plus_kind                                                (else LEON_FASTQ_R_PLUS_TEXT):
 *     0: it is bare; 1: it repeats the header (the first line without its '@'); -1: the '+' lines of the split records are all the
 *     same one of the two.  A bare '+' under an empty header agrees with both and is counted in neither of plus_bare and plus_header;
 *     any other text after the '+' agrees with nothing.
 * The rules are tried in this order; `reason` is the first that record n_records broke.
 * The call splits the longest prefix of records that are whole, regular and at most max_records, nothing after it: the headers without
 * their '@', the second lines (bases) and the fourth lines (qualities), each back to back, header_off[n_records + 1] and
 * base_off[n_records + 1] beginning with 0 (the qualities share the bases' offsets).  `consumed`: the first byte not taken.  `stop`:
 *   LEON_FASTQ_MAX        n_records == max_records;
 *   LEON_FASTQ_IRREGULAR  record n_records is whole and not regular -- or, with last != 0, fewer than four lines are left behind the
 *                         split records and one of them is not empty (LEON_FASTQ_R_PARTIAL): the caller's parser is its judge;
 *   LEON_FASTQ_END        the text ran out: what is left is no whole record, or nothing.  With last != 0 the lines left (fewer than
 *                         four, all empty) are consumed: consumed == n_text.
 * bytes_cap: the room of each of the three blobs; records_cap: the entries of each offset table.  LEON_E_OVERFLOW when header_bytes or
 * base_bytes is above bytes_cap or n_records + 1 above records_cap (the result says what is needed; what the blobs and tables hold is not defined then, their ends are respected): a
 * caller with bytes_cap >= n_text and records_cap >= n_text / 4 + 2 never sees it.  LEON_E_INVALID: null pointers, n_text >= 2^32, a
 * plus_kind outside -1 .. 1.  Whatever else the text holds is data, never an error.
 * The device form (fastq_kernels.hip: k_fq_newlines, k_fq_check, k_fq_split) takes every pointer but `res` in DEVICE memory, no
 * alignment asked, works on a stream of its own and is complete on return; nothing outside the text is read, nothing behind
 * header_bytes / base_bytes / n_records + 1 entries is written.  The host form is the same contract in plain serial code (host_fastq.h)
 * and needs no GPU.  Errors: leon_last_error(NULL). */
#define LEON_FASTQ_MAX 0u
#define LEON_FASTQ_END 1u
#define LEON_FASTQ_IRREGULAR 2u
#define LEON_FASTQ_R_NONE 0u
#define LEON_FASTQ_R_HEADER 1u
#define LEON_FASTQ_R_PLUS 2u
#define LEON_FASTQ_R_LENGTH 3u
#define LEON_FASTQ_R_PLUS_TEXT 4u
#define LEON_FASTQ_R_PARTIAL 5u
typedef struct leon_fastq_split_result {
    uint64_t n_records;      /* records 0 .. n_records-1 were split */
    uint64_t consumed;       /* bytes of text they occupy: record n_records begins at text[consumed] */
    uint64_t header_bytes, base_bytes;      /* quality bytes == base_bytes */
    uint32_t stop;           /* LEON_FASTQ_MAX, LEON_FASTQ_END or LEON_FASTQ_IRREGULAR */
    uint32_t reason;         /* under LEON_FASTQ_IRREGULAR: the LEON_FASTQ_R_* rule record n_records broke; else LEON_FASTQ_R_NONE */
    uint64_t plus_bare, plus_header;        /* among the split records: '+' lines that are bare / repeat the header, headers non-empty */
} leon_fastq_split_result;
int leon_fastq_split_device(int device_id, const uint8_t* d_text, uint64_t n_text, int last, uint64_t max_records, int plus_kind,
                            uint8_t* d_headers, uint64_t* d_header_off, uint8_t* d_bases, uint64_t* d_base_off, uint8_t* d_quals,
                            uint64_t bytes_cap, uint64_t records_cap, leon_fastq_split_result* res);
int leon_host_fastq_split(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, int plus_kind, uint8_t* headers,
                          uint64_t* header_off, uint8_t* bases, uint64_t* base_off, uint8_t* quals, uint64_t bytes_cap, uint64_t records_cap,
                          leon_fastq_split_result* res);

/* -- FASTA text split into records --
 * The text begins at a record start.  Lines end at '\n'; one '\r' directly in front of the '\n' is dropped, a '\r' anywhere else is
 * kept; with last != 0 the end of the text ends a line that has no '\n' (that line keeps a '\r' at its end).  A HEADER line is a
 * non-empty line whose first byte is '>'; every other line is a SEQUENCE line, whatever it holds.  Record r is the r-th header line
 * and the sequence lines behind it, up to the next header line.  A record is WHOLE when the header line that follows it has its first
 * byte inside the text (the rest of that line may be missing); with last != 0 the end of the text ends a record as well; without it
 * the text's last record is never whole.  `wrap` says which whole records are REGULAR:
 *   wrap = W > 0, the file's line width: the record has at least one sequence line   (else LEON_FASTA_R_NO_SEQUENCE),
 *                 none of its lines is empty                                          (else LEON_FASTA_R_EMPTY_LINE),
 *                 every sequence line but its last has exactly W bytes, the last one 1 .. W   (else LEON_FASTA_R_WIDTH);
 *   wrap = 0, no width seen yet: the record has exactly one sequence line (none: LEON_FASTA_R_NO_SEQUENCE; a first line that is not
 *                 the last: LEON_FASTA_R_MULTILINE) and that line is not empty       (else LEON_FASTA_R_EMPTY_LINE);
 *   wrap = LEON_FASTA_ANY_WIDTH, the file's width is lost already: every whole record is regular, empty lines contribute nothing, a
 *                 record without sequence lines has 0 bases.
 * A text that is not empty and does not begin with '>' breaks LEON_FASTA_R_HEADER under every wrap: its record 0 is what lies in front
 * of the first header line; no other record can break that rule.  `reason` is the one of record n_records' first offending line (a
 * record without sequence: its header line); on one line, empty comes before width and before multi-line.
 * The call splits the longest prefix of records that are whole, regular and at most max_records, nothing after it: the header lines
 * without their '>' back to back, the sequence lines back to back -- a record's lines joined --, header_off[n_records + 1] and
 * base_off[n_records + 1] beginning with 0.  There are no qualities.  `stop`:
 *   LEON_FASTA_MAX        n_records == max_records;
 *   LEON_FASTA_IRREGULAR  record n_records is whole and not regular: the caller's parser is its judge.  next_header is the first byte
 *                         of the header line behind that record, n_text when the text has none: the record is text[consumed, next_header);
 *   LEON_FASTA_END        the text ran out: what is left is no whole record, or nothing.
 * `consumed` is the first byte of record n_records' header line (n_text when every record was split, which takes last != 0).
 * single_max: the longest sequence among the split records that sat on ONE line (0: none did).  next_header is 0 unless the stop is
 * LEON_FASTA_IRREGULAR.
 * bytes_cap: the room of each blob; records_cap: the entries of each offset table.  LEON_E_OVERFLOW when header_bytes or base_bytes is
 * above bytes_cap or n_records + 1 above records_cap (the result says what is needed; what the blobs and tables hold is not defined
 * then, their ends are respected): a caller with bytes_cap >= n_text and records_cap >= n_text / 2 + 2 never sees it.  LEON_E_INVALID:
 * null pointers, n_text >= 2^32.  Whatever else the text holds is data, never an error.
 * The device form (fastq_kernels.hip: k_fq_newlines, k_fa_lines, k_fa_heads, k_fa_offsets, k_fa_split) takes every pointer but `res` in
 * DEVICE memory, no alignment asked, works on a stream of its own and is complete on return; nothing outside the text is read, nothing
 * behind header_bytes / base_bytes / n_records + 1 entries is written.  The host form is the same contract in plain serial code
 * (host_fasta.h) and needs no GPU.  Errors: leon_last_error(NULL). */
#define LEON_FASTA_ANY_WIDTH (~(uint64_t)0)
#define LEON_FASTA_MAX 0u
#define LEON_FASTA_END 1u
#define LEON_FASTA_IRREGULAR 2u
#define LEON_FASTA_R_NONE 0u
#define LEON_FASTA_R_HEADER 1u
#define LEON_FASTA_R_NO_SEQUENCE 2u
#define LEON_FASTA_R_EMPTY_LINE 3u
#define LEON_FASTA_R_WIDTH 4u
#define LEON_FASTA_R_MULTILINE 5u
typedef struct leon_fasta_split_result {
    uint64_t n_records;      /* records 0 .. n_records-1 were split */
    uint64_t consumed;       /* bytes of text they occupy: record n_records' header line begins at text[consumed] */
    uint64_t header_bytes, base_bytes;
    uint32_t stop;           /* LEON_FASTA_MAX, LEON_FASTA_END or LEON_FASTA_IRREGULAR */
    uint32_t reason;         /* under LEON_FASTA_IRREGULAR: the LEON_FASTA_R_* rule record n_records broke; else LEON_FASTA_R_NONE */
    uint64_t single_max;     /* the longest sequence among the split records that sat on one line */
    uint64_t next_header;    /* under LEON_FASTA_IRREGULAR: where the record behind record n_records begins, or n_text */
} leon_fasta_split_result;
int leon_fasta_split_device(int device_id, const uint8_t* d_text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap,
                            uint8_t* d_headers, uint64_t* d_header_off, uint8_t* d_bases, uint64_t* d_base_off, uint64_t bytes_cap,
                            uint64_t records_cap, leon_fasta_split_result* res);
int leon_host_fasta_split(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap, uint8_t* headers,
                          uint64_t* header_off, uint8_t* bases, uint64_t* base_off, uint64_t bytes_cap, uint64_t records_cap,
                          leon_fasta_split_result* res);

/* -- every sequence letter kept: lower-case runs and bytes outside ACGTN --
 * For the n_bytes bases at d_bases (the reads' bases one after another): a RUN is a maximal interval [begin, end) of bytes in
 * 'a'..'z'; an ODD byte is one that, folded to upper case when it is lower-case, is none of A C G T N; the FOLDED buffer holds the
 * upper-case form where that is one of A C G T N and 'N' elsewhere -- what the DNA coder can carry.  Positions are relative to
 * d_bases, which may have any alignment; the tables are HOST memory; nothing outside [d_bases, d_bases + n_bytes) is read or written.
 * The three device calls take no context, work on a stream of their own and are complete on return (letters_kernels.hip).
 * count: the runs and odd bytes of the buffer; writes nothing to it.
 * take:  runs (2 * n_runs words: begin, end), odd_pos and odd_byte (the ORIGINAL bytes) in ascending position, and folds d_bases in
 *        place.  LEON_E_STATE when the buffer does not hold exactly n_runs runs and n_odd odd bytes: nothing has changed then.
 * apply: the inverse on a folded (decoded) buffer: inside every run a byte in 'A'..'Z' gets | 0x20, then every odd record overwrites
 *        its position.  Both forms check the tables before anything is touched and refuse with LEON_E_INVALID and the same words:
 *        begin < end <= n_bytes, runs ascending and not overlapping (end[i] <= begin[i + 1]), odd_pos strictly ascending and
 *        < n_bytes, null pointers with non-zero counts.
 * n_bytes == 0 and empty tables are LEON_OK without a launch.  Errors: leon_last_error(NULL). */
int leon_letters_count_device(int device_id, const uint8_t* d_bases, uint64_t n_bytes, uint64_t* n_runs, uint64_t* n_odd);
int leon_letters_take_device(int device_id, uint8_t* d_bases, uint64_t n_bytes, uint64_t* runs, uint64_t n_runs, uint64_t* odd_pos, uint8_t* odd_byte,
                             uint64_t n_odd);
int leon_letters_apply_device(int device_id, uint8_t* d_bases, uint64_t n_bytes, const uint64_t* runs, uint64_t n_runs, const uint64_t* odd_pos,
                              const uint8_t* odd_byte, uint64_t n_odd);
/* apply on n_threads host threads (0 = all this process may use); needs no GPU */
int leon_host_letters_apply(uint8_t* bases, uint64_t n_bytes, const uint64_t* runs, uint64_t n_runs, const uint64_t* odd_pos, const uint8_t* odd_byte,
                            uint64_t n_odd, uint32_t n_threads);

/* Start a new output file on the same context: forgets the anchor dictionary, the dictionary stream and the
 * read/block counters (a fresh Leon object upstream); keeps the bloom and the device buffers. */
int leon_dna_reset_stream(leon_dna_ctx* ctx);

int leon_dna_get_stats(const leon_dna_ctx* ctx, leon_dna_stats* out);

/* Measurement hook (profiles/scripts/walk_order.py): the NEXT batch's reads are walked in the order of d_keys (one 48-bit key
 * per read of the batch, device memory, the caller's until the call returns) instead of the order of their anchors' addresses.
 * Changes which lanes share bloom sectors, never the bytes: walk events are indexed by read position. */
int leon_dna_debug_walk_order(leon_dna_ctx* ctx, const uint64_t* d_keys);

/* -- traces of the last batch (need LEON_F_KEEP_TRACE); for stage-wise parity tests -- */
int leon_dna_trace_anchors(leon_dna_ctx* ctx, int32_t* anchor_pos, uint32_t* anchor_addr, uint8_t* flags,
                           uint64_t n_reads);
int leon_dna_trace_events(leon_dna_ctx* ctx, uint8_t* events, uint64_t n_bases);
int leon_dna_anchor_kmers(leon_dna_ctx* ctx, uint64_t* kmers, uint64_t n_anchors);

/* -- RangeEncoder::encode over independent symbol streams (one Order0Model set per stream) --
 * syms: 2 bytes per symbol (model id, value); stream i covers symbols [begin[i], begin[i+1]).
 * model ids as in DESIGN.md (8 small models, 8 numeric groups x 9).  Output concatenated, sizes[i]. */
int leon_rc_encode_streams(leon_dna_ctx* ctx, const uint8_t* syms, const uint64_t* begin, uint64_t n_streams,
                           uint8_t* out, uint64_t out_cap, uint64_t* sizes);

#ifdef __cplusplus
}
#endif
#endif
