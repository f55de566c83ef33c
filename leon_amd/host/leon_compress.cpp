// leon_compress.cpp -- `leon -c` (see leon_host.hpp).  One pass over the input, batch by batch.  A batch is cut into records by the host
// parser (bank.hpp: its blobs are in host memory) or, under `-record-parse device`, split on the device (fastq_reader.hpp: they are in
// device memory); the pass sees a BatchView either way and every consumer takes each blob where it lies:
//      headers  -> leon_header_encode_batch / _device  -> leon/header/block_<i>
//      bases    -> appended to a device-resident copy of the reads per GPU (never all of it on the host)
//      qualities, -lossless -> leon/qual/block_<i>, by the encoder `-qual-deflate` picks: zlib on the host threads
//                 (leon_host_qual_encode_blocks) or the device's deflate (leon_qual_deflate_blocks_device)
//      qualities, lossy (the default) -> resident on device 0 beside the bases, while they fit (LEON_QUAL_RESIDENT_MB)
//      -checksum: a CRC-32 per block and stream, on the device or the host threads, wherever the bytes are
//    then: solid k-mers of the resident reads (leon_kmer_solid_device, automatic threshold unless -abundance) -> bloom ->
//      leon_dna_encode_batch_device over the resident reads -> leon/dna/block_<i>, anchor dictionary, bloom, tables;
//      lossy qualities need the bloom: smoothed on the device (leon_qual_smooth_batch_device) where they are resident, else fed
//      through from a second pass over the file; then the same blocks by the same encoders.
#include "leon_internal.hpp"

#include "bank.hpp"
#include "fastq_reader.hpp"

#include <zlib.h>

#include <future>
#include <iostream>
#include <map>
#include <mutex>

namespace leon_host {
namespace {

using namespace layout;

// One stream's blocks on their way into the container (Leon::writeBlock / writeBlockLena).  Blocks of one stream come from
// one thread in increasing id, or -- DNA blocks of a multi-GPU run -- from one thread per GPU with disjoint ids.  `in_order`: such a
// run's blocks are written in increasing id all the same -- a block that arrives ahead of its turn waits in `ahead` -- so that the
// container is the bytes `-gpus 1` writes (the file's layout follows the order in which its datasets are made).
struct StreamWriter {
    Container* out = nullptr;
    std::mutex* mu = nullptr;
    const char* group = nullptr;
    std::vector<uint64_t> sizes, reads;          // per block id
    uint64_t bytes = 0;
    std::string error;
    bool in_order = false;
    uint64_t next_id = 0;
    std::map<uint64_t, std::pair<std::vector<uint8_t>, uint32_t>> ahead;
    void put(uint64_t block_id, const uint8_t* payload, uint64_t size, uint32_t n_reads) {
        if (block_id >= sizes.size()) { sizes.resize(block_id + 1, ~0ull); reads.resize(block_id + 1, 0); }
        out->putBytes(Container::blockPath(group, block_id), payload, size);
        sizes[block_id] = size; reads[block_id] = n_reads; bytes += size;
    }
    static int sink(void* user, uint64_t block_id, const uint8_t* payload, uint64_t size, uint32_t n_reads) {
        StreamWriter* w = static_cast<StreamWriter*>(user);
        try {
            std::lock_guard<std::mutex> g(*w->mu);
            if ((block_id < w->sizes.size() && w->sizes[block_id] != ~0ull) || w->ahead.count(block_id)) throw Exception("block " + std::to_string(block_id) + " arrived twice");
            if (w->in_order && block_id != w->next_id) { w->ahead[block_id] = std::make_pair(std::vector<uint8_t>(payload, payload + size), n_reads); return 0; }
            w->put(block_id, payload, size, n_reads);
            if (w->in_order)
                for (w->next_id++; !w->ahead.empty() && w->ahead.begin()->first == w->next_id; w->next_id++) {
                    const auto& b = w->ahead.begin()->second;
                    w->put(w->next_id, b.first.data(), b.first.size(), b.second);
                    w->ahead.erase(w->ahead.begin());
                }
            return 0;
        } catch (const std::exception& e) {        // no exception may cross the C boundary
            w->error = e.what();
            return 1;
        }
    }
    void complete(uint64_t n_blocks, const char* what) const {
        if (sizes.size() != n_blocks) throw Exception(std::string(what) + ": " + std::to_string(sizes.size()) + " blocks written, " + std::to_string(n_blocks) + " expected");
        for (uint64_t s : sizes) if (s == ~0ull) throw Exception(std::string(what) + ": a block is missing");
    }
    // the stream's block table: payload bytes, reads, and a third column per block
    std::vector<uint64_t> table(const std::vector<uint64_t>& third) const {
        std::vector<uint64_t> t;
        for (size_t b = 0; b < third.size(); b++) { t.push_back(sizes[b]); t.push_back(reads[b]); t.push_back(third[b]); }
        return t;
    }
};
void check_sink(leon_dna_ctx* ctx, int rc, const StreamWriter& w, const char* what) {
    if (rc == LEON_E_SINK && !w.error.empty()) throw Exception(std::string(what) + ": " + w.error);
    check(ctx, rc, what);
}

// the reads' bases, resident in HBM on one device: appended batch by batch, offsets kept on the host until the pass ends
struct ResidentReads {
    int device = 0;
    DeviceMem bases, off;
    uint64_t cap = 0, n_bases = 0;
    uint8_t* d_bases() const { return bases.as<uint8_t>(); }
    uint64_t* d_off() const { return off.as<uint64_t>(); }
    void reserve(uint64_t need) {
        if (need <= cap) return;
        const uint64_t nc = std::max<uint64_t>(need + need / 4, 1ull << 26);
        DeviceMem grown;
        grown.alloc(device, nc + 64);
        if (n_bases) check(nullptr, leon_device_copy(device, grown.get(), bases.get(), n_bases), "leon_device_copy");
        bases = std::move(grown); cap = nc;
    }
    void append(const Blob& text) {                              // text.dev: memory of the same device
        reserve(n_bases + text.bytes);
        if (text.dev && text.bytes) check(nullptr, leon_device_copy(device, d_bases() + n_bases, text.dev, text.bytes), "leon_device_copy");
        if (!text.dev) check(nullptr, leon_device_upload(device, d_bases() + n_bases, text.host, text.bytes), "leon_device_upload");
        n_bases += text.bytes;
    }
    void set_offsets(const std::vector<uint64_t>& offsets) {
        off.alloc(device, offsets.size() * 8);
        check(nullptr, leon_device_upload(device, off.get(), offsets.data(), offsets.size() * 8), "leon_device_upload");
    }
};

size_t deflated_size(const std::string& text, int strategy) {
    z_stream z{};
    if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15, 8, strategy) != Z_OK) return 0;
    std::vector<uint8_t> out(deflateBound(&z, (uLong)text.size()));
    z.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(text.data())); z.avail_in = (uInt)text.size();
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    const int rc = deflate(&z, Z_FINISH);
    const size_t n = rc == Z_STREAM_END ? (size_t)z.total_out : 0;
    deflateEnd(&z);
    return n;
}
bool runs_are_enough(const char* quals, const uint64_t* off, uint64_t n_reads) {
    std::string text;
    for (uint64_t r = 0; r < n_reads && text.size() < (256u << 10); r++) { text.append(quals + (off[r] - off[0]), off[r + 1] - off[r]); text.push_back('\n'); }
    if (text.size() < 1024) return true;
    const size_t d = deflated_size(text, Z_DEFAULT_STRATEGY), r = deflated_size(text, Z_RLE);
    return d && r && (double)r <= 1.02 * (double)d;
}

// A blob's bytes in memory of `device`: where they lie, or uploaded into `room`.  On the host: where they lie, or downloaded into `room`.
// (A blob is on `device` when it is on a device at all: the device reader splits on device 0 of the run.)
const void* on_device(const Blob& b, int device, ScratchMem& room) {
    if (b.dev) return b.dev;
    void* const d = room.fit(device, b.bytes);
    if (b.bytes) check(nullptr, leon_device_upload(device, d, b.host, b.bytes), "leon_device_upload");
    return d;
}
const char* on_host(const Blob& b, int device, std::string& room) {
    if (b.host) return b.host;
    room.resize(b.bytes);
    if (b.bytes) check(nullptr, leon_device_download(device, &room[0], b.dev, b.bytes), "leon_device_download");
    return room.data();
}

// a job that runs beside the pass is never left running over what it reads
template <class T> struct Join { std::future<T>& f; ~Join() { if (f.valid()) { try { f.get(); } catch (...) {} } } };

// `-c` from the first byte read to the last line printed; the stages below run in the order of run()
struct Compressor {
    Leon& o;                                                     // the options
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    const uint32_t k, rpb = Leon::READ_PER_BLOCK, cores;
    const int n_gpus;
    uint64_t batch_reads = 64ull * rpb;                         // a batch of the pass over the file: LEON_BATCH_BLOCKS (test aid) blocks, 64 by default
    Choice qual_enc = Choice::Host;
    const bool checksum;
    Bank bank;
    std::unique_ptr<FastqDeviceReader> dreader;                  // `-record-parse device`: the records are split on the device
    bool fastq = false, keep_header = false, keep_qual = false;
    std::string tmp_name;                                        // renamed at the very end: a failed run leaves no .leon behind
    struct TmpGuard { std::string p; bool keep = false; ~TmpGuard() { if (!keep) std::remove(p.c_str()); } } guard;
    std::unique_ptr<Container> out;
    std::mutex out_mu;
    StreamWriter wh, wd, wq;
    std::vector<std::unique_ptr<ResidentReads>> store;             // one resident copy of the reads per GPU
    int dev0 = 0;                                                // store[0]'s device: the headers', the qualities', the k-mers'
    // Lossy qualities need the bloom, which needs the whole file: they stay resident on device 0 (one byte per base, indexed
    // like the bases) until then, unless the file is too large for that (LEON_QUAL_RESIDENT_MB, default 64 GB): then a
    // second pass over the file feeds them through.
    std::unique_ptr<ResidentReads> qstore;
    bool qstore_used = false;
    uint64_t qual_resident_max = 0;
    std::vector<uint64_t> offsets{0};                            // base offsets of every read, absolute in the resident copy
    std::string first_header;
    uint64_t n_reads = 0, n_blocks = 0, n_bases = 0, header_bytes = 0, qual_bytes = 0;
    std::vector<uint64_t> hdr_text;                              // bytes of header text per read block: the decoder sizes its buffers from it
    bool qual_on_device = false;
    ScratchMem d_qbuf;                                        // a batch's qualities on the device, for its deflate or smoothing (one job at a time uses it)
    std::string h_qbuf;                                          // ... and on the host, for zlib, when they were split on the device
    ReadBatch buffers[2];                                        // the reader's two batches: the host parser's,
    DeviceBatch dbuffers[2];                                     // or the device reader's
    double w_reader = 0, w_headers = 0, w_quals = 0, w_uploads = 0;   // where the pass's own thread spent its time (-verbose)
    // `-checksum`: a CRC-32 per read block and stream (leon/metadata/checksums), each taken where the bytes lie
    std::vector<uint32_t> sum_dna, sum_hdr, sum_qual;            // per block; the jobs of a batch fill their blocks' words
    std::vector<uint64_t> file_block_off;
    std::vector<uint64_t> letter_runs, letter_odd_pos;           // begin, end pairs; positions in the file's bases
    std::vector<uint8_t> letter_odd_bytes;
    double t_parse = 0, t_kmers = 0, t_bloom = 0, t_encode = 0;
    uint64_t hist[256] = {0};
    DeviceMem d_solid; uint64_t n_solid = 0;
    uint32_t abundance = 0;
    uint64_t tai = 0, batch_blocks = 1;
    std::vector<CtxPtr> ctx;
    std::vector<uint8_t> bloom;
    const uint8_t* dict = nullptr; uint64_t dict_size = 0, n_anchors = 0;
    std::vector<uint64_t> dict_piece_table;                      // -dict-pieces: what leon/anchors/dict_piece_table gets
    // The jobs that run beside the pass read the members above (the batch buffers, d_qbuf, the writers) in place: they are the last
    // members, so they are joined before anything they read goes.
    std::future<void> qual_job, hdr_sum_job;
    Join<void> join_quals{qual_job}, join_sums{hdr_sum_job};

    explicit Compressor(Leon& leon);
    void run();
    void pass_over_file();
    void header_sums(const BatchView& batch, uint64_t got, uint64_t block0);
    void start_lossless_quals(const BatchView& batch, uint64_t got, uint64_t block0);
    void take_letters();
    void kmers_and_bloom();
    void encode_dna();
    void pick_qual_encoder(const BatchView& batch, uint64_t n);
    Blob stage_quals(const BatchView& batch, uint64_t got, uint64_t block0, std::string& room);
    void deflate_blocks(const Blob& quals, const uint64_t* off, uint64_t got, uint64_t first_block);
    void lossy_quals_resident();
    void lossy_quals_second_pass();
    void write_tables();
    void report();
    bool has_letters() const { return !letter_runs.empty() || !letter_odd_pos.empty(); }
};

Compressor::Compressor(Leon& leon)
    : o(leon), k((uint32_t)leon._kmerSize), cores((uint32_t)leon._nbCores), n_gpus(leon._gpus),
      checksum(leon._checksum), bank(leon._inputFilename, input_inflate_device(leon._inputInflate, leon._inputFilename), leon._verbose) {
    fastq = bank.isFastq();
    keep_header = !o._noHeader; keep_qual = fastq && !o._noQual;
    if (const char* e = getenv("LEON_BATCH_BLOCKS")) { const long v = atol(e); if (v > 0) batch_reads = (uint64_t)v * rpb; }   // (tests: several batches on a small file)
    // X.fastq.gz -> X.fastq.leon, data/toy.fasta -> data/toy.fasta.leon (/root/reference/scripts/simple_test.sh:51,54, INSTALL:21-23)
    std::string stem = o._inputFilename;
    if (ends_with(stem, ".gz")) stem.resize(stem.size() - 3);
    o._outputFilename = stem + ".leon";
    tmp_name = o._outputFilename + ".tmp";
    guard.p = tmp_name;
    out.reset(new Container(tmp_name, Container::CREATE));
    wh.out = wd.out = wq.out = out.get(); wh.mu = wd.mu = wq.mu = &out_mu;
    wh.group = GROUP_HEADER; wd.group = GROUP_DNA; wq.group = GROUP_QUAL;
    wd.in_order = n_gpus > 1;
    for (int g = 0; g < n_gpus; g++) { store.emplace_back(new ResidentReads()); store.back()->device = device_for(g); }
    dev0 = store[0]->device;
    if (record_parse_on_device(o._recordParse)) {
        // (FASTA goes to the device under `-record-parse-fasta` only, DESIGN.md 4.17: `-record-parse device` alone keeps its meaning)
        const char* host_why = !fastq && !o._recordParseFasta ? "FASTA input" : bank.isGzip() ? "gzip input that is not inflated on the device" : nullptr;
        if (!host_why) {
            const bool bgzf = bank.inflatesOnDevice();
            bank.dropSource();                                   // (it has said what the file is; the device reader reads it from its first byte)
            dreader.reset(new FastqDeviceReader(o._inputFilename, dev0, bgzf, o._verbose, !fastq));
        }
        if (o._verbose && host_why) std::cout << "parse: records cut on the host (" << host_why << ")" << std::endl;
        if (o._verbose && !host_why) std::cout << "parse: records split on the device (" << (fastq ? "k_fq_split" : "k_fa_split") << "), spans of " << dreader->spanBytes() << " bytes" << std::endl;
    }
}

void Compressor::run() {
    pass_over_file();
    kmers_and_bloom();
    encode_dna();
    // lossy qualities (the default): smoothed against the bloom on the device, then the same zlib blocks
    if (keep_qual && !o._lossless && qstore && qstore->n_bases == n_bases) lossy_quals_resident();
    else if (keep_qual && !o._lossless) lossy_quals_second_pass();
    write_tables();
    report();
}

// `-checksum`: the headers' words.  Of headers in device memory, there; of the host parser's, on the host threads by a job of their own,
// beside the next batch's parsing: the pass's thread is its bottleneck.  (Reads the batch's buffer in place, like qual_job: joined
// before the reader gets it back.)
void Compressor::header_sums(const BatchView& batch, uint64_t got, uint64_t block0) {
    const Blob headers = batch.headers;
    const uint64_t* const hoff = batch.header_off;
    uint32_t* sums = sum_hdr.data() + block0;
    if (headers.dev) {                                           // (no bytes: the words stay 0, the CRC of nothing)
        const std::vector<uint64_t> boff = block_offsets(hoff, got, rpb);
        if (headers.bytes) sums_on_device(dev0, headers.dev, headers.bytes, boff.data(), boff.size() - 1, sums);
        return;
    }
    const uint32_t n_thr = cores;
    hdr_sum_job = std::async(std::launch::async, [headers, hoff, got, n_thr, sums] {
        const std::vector<uint64_t> boff = block_offsets(hoff, got, Leon::READ_PER_BLOCK);
        sums_on_host(headers.host, headers.bytes, boff.data(), boff.size() - 1, n_thr, sums);
    });
}

// `-lossless`: the batch's quality blocks, deflated while the next batch is being parsed: on the device, or on the host threads
void Compressor::start_lossless_quals(const BatchView& batch, uint64_t got, uint64_t block0) {
    if (n_reads == 0) pick_qual_encoder(batch, got);
    // (the host parser's are read in place: moving the strings out would make the reader allocate and fault in half a gigabyte per
    // batch -- 0.23 s of every batch at 100 M reads when this path did)
    qual_job = std::async(std::launch::async, [this, batch, got, block0] {
        deflate_blocks(stage_quals(batch, got, block0, h_qbuf), batch.qual_off, got, block0);
    });
}

// A batch's qualities on their way into blocks: to where the picked encoder reads them -- device memory (d_qbuf when they have to be
// uploaded) or the host (`room` when they have to be downloaded) --, the `-checksum` words taken on the device when the bytes are or
// have just been put there, else on the host threads.  What comes back says where the encoder finds them.
Blob Compressor::stage_quals(const BatchView& batch, uint64_t got, uint64_t block0, std::string& room) {
    Blob q = batch.quals;
    if (qual_on_device) q.dev = on_device(q, dev0, d_qbuf);
    if (checksum) {
        const std::vector<uint64_t> boff = block_offsets(batch.qual_off, got, rpb);
        if (q.dev) sums_on_device(dev0, q.dev, q.bytes, boff.data(), boff.size() - 1, sum_qual.data() + block0);
        else sums_on_host(q.host, q.bytes, boff.data(), boff.size() - 1, cores, sum_qual.data() + block0);
    }
    if (!qual_on_device) q.host = on_host(q, dev0, room);
    return q;
}

void Compressor::pass_over_file() {
    qual_enc = qual_encoder_choice(o._qualDeflate);
    qual_resident_max = 64ull << 30;
    if (const char* e = getenv("LEON_QUAL_RESIDENT_MB")) qual_resident_max = (uint64_t)std::max<long long>(0, atoll(e)) << 20;
    if (fastq && !o._noQual && !o._lossless && qual_resident_max) { qstore.reset(new ResidentReads()); qstore->device = dev0; }
    qstore_used = qstore != nullptr;
    CtxPtr hdr_ctx;
    if (keep_header) hdr_ctx = make_ctx(k, 1000, dev0);
    // the reader runs one batch ahead on its own thread: batch i + 1 is parsed while batch i's headers are coded on the device
    // and its bases (and qualities) cross to it -- or, split on the device, are copied there
    const uint64_t want = batch_reads;
    std::function<BatchView(uint32_t)> parse_next;               // fills buffer i of the reader's kind
    if (dreader) parse_next = [r = dreader.get(), b = dbuffers, want](uint32_t i) { r->next(b[i], want); return b[i].view(); };
    else parse_next = [r = &bank, b = buffers, want](uint32_t i) { b[i].clear(); r->next(b[i], want); return b[i].view(); };
    std::future<BatchView> parsing = std::async(std::launch::async, parse_next, 0u);
    Join<BatchView> parse_join{parsing};                         // (never left running over dead buffers)
    ScratchMem d_header_off;
    std::string host_bases;
    for (uint32_t cur = 0;; cur ^= 1) {
        auto t_w = std::chrono::steady_clock::now();
        const BatchView batch = parsing.get();                   // (the reader's exceptions surface here)
        const uint64_t got = batch.n;
        w_reader += seconds_since(t_w);
        if (!got) break;
        // the quality blocks of the batch before read this buffer's twin in place: they are done (they started a whole batch ago)
        // before the reader is allowed to fill it again
        t_w = std::chrono::steady_clock::now();
        if (qual_job.valid()) qual_job.get();
        if (hdr_sum_job.valid()) hdr_sum_job.get();
        w_quals += seconds_since(t_w);
        if (got == batch_reads) parsing = std::async(std::launch::async, parse_next, cur ^ 1);
        if (n_reads == 0) first_header = dreader ? dreader->firstHeader() : std::string(batch.headers.host, batch.header_off[1]);
        const uint64_t batch_blocks_n = (got + rpb - 1) / rpb, batch_block0 = n_reads / rpb;
        if (checksum) { sum_hdr.resize(batch_block0 + batch_blocks_n, 0); sum_qual.resize(batch_block0 + batch_blocks_n, 0); }   // (no job is running: both were joined above)
        t_w = std::chrono::steady_clock::now();
        if (keep_header && checksum) header_sums(batch, got, batch_block0);
        if (keep_header) {
            const uint8_t* const first = reinterpret_cast<const uint8_t*>(first_header.data());
            if (batch.headers.dev) {
                uint64_t* const d_off = static_cast<uint64_t*>(d_header_off.fit(dev0, (got + 1) * 8));
                check(nullptr, leon_device_upload(dev0, d_off, batch.header_off, (got + 1) * 8), "leon_device_upload");
                check_sink(hdr_ctx.get(), leon_header_encode_batch_device(hdr_ctx.get(), static_cast<const uint8_t*>(batch.headers.dev), d_off, got, n_reads, first, first_header.size(),
                                                                          StreamWriter::sink, &wh),
                           wh, "leon_header_encode_batch_device");
            } else
                check_sink(hdr_ctx.get(), leon_header_encode_batch(hdr_ctx.get(), reinterpret_cast<const uint8_t*>(batch.headers.host), batch.header_off, got, n_reads, first,
                                                                   first_header.size(), StreamWriter::sink, &wh),
                           wh, "leon_header_encode_batch");
            header_bytes += batch.headers.bytes;
            for (uint64_t r = 0; r < got; r += rpb) hdr_text.push_back(batch.header_off[std::min<uint64_t>(got, r + rpb)] - batch.header_off[r]);   // (batches are whole blocks but the last)
        }
        w_headers += seconds_since(t_w);
        qual_bytes += batch.quals.bytes;
        t_w = std::chrono::steady_clock::now();
        if (keep_qual && o._lossless) start_lossless_quals(batch, got, batch_block0);
        w_quals += seconds_since(t_w);
        t_w = std::chrono::steady_clock::now();
        Blob through_host = batch.bases;                         // for the devices the bases are not on: downloaded once if they have to be
        through_host.dev = nullptr;
        for (auto& st : store) {
            if (batch.bases.dev && st->device == dev0) { st->append(batch.bases); continue; }
            if (!through_host.host) through_host.host = on_host(batch.bases, dev0, host_bases);
            st->append(through_host);
        }
        if (qstore) {                                            // lossy mode: the qualities wait in HBM, beside the bases, for the bloom
            try { qstore->append(batch.quals); }
            catch (const Exception&) { qstore.reset(); }         // no room: they are read again from the file afterwards
            if (qstore && qstore->n_bases > qual_resident_max) qstore.reset();
        }
        for (uint64_t i = 1; i <= got; i++) offsets.push_back(offsets[n_reads] + batch.base_off[i]);
        w_uploads += seconds_since(t_w);
        n_reads += got;
        if (got < batch_reads) break;                            // the partial batch is the last one
    }
    hdr_ctx.reset();
    if (qual_job.valid()) qual_job.get();
    if (hdr_sum_job.valid()) hdr_sum_job.get();
    n_blocks = (n_reads + rpb - 1) / rpb; n_bases = offsets.back();
    for (auto& st : store) st->set_offsets(offsets);
    // `-checksum`: the bases' words from device 0's resident copy; the lossy qualities' once they are smoothed
    if (checksum) {
        file_block_off = block_offsets(offsets.data(), n_reads, rpb);
        sum_dna.assign(n_blocks, 0); sum_hdr.resize(n_blocks, 0); sum_qual.resize(n_blocks, 0);
        sums_on_device(dev0, store[0]->d_bases(), n_bases, file_block_off.data(), n_blocks, sum_dna.data());
    }
    if (o._letters) take_letters();
    t_parse = seconds_since(t_start);
}

// `-letters`: lower-case runs and bytes outside ACGTN out of every device's resident copy, which is folded to what the coder carries
// (DESIGN.md 4.12).  Behind the checksum: the stored digest is of the ORIGINAL bytes.  Slices of at most 1 GiB bound the calls' tables.
void Compressor::take_letters() {
    uint64_t slice = 1ull << 30;
    if (const char* e = getenv("LEON_LETTERS_SLICE")) { const long long v = atoll(e); if (v > 0) slice = (uint64_t)v; }   // (tests: several slices on a small file)
    std::vector<uint64_t> runs, pos;
    std::vector<uint8_t> bytes;
    for (size_t g = 0; g < store.size(); g++)
        for (uint64_t at = 0; at < n_bases; at += slice) {
            const uint64_t nb = std::min(slice, n_bases - at);
            uint64_t nr = 0, no = 0;
            check(nullptr, leon_letters_count_device(store[g]->device, store[g]->d_bases() + at, nb, &nr, &no), "leon_letters_count_device");
            if (!nr && !no) continue;
            runs.resize(2 * nr); pos.resize(no); bytes.resize(no);
            check(nullptr, leon_letters_take_device(store[g]->device, store[g]->d_bases() + at, nb, runs.data(), nr, pos.data(), bytes.data(), no), "leon_letters_take_device");
            if (g) continue;                                     // the replicas hold the same bytes: device 0's tables are the file's
            for (uint64_t r = 0; r < nr; r++) {
                if (r == 0 && !letter_runs.empty() && letter_runs.back() == at && runs[0] == 0) letter_runs.back() = at + runs[1];   // a run across the slices' join
                else { letter_runs.push_back(at + runs[2 * r]); letter_runs.push_back(at + runs[2 * r + 1]); }
            }
            for (uint64_t i = 0; i < no; i++) letter_odd_pos.push_back(at + pos[i]);
            letter_odd_bytes.insert(letter_odd_bytes.end(), bytes.begin(), bytes.end());
        }
}

// solid k-mers -> bloom (Leon::executeCompression: DSK, then createBloom)
void Compressor::kmers_and_bloom() {
    const auto t_count = std::chrono::steady_clock::now();
    if (n_reads) {
        uint64_t* solid = nullptr;
        const int rc = leon_kmer_solid_device(dev0, store[0]->d_bases(), store[0]->d_off(), n_reads, k, (uint32_t)std::max(o._abundance, 0), 0, &solid, &n_solid, hist);
        d_solid.reset(solid);
        check(nullptr, rc, "leon_kmer_solid_device");
    }
    t_kmers = seconds_since(t_count);
    abundance = (uint32_t)o._abundance;
    if (o._abundance == 0) (void)leon_kmer_auto_cutoff(hist, &abundance);
    tai = std::max<uint64_t>(n_solid * 12, 1000);                // NBITS_PER_KMER = 12 [RECALLED]
    // the DNA stream goes to the device in batches of whole read blocks: the file at once up to 100 M reads, else 2 000 blocks
    // (100 M reads) per leon_dna_encode_batch_device call -- the reads stay resident in HBM, the per-batch buffers are bounded
    batch_blocks = std::max<uint64_t>(std::min<uint64_t>(n_blocks, 2000), 1);
    if (const char* e = getenv("LEON_BATCH_BLOCKS")) { const long v = atol(e); if (v > 0) batch_blocks = (uint64_t)v; }   // (tests: several batches on a small file)
    uint64_t batch_max_reads = 0, batch_max_bases = 0;
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += batch_blocks) {
        const uint64_t r0 = b0 * rpb, r1 = std::min<uint64_t>(n_reads, (b0 + batch_blocks) * rpb);
        batch_max_reads = std::max(batch_max_reads, r1 - r0); batch_max_bases = std::max(batch_max_bases, offsets[r1] - offsets[r0]);
    }
    for (int g = 0; g < n_gpus; g++) {
        ctx.push_back(make_ctx(k, tai, store[g]->device, 7, 12, Leon::READ_PER_BLOCK, o._dictPieces ? LEON_F_DICT_PIECES : 0u, o._dictPieceAnchors));
        check(ctx[g].get(), leon_dna_set_shard(ctx[g].get(), (uint32_t)g, (uint32_t)n_gpus), "leon_dna_set_shard");
        // every per-batch buffer sized now, in one go, before the bloom is built and copied: the first (usually only) encode
        // call then allocates nothing large
        check(ctx[g].get(), leon_dna_reserve(ctx[g].get(), batch_max_reads, batch_max_bases), "leon_dna_reserve");
    }
    check(ctx[0].get(), leon_dna_bloom_insert_device(ctx[0].get(), d_solid.as<uint64_t>(), n_solid), "leon_dna_bloom_insert_device");
    uint64_t bloom_bytes = 0;
    check(ctx[0].get(), leon_dna_bloom_nbytes(ctx[0].get(), &bloom_bytes), "leon_dna_bloom_nbytes");
    bloom.resize(bloom_bytes);
    check(ctx[0].get(), leon_dna_bloom_download(ctx[0].get(), bloom.data(), bloom_bytes), "leon_dna_bloom_download");
    for (int g = 1; g < n_gpus; g++) check(ctx[g].get(), leon_dna_bloom_upload(ctx[g].get(), bloom.data(), bloom_bytes), "leon_dna_bloom_upload");
    t_bloom = seconds_since(t_count);
}

// the DNA stream: Dispatcher::iterate(bank, DnaEncoder(this)) upstream, the device path here
void Compressor::encode_dna() {
    const auto t_dna = std::chrono::steady_clock::now();
    std::vector<std::string> gpu_error(n_gpus);
    auto encode_on = [&](int g) {
        try {
            for (uint64_t b0 = 0; b0 < n_blocks; b0 += batch_blocks) {
                const uint64_t r0 = b0 * rpb, r1 = std::min<uint64_t>(n_reads, (b0 + batch_blocks) * rpb);
                int rc = leon_dna_encode_batch_device(ctx[g].get(), store[g]->d_bases(), store[g]->d_off() + r0, r1 - r0, r0, StreamWriter::sink, &wd);
                check_sink(ctx[g].get(), rc, wd, "leon_dna_encode_batch_device");
            }
        } catch (const std::exception& e) { gpu_error[g] = e.what(); }
    };
    if (n_gpus == 1) encode_on(0);
    else {
        std::vector<std::thread> th;
        for (int g = 0; g < n_gpus; g++) th.emplace_back(encode_on, g);
        for (auto& t : th) t.join();
    }
    for (const std::string& e : gpu_error) if (!e.empty()) throw Exception(e);
    check(ctx[0].get(), leon_dna_finish(ctx[0].get(), &dict, &dict_size, &n_anchors), "leon_dna_finish");
    for (int g = 1; g < n_gpus; g++) { const uint8_t* d; uint64_t ds, na; check(ctx[g].get(), leon_dna_finish(ctx[g].get(), &d, &ds, &na), "leon_dna_finish"); }
    if (o._dictPieces) {                                         // the table beside the stream: the kind, anchors per piece, every piece's bytes
        const uint64_t* piece_off = nullptr; uint64_t n_pieces = 0; uint32_t piece_anchors = 0;
        check(ctx[0].get(), leon_dna_dict_pieces(ctx[0].get(), &piece_off, &n_pieces, &piece_anchors), "leon_dna_dict_pieces");
        dict_piece_table.assign(2, 0);
        dict_piece_table[0] = DICT_PIECES_ORDER0; dict_piece_table[1] = piece_anchors;
        for (uint64_t p = 0; p < n_pieces; p++) dict_piece_table.push_back(piece_off[p + 1] - piece_off[p]);
    }
    t_encode = seconds_since(t_dna);
}

// the sample that picks the encoder under `auto`: of the batch's first n reads those of the first 256 KB of lines (where runs_are_enough
// stops reading), downloaded when they are in device memory
void Compressor::pick_qual_encoder(const BatchView& batch, uint64_t n) {
    qual_on_device = qual_enc == Choice::Device;
    if (qual_enc != Choice::Auto) return;
    uint64_t m = 0;
    while (m < n && batch.qual_off[m] + m < (256u << 10)) m++;
    Blob sample = batch.quals;
    sample.bytes = batch.qual_off[m];
    std::string room;
    qual_on_device = runs_are_enough(on_host(sample, dev0, room), batch.qual_off, m);
}
// `got` reads' quality blocks into the container, by whoever was picked: from quals.dev (device memory) or quals.host
void Compressor::deflate_blocks(const Blob& quals, const uint64_t* off, uint64_t got, uint64_t first_block) {
    if (qual_on_device) {
        const int rc = leon_qual_deflate_blocks_device(dev0, static_cast<const uint8_t*>(quals.dev), off, got, Leon::READ_PER_BLOCK, StreamWriter::sink, &wq, first_block);
        check_sink(nullptr, rc, wq, "leon_qual_deflate_blocks_device");
    } else {
        const int rc = leon_host_qual_encode_blocks(reinterpret_cast<const uint8_t*>(quals.host), off, got, Leon::READ_PER_BLOCK, -1, cores, StreamWriter::sink, &wq, first_block);
        check_sink(nullptr, rc, wq, "leon_host_qual_encode_blocks");
    }
}

// The qualities are resident: smoothed where they lie, then back to the host chunk by chunk: chunk i is deflated by the host threads
// while chunk i + 1 is copied.
void Compressor::lossy_quals_resident() {
    // ONE call over the whole file: the library smooths the reads in the order of their minimizers, so that reads of the same
    // locus follow one another and share their bloom probes in cache -- which needs them all in one call
    // ... up to the DNA stream's batch size (2 000 blocks = 100 M reads: a call's work buffers grow with its reads, on top of the
    // resident bases and qualities).  A call the device has no room for is retried in halves: smoothing is idempotent (it
    // depends on the bases and on whether a quality is above '@'), and the reads' order inside a call only decides who
    // shares probes with whom, never the bytes.
    for (uint64_t r = 0, step = batch_blocks * rpb; r < n_reads;) {
        const uint64_t got = std::min<uint64_t>(step, n_reads - r);
        const int rc = leon_qual_smooth_batch_device(ctx[0].get(), store[0]->d_bases(), store[0]->d_off() + r, got, qstore->d_bases() + offsets[r]);
        if (rc == LEON_E_HIP && step > 64ull * rpb) { step = std::max<uint64_t>(64ull * rpb, (step / 2 + rpb - 1) / rpb * rpb); leon_device_trim(); continue; }
        check(ctx[0].get(), rc, "leon_qual_smooth_batch_device");
        r += got;
    }
    // what is stored, and summed under `-checksum`, is the smoothed bytes: chunk by chunk through the tail every quality batch takes
    struct { std::string quals; std::vector<uint64_t> off; } chunk[2];   // (chunk i's job reads its own while chunk i + 1 is staged)
    Join<void> join{qual_job};
    for (uint64_t r = 0, i = 0; r < n_reads; i ^= 1) {
        const uint64_t got = std::min<uint64_t>(batch_reads, n_reads - r), first_block = r / rpb;
        std::vector<uint64_t>& off = chunk[i].off;
        off.resize(got + 1);
        for (uint64_t j = 0; j <= got; j++) off[j] = offsets[r + j] - offsets[r];
        BatchView batch;
        batch.quals.dev = qstore->d_bases() + offsets[r]; batch.quals.bytes = off[got];
        batch.qual_off = off.data(); batch.n = got;
        if (r == 0) pick_qual_encoder(batch, std::min<uint64_t>(got, 4000));
        const Blob quals = stage_quals(batch, got, first_block, chunk[i].quals);
        if (qual_job.valid()) qual_job.get();
        if (qual_on_device) deflate_blocks(quals, batch.qual_off, got, first_block);       // deflated where they lie
        else qual_job = std::async(std::launch::async, [this, quals, batch, got, first_block] { deflate_blocks(quals, batch.qual_off, got, first_block); });
        r += got;
    }
    if (qual_job.valid()) qual_job.get();
    qstore.reset();
}

// The qualities did not stay on the device: a second pass over the file feeds them through, batch by batch.
void Compressor::lossy_quals_second_pass() {
    Bank again(o._inputFilename, input_inflate_device(o._inputInflate, o._inputFilename), o._verbose);      // (`-input-inflate`: the same choice)
    ReadBatch& batch = buffers[0];
    uint64_t r = 0;
    for (;;) {
        batch.clear();
        const uint64_t got = again.next(batch, batch_reads);
        if (!got) break;
        if (r + got > n_reads || batch.bases.size() != offsets[r + got] - offsets[r]) throw Exception(o._inputFilename + " changed while it was being compressed");
        uint8_t* const d_q = static_cast<uint8_t*>(d_qbuf.fit(dev0, batch.quals.size()));
        check(nullptr, leon_device_upload(dev0, d_q, batch.quals.data(), batch.quals.size()), "leon_device_upload");
        check(ctx[0].get(), leon_qual_smooth_batch_device(ctx[0].get(), store[0]->d_bases(), store[0]->d_off() + r, got, d_q), "leon_qual_smooth_batch_device");
        BatchView smoothed = batch.view();                       // on the device only: what the host holds is the file's own bytes
        smoothed.quals.host = nullptr; smoothed.quals.dev = d_q;
        if (r == 0) pick_qual_encoder(smoothed, std::min<uint64_t>(got, 4000));
        deflate_blocks(stage_quals(smoothed, got, r / rpb, batch.quals), smoothed.qual_off, got, r / rpb);   // (zlib: downloaded over them)
        r += got;
        if (got < batch_reads) break;
    }
    if (r != n_reads) throw Exception(o._inputFilename + " changed while it was being compressed");
}

void Compressor::write_tables() {
    wd.complete(n_blocks, "DNA stream");
    if (keep_header) wh.complete(n_blocks, "header stream");
    if (keep_qual) wq.complete(n_blocks, "quality stream");
    std::vector<uint64_t> blk_bases(n_blocks);
    for (uint64_t b = 0; b < n_blocks; b++) blk_bases[b] = offsets[std::min<uint64_t>(n_reads, (b + 1) * rpb)] - offsets[b * rpb];
    std::vector<uint64_t> table = wd.table(blk_bases);
    out->putU64(DS_DNA_TABLE, table.data(), table.size());
    if (keep_header) {
        table = wh.table(hdr_text);
        out->putU64(DS_HEADER_TABLE, table.data(), table.size());
        out->putBytes(DS_FIRST_HEADER, first_header.data(), first_header.size());
    }
    if (keep_qual) {
        table = wq.table(blk_bases);
        out->putU64(DS_QUAL_TABLE, table.data(), table.size());
    }
    if (fastq && keep_header && keep_qual) {                     // '+' lines that repeat the header (or carry text): `diff` sees them (simple_test.sh:62)
        const std::string plus = dreader ? dreader->parser().plusLines() : bank.plusLines();
        if (!plus.empty()) out->putBytes(DS_PLUS_LINES, plus.data(), plus.size());
    }
    if (checksum) {                                              // kind, then per block: dna, header, quality (0 for a stream the file does not have)
        table.assign(1, CHECKSUM_CRC32);
        for (uint64_t b = 0; b < n_blocks; b++) { table.push_back(sum_dna[b]); table.push_back(keep_header ? sum_hdr[b] : 0); table.push_back(keep_qual ? sum_qual[b] : 0); }
        out->putU64(DS_CHECKSUMS, table.data(), table.size());
    }
    if (has_letters()) {                                         // kind, then begin, end of every run; the odd bytes' two tables when there are any
        table.assign(1, LETTERS_RUNS_AND_BYTES);
        table.insert(table.end(), letter_runs.begin(), letter_runs.end());
        out->putU64(DS_LETTER_RUNS, table.data(), table.size());
        if (!letter_odd_pos.empty()) {
            out->putU64(DS_LETTER_ODD_POS, letter_odd_pos.data(), letter_odd_pos.size());
            out->putBytes(DS_LETTER_ODD_BYTES, letter_odd_bytes.data(), letter_odd_bytes.size());
        }
    }
    if (o._dictPieces) {
        out->putBytes(DS_ANCHOR_DICT_PIECES, dict, dict_size);
        out->putU64(DS_ANCHOR_DICT_PIECE_TABLE, dict_piece_table.data(), dict_piece_table.size());
    } else out->putBytes(DS_ANCHOR_DICT, dict, dict_size);
    out->putBytes(DS_BLOOM_BITS, bloom.data(), bloom.size());
    const uint8_t info = (uint8_t)((fastq ? 0 : INFO_FASTA) | (keep_header ? 0 : INFO_NO_HEADER) | (keep_qual ? 0 : INFO_NO_QUAL) | (o._lossless ? INFO_LOSSLESS : 0));
    out->putBytes(DS_INFOBYTE, &info, 1);
    uint64_t params[PARAM_COUNT] = {0};
    params[P_VERSION_MAJOR] = 1; params[P_VERSION_MINOR] = 1; params[P_VERSION_PATCH] = 0;       // Leon 1.1.0, /root/reference/CMakeLists.txt:9-11
    params[P_KMER_SIZE] = k; params[P_READS_PER_BLOCK] = rpb; params[P_N_READS] = n_reads; params[P_N_ANCHORS] = n_anchors;
    params[P_ABUNDANCE] = abundance; params[P_BLOOM_TAI] = tai; params[P_BLOOM_N_HASH] = 7; params[P_BLOOM_BLOCK_NBITS] = 12;
    params[P_TOTAL_BASES] = n_bases; params[P_FASTA_LINE_WIDTH] = fastq ? 0 : dreader ? dreader->parser().fastaLineWidth() : bank.fastaLineWidth();
    params[P_CONTAINER_REV] = CONTAINER_REV;
    params[P_QUAL_ENCODER] = !keep_qual ? QUAL_ENC_NONE : qual_on_device ? QUAL_ENC_DEVICE_RLE : QUAL_ENC_ZLIB;
    out->putU64(DS_PARAMS, params, PARAM_COUNT);
    out->close();
    if (std::rename(tmp_name.c_str(), o._outputFilename.c_str()) != 0) throw Exception("cannot write " + o._outputFilename);
    guard.keep = true;
}

void Compressor::report() {
    const uint64_t dna_bytes = wd.bytes + dict_size;
    std::cout << "DNA stream: " << n_reads << " reads, " << n_bases << " bases -> " << dna_bytes << " bytes (" << n_anchors << " anchors, "
              << n_blocks << " blocks, abundance threshold " << abundance << (o._abundance ? "" : " (automatic)") << ", " << n_solid << " solid k-mers)\n";
    if (keep_header) std::cout << "header stream: " << header_bytes << " bytes -> " << wh.bytes << " bytes\n";
    if (keep_qual) std::cout << "quality stream (" << (o._lossless ? "lossless" : "lossy") << "): " << qual_bytes << " bytes -> " << wq.bytes << " bytes"
                             << (qual_on_device ? " (deflated on the device: runs + dynamic Huffman codes)" : " (zlib on the host threads)") << "\n";
    if (checksum) std::cout << "checksums: CRC-32 of " << n_blocks << " blocks (dna" << (keep_header ? ", header" : "") << (keep_qual ? ", quality" : "") << ")\n";
    std::cout << "written to " << o._outputFilename << std::endl;
    if (o._verbose && o._dictPieces)
        std::cout << "dictionary: " << dict_piece_table.size() - 2 << " pieces of " << dict_piece_table[1] << " anchors on the device (k_dict_encode_pieces), " << dict_size << " bytes\n";
    if (o._verbose && o._letters) {
        const uint64_t letter_table_bytes = 8 * (1 + letter_runs.size()) + 9 * letter_odd_pos.size();
        if (has_letters()) std::cout << "letters: " << letter_runs.size() / 2 << " lower-case run(s), " << letter_odd_pos.size() << " other byte(s) kept (" << letter_table_bytes << " bytes)\n";
        else std::cout << "letters: none\n";
    }
    if (o._verbose && dreader) dreader->report();
    if (o._verbose)
        std::cout << "time: parse + headers" << (keep_qual && o._lossless ? " + qualities " : " ") << t_parse << " s, k-mer counting " << t_kmers << " s, contexts + bloom "
                  << t_bloom - t_kmers << " s, DNA encode " << t_encode << " s, total " << seconds_since(t_start) << " s\n"
                  << "the pass over the file: waited for the reader " << w_reader << " s, header blocks " << w_headers << " s, waited for the previous batch's quality blocks "
                  << w_quals << " s, bases" << (qstore_used ? " + qualities" : "") << " to the device " << w_uploads << " s" << std::endl;
}

}  // namespace

void Leon::executeCompression() {
    if (_kmerSize < 3 || _kmerSize > 63) throw Exception("-kmer-size must be in 3..63");
    Compressor(*this).run();
}

}  // namespace leon_host
