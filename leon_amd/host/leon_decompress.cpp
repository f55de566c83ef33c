// leon_decompress.cpp -- `leon -d` (see leon_host.hpp), block group by block group: leon_dna_decode_blocks (device),
// leon_host_header_decode_blocks, leon_host_qual_decode_blocks, records written as FASTA / FASTQ text.
//
// Three stages, each round through them in turn, the stages of different rounds side by side:
//   A (the caller's thread) the payloads out of the container, the DNA blocks on the device -- of `dna_rounds` rounds per device call:
//                     a call costs one block's serial chain whatever the number of blocks, so a large file makes two calls;
//   B (a task)        a round's header blocks (their symbols on the device for rounds of many blocks: the host threads are idle
//                     meanwhile) and, beside them, its quality blocks; one round at a time;
//   C (a task)        formatting and writing, in file order, once A and B of the round are done.
// A never waits for B or C of its own rounds -- only for C of rounds further back (memory).
// (Round 5, measured at configuration #3 and not kept -- profiles/r5_cli_decode_trials.txt: all four rounds in ONE call, one chain instead
// of two: 9.96 s for this stage against 7.15, `-d -test-file` 23.9 s against 20.2 -- the header and quality blocks of ALL rounds then run
// beside the call on the same 16 CPUs that stage its 15 GB of output back; and -test-file's comparison moved into the formatting threads
// (each compares its share with the original as it writes it) instead of both files read back at the end: 22.2 s.  What bounds -d on a
// box that grants 16 CPUs is the host's share -- header text 6.2 s, quality blocks 3.2-3.5 s, formatting + writing 6.8-7.8 s of all
// cores each -- not the number of device calls or where the comparison runs.)
#include "leon_internal.hpp"

#include "bank.hpp"

#include <fcntl.h>

#include <atomic>
#include <deque>
#include <future>
#include <iostream>
#include <mutex>

namespace leon_host {
namespace {

using namespace layout;

// Who rebuilds the header text of `-d`.  Not given, or `host`: the host threads (from the payloads, or from symbols the device decoded
// where a round has LEON_HEADER_DEVICE_BLOCKS blocks).  `device`: symbols and text of every header block in one device call
// (leon_header_decode_text), the rounds fetch their blocks' text; blocks the kernel declines go to the host decoder.  `auto`: the
// device for files of at least kHeaderTextAutoBlocks blocks.  The restored file is the same bytes whichever way.
// Measured with `-d -test-file`, the ways alternating (profiles/README.md): 200 blocks, the host ahead (4.3-4.6 s against 4.6-4.7: one wave's
// chain of 50 000 headers outlasts sixteen cores on 200 blocks); 1 000 blocks, the device ahead in every pair (12.6 / 13.5 / 14.3 s against
// 12.6 / 15.1 / 15.9); 2 000 blocks, by 1.4-3.2 s of 24-27.  The smallest count at which the device won:
constexpr uint64_t kHeaderTextAutoBlocks = 1000;
// Who formats the records of `-d` (lead byte, header, sequence lines, '+' line, qualities).  Not given, or `host`: the host threads
// (Decoder::write_round).  `device`: the bases never leave the device (leon_dna_decode_blocks_device), the header text stays there too under
// `-header-text device`, the qualities go up, leon_records_format_device writes the text and it comes back in pinned pieces that are
// written to the file as they are.  A file whose '+' lines are mixed is formatted on the host whatever the option says.  `auto`: the device
// for files of at least kRecordTextAutoBlocks blocks (no file today: see the constant).  The restored file is the same bytes whichever way.
// Measured with `-d` and `-d -test-file`, the ways alternating, three each (profiles/README.md): 200 blocks, the device ahead in every pair
// (3.05-3.74 s against 4.03-4.41); 1 000 blocks, ahead in four pairs of six (9.7-12.1 s against 10.8-11.9); 2 000 blocks, in five of six
// (18.1-20.8 s against 17.6-22.9).  Ahead on average everywhere, but there is no block count FROM which it was ahead in every pair, and
// that is the rule `auto` follows (as kHeaderTextAutoBlocks does): `auto` = `host` until a measurement says otherwise.
constexpr uint64_t kRecordTextAutoBlocks = ~0ull;
// Who inflates the quality blocks of `-d`.  Not given, or `host`: zlib on the host threads (leon_host_qual_decode_blocks).  `device`:
// leon_qual_inflate_blocks_device, per round, beside the DNA decode -- under `-record-text device` straight into the device buffer the
// formatter reads (the round's upload of the inflated qualities disappears; the reads' offsets, 8 bytes each, come to the host for the
// check that a read's quality and sequence lengths agree), otherwise into a buffer that is downloaded into the round's host arrays.
// A round for which the device has no memory is inflated on the host.  The restored file is the same bytes whichever way.
// The rule of kHeaderTextAutoBlocks: the smallest measured block count FROM which `device` was ahead of `host` in every alternating
// pair.  No such count has been measured (profiles/README.md, "qual_inflate": the command's runs at the three sizes are still to be
// made), so `auto` = `host` until a measurement says otherwise.
constexpr uint64_t kQualInflateAutoBlocks = ~0ull;

// bytes that are about to be overwritten anyway: std::vector would clear all of them first, on the critical path
struct RawBytes {
    std::unique_ptr<uint8_t[]> p; uint64_t n = 0;
    void resize(uint64_t want) { if (want > n) { p.reset(); p.reset(new uint8_t[want]); n = want; } }
    uint8_t* data() const { return p.get(); }
    uint64_t size() const { return n; }
};
// what one round hands from the decoding stage to the writing stage
struct DnaGroup {                                            // the DNA blocks of one device call: the bases and lengths of its rounds
    RawBytes bases; std::unique_ptr<uint32_t[]> lens;
    // `-record-text device`: the bases and lengths stay in device buffers of the call's own, until its last round is written
    DeviceMem d_bases, d_lens;
    std::atomic<uint32_t> rounds_left{0};
    void release_device() { d_bases.reset(); d_lens.reset(); }
};
struct Round {
    uint64_t read_index = 0, file_off = 0, g_reads = 0, g_bases = 0, n_text = 0, nb = 0, hdr_text_bytes = 0, block0 = 0;
    std::shared_ptr<DnaGroup> dna; uint64_t base0 = 0, read0 = 0;   // this round's share of them
    uint64_t file_base0 = 0;                                 // the round's first base in the file's bases (the letter tables' positions)
    const uint8_t* bases() const { return own_bases.p ? own_bases.p.get() : dna->bases.p.get() + base0; }
    uint8_t* d_bases() const { return dna->d_bases.as<uint8_t>() + base0; }
    bool on_device = false;                                  // `-record-text device`: the round's bases are in dna->d_bases
    bool last = false;                                       // the file's last round (`-gz`: its text closes the BGZF stream)
    bool hdr_in_set = false;                                 // ... and its header text lies in the device's header-text set:
    const uint8_t* d_hdr = nullptr; const uint64_t* d_hdr_off = nullptr; uint64_t d_hdr_size = 0;
    RawBytes own_bases;                                      // (a round that had to come back to the host: no device memory for its text)
    const uint32_t* lens() const { return dna->lens.get() + read0; }
    RawBytes hdr, qual, pay_h, pay_q;                        // (gigabytes each: never zero-filled)
    std::vector<uint64_t> off_h, off_q, blk_bases;
    std::vector<uint32_t> blk_reads;
    std::vector<uint64_t> hdr_off, qual_off;
    DeviceMem d_qual;                                        // `-qual-inflate device` under `-record-text device`: the qualities, inflated where the formatter reads them
    std::vector<uint32_t> sum_hdr, sum_qual;                 // the restored blocks' digests, taken by stage B where the bytes lay (empty: not taken)
};
typedef std::shared_ptr<Round> RoundPtr;

// what the container says about itself, checked before anything is decoded or sized from it (leon_plan.hpp)
struct Metadata {
    plan::Params p;
    bool fasta_in = false, has_header = false, has_qual = false;
    bool fastq_out = false;                                  // "-noqual ... will decompress to fasta"
    std::vector<uint64_t> tdna, thdr, tqual;                 // the block tables, 3 words per block
    std::vector<uint8_t> first_header;
    bool has_sums = false;                                   // block checksums (`-c -checksum`): verified whenever the table is there, round by round
    std::vector<uint64_t> tsum;
    // the letters the coder does not carry (`-c -letters`): put back whenever the tables are there, round by round, where
    // the decoded bases lie, before the round is verified and formatted
    bool has_letters = false;
    std::vector<uint64_t> lt_runs, lt_pos;                   // begin, end pairs (the kind word taken off); positions in the file's bases
    std::vector<uint8_t> lt_bytes;
    PlusLines plus;                                          // FASTQ '+' lines that are not bare (absent: all of them are)
    uint64_t wrap = 0;                                       // sequences wrapped at this width in the original (0: one line)
    char lead = '>';
};
Metadata read_metadata(Container& in, const std::string& file) {
    Metadata m;
    const std::vector<uint8_t> infov = in.getBytes(DS_INFOBYTE);
    m.p = plan::check_params(file, infov, in.getU64(DS_PARAMS));
    m.fasta_in = m.p.info & INFO_FASTA; m.has_header = !(m.p.info & INFO_NO_HEADER); m.has_qual = !(m.p.info & INFO_NO_QUAL);
    m.fastq_out = !m.fasta_in && m.has_qual;
    m.wrap = m.fasta_in ? m.p.fasta_line_width : 0;
    m.lead = m.fastq_out ? '@' : '>';
    m.tdna = in.getU64(DS_DNA_TABLE);
    plan::check_dna_table(file, m.tdna, m.p);
    if (m.has_header) {
        m.thdr = in.getU64(DS_HEADER_TABLE);
        m.first_header = in.getBytes(DS_FIRST_HEADER);
        plan::check_header_table(file, m.thdr, m.tdna, m.p);
    }
    if (m.has_qual) {
        m.tqual = in.getU64(DS_QUAL_TABLE);
        plan::check_qual_table(file, m.tqual, m.tdna, m.p);
    }
    m.has_sums = in.exists(DS_CHECKSUMS);
    if (m.has_sums) {
        m.tsum = in.getU64(DS_CHECKSUMS);
        plan::check_checksum_table(file, m.tsum, m.p.n_blocks);
    }
    m.has_letters = in.exists(DS_LETTER_RUNS);
    if (m.has_letters) {
        m.lt_runs = in.getU64(DS_LETTER_RUNS);
        plan::check_letter_runs(m.lt_runs, m.p.total_bases);
        const bool has_pos = in.exists(DS_LETTER_ODD_POS), has_bytes = in.exists(DS_LETTER_ODD_BYTES);
        if (has_pos != has_bytes) throw plan::letters_error(has_pos ? DS_LETTER_ODD_BYTES : DS_LETTER_ODD_POS, "is missing");
        if (has_pos) { m.lt_pos = in.getU64(DS_LETTER_ODD_POS); m.lt_bytes = in.getBytes(DS_LETTER_ODD_BYTES); }
        plan::check_letter_bytes(m.lt_pos, m.lt_bytes, m.p.total_bases);
    }
    return m;
}

// `-gz`: a round's text leaves as BGZF members of LEON_BGZF_MEMBER_TEXT bytes, compressed where the device has it
// (leon_text_bgzf_device); what does not fill a member waits in `carry` and goes in front of the next round's text, so the file is
// the same bytes however the text was cut into rounds and whoever formatted them.  All of it is stage C's (one round at a time).
// `-gz-records`: the members are cut at record starts (leon_text_bgzf_records_device with the records' offsets), and
// the carry -- whole records, at most one member's text -- is the next call's head.  `-gz-index`: every member's place in the file and
// in the text is kept for X.d.gz.gzi.  `-gz-matches`: the members' blocks come from k_deflate_lz_chunks
// (leon_text_bgzf_device_ex with LEON_BGZF_F_MATCHES); cuts, carry and index are the same.
// `-bam`: the same writer over unaligned BAM records (leon_records_bam_device / leon_host_records_bam) where `-gz` has
// the records' text; the BAM header is the carry the writer begins with, the head of its first call (one record start of its own).
struct BgzfWriter {
    static constexpr uint64_t HEAD = LEON_BGZF_MEMBER_TEXT;  // room in front of a round's text for the carry (at most one member's text)
    int fd = -1, device = 0;
    const std::string* out_name = nullptr;
    std::vector<uint8_t> carry;
    uint64_t file_at = 0, members = 0, text = 0;
    bool closed = false, records = false, index = false, matches = false;
    std::vector<uint64_t> gzi;                               // `-gz-index`: per data member, its offset in the file and in the text
    std::vector<uint64_t> m_out, m_text;
    // n_head + n_body bytes of device memory (the carry and a text behind it) through the call; returns the bytes it took.  The body's
    // records start at d_rec_off[0 .. n_records] (device memory; looked at under `-gz-records` only)
    uint64_t compress(const uint8_t* d_all, uint64_t n_head, uint64_t n_body, const uint64_t* d_rec_off, uint64_t n_records, bool last) {
        FileSink sink{fd, file_at};
        uint64_t taken = 0, out_bytes = 0, n_members = 0;
        const uint64_t n_all = n_head + n_body;
        if (!records && !index && !matches) {
            const int rc = leon_text_bgzf_device(device, d_all, n_all, last ? 1 : 0, FileSink::piece, &sink, &taken, &out_bytes, &n_members);
            if (rc == LEON_E_SINK) throw Exception("cannot write " + *out_name);
            check(nullptr, rc, "leon_text_bgzf_device");
        } else {
            if (!records) { n_head = 0; n_body = n_all; d_rec_off = nullptr; n_records = 0; }      // fixed cuts, with the members' places
            const uint64_t cap = !index ? 0 : records ? 3 * (n_all / HEAD) + 2 : n_all / HEAD + 1;
            if (m_out.size() < cap) { m_out.resize(cap); m_text.resize(cap); }
            uint64_t* const t_out = index ? m_out.data() : nullptr, * const t_text = index ? m_text.data() : nullptr;
            const int rc = matches ? leon_text_bgzf_device_ex(device, d_all, n_head, n_body, d_rec_off, n_records, last ? 1 : 0, FileSink::piece, &sink, &taken, &out_bytes,
                                                              t_out, t_text, cap, &n_members, LEON_BGZF_F_MATCHES)
                                   : leon_text_bgzf_records_device(device, d_all, n_head, n_body, d_rec_off, n_records, last ? 1 : 0, FileSink::piece, &sink, &taken,
                                                                   &out_bytes, t_out, t_text, cap, &n_members);
            if (rc == LEON_E_SINK) throw Exception("cannot write " + *out_name);
            check(nullptr, rc, matches ? "leon_text_bgzf_device_ex" : "leon_text_bgzf_records_device");
            if (index) for (uint64_t c = 0; c < n_members; c++) { gzi.push_back(file_at + m_out[c]); gzi.push_back(text + m_text[c]); }
        }
        file_at += out_bytes; members += n_members; text += taken;
        if (last) closed = true;
        return taken;
    }
    // `-gz-records`, a text the host formatted: pieces of whole records of at most one slice of the call, each with what the piece
    // before left as its head; leon_host_bgzf_record_cuts says where a piece's rest begins, and the device has to agree
    void records_from_host(uint8_t* p_text, uint64_t n_text, const std::vector<uint64_t>& rec_off, bool last, uint64_t piece) {
        const uint64_t n_rec = rec_off.size() - 1;
        uint64_t head = carry.size(), ra = 0;                 // the piece's text begins at p_text + rec_off[ra] - head
        std::vector<uint64_t> rel;
        do {
            uint64_t rb = (uint64_t)(std::upper_bound(rec_off.begin() + ra, rec_off.end(), rec_off[ra] + (piece > head ? piece - head : 0)) - rec_off.begin()) - 1;
            rb = std::min(std::max(rb, ra + 1), n_rec);       // at least one record
            const uint64_t n = rb - ra, body = rec_off[rb] - rec_off[ra], m = head + body;
            DeviceMem d, d_off;
            if (!d.try_alloc(device, m + 64) || !d_off.try_alloc(device, (n + 1) * 8)) {
                if (n <= 1) throw Exception("-gz-records: the device has no memory for the text of one record");
                piece = std::max<uint64_t>(piece / 2, 1);
                continue;
            }
            rel.resize(n + 1);
            for (uint64_t i = 0; i <= n; i++) rel[i] = rec_off[ra + i] - rec_off[ra];
            if (m) check(nullptr, leon_device_upload(device, d.get(), p_text + rec_off[ra] - head, m), "leon_device_upload");
            check(nullptr, leon_device_upload(device, d_off.get(), rel.data(), (n + 1) * 8), "leon_device_upload");
            const bool fin = last && rb == n_rec;
            uint64_t host_members = 0, host_taken = 0;
            check(nullptr, leon_host_bgzf_record_cuts(rel.data(), n, head, fin ? 1 : 0, nullptr, nullptr, 0, &host_members, &host_taken), "leon_host_bgzf_record_cuts");
            if (compress(d.as<uint8_t>(), head, body, d_off.as<uint64_t>(), n, fin) != host_taken)
                throw Exception("leon_text_bgzf_records_device: a piece was not cut where leon_host_bgzf_record_cuts cuts it");
            head = m - host_taken; ra = rb;
        } while (ra < n_rec);
        carry.assign(p_text + n_text - head, p_text + n_text);
    }
    // a text the host formatted, with HEAD bytes of room in front of it: up it goes behind the carry, in pieces of whole members of at
    // most one slice of the call; a piece the device has no memory for is halved
    void from_host(uint8_t* p_text, uint64_t n_text, const std::vector<uint64_t>& rec_off, bool last) {
        const uint64_t nc = carry.size();
        uint8_t* const all = p_text - nc;
        if (nc) memcpy(all, carry.data(), nc);
        const uint64_t n_all = nc + n_text, todo = last ? n_all : n_all - n_all % HEAD;
        uint64_t piece = 512ull << 20;
        if (const char* e = getenv("LEON_BGZF_SLICE")) { const long long v = atoll(e); if (v > 0) piece = (uint64_t)v; }
        if (records) return records_from_host(p_text, n_text, rec_off, last, piece);
        piece = std::max<uint64_t>(piece / HEAD, 1) * HEAD;
        for (uint64_t at = 0; at < todo;) {
            const uint64_t m = std::min(piece, todo - at);
            DeviceMem d;
            if (!d.try_alloc(device, m + 64)) {
                if (piece <= HEAD) throw Exception("-gz: the device has no memory for the text of one BGZF member");
                piece = std::max<uint64_t>(piece / 2 / HEAD, 1) * HEAD;
                continue;
            }
            check(nullptr, leon_device_upload(device, d.get(), all + at, m), "leon_device_upload");
            if (compress(d.as<uint8_t>(), 0, m, nullptr, 0, last && at + m == todo) != m) throw Exception("leon_text_bgzf_device: a piece of whole members was not taken whole");
            at += m;
        }
        carry.assign(all + todo, all + n_all);
    }
    // a text the device formatted, with HEAD bytes of room in front of it: it never crosses to the host uncompressed
    void from_device(uint8_t* d_text, uint64_t n_text, const uint64_t* d_rec_off, uint64_t n_records, bool last) {
        const uint64_t nc = carry.size(), n_all = nc + n_text;
        uint8_t* const d_all = d_text - nc;
        if (nc) check(nullptr, leon_device_upload(device, d_all, carry.data(), nc), "leon_device_upload");
        const uint64_t taken = compress(d_all, nc, n_text, d_rec_off, n_records, last);
        carry.resize(n_all - taken);
        if (!carry.empty()) check(nullptr, leon_device_download(device, carry.data(), d_all + taken, carry.size()), "leon_device_download");
    }
};

struct SymSet { leon_header_symbols* h = nullptr; ~SymSet() { leon_header_symbols_free(h); } };
struct TextSet { leon_header_text* h = nullptr; ~TextSet() { leon_header_text_free(h); } };   // (`-header-text device`: the text, in device memory)
// the output file: a failed run leaves no partial output behind
struct OutFile {
    int fd = -1; std::string path; bool keep = false;
    ~OutFile() { if (fd >= 0) ::close(fd); if (!keep && !path.empty()) std::remove(path.c_str()); }
};
// waits for a task on every way out of a scope, whatever it threw
struct WaitFor { std::future<void>& f; ~WaitFor() { if (f.valid()) { try { f.get(); } catch (...) {} } } };
void lap(std::chrono::steady_clock::time_point& t, double& acc) { const auto n = std::chrono::steady_clock::now(); acc += std::chrono::duration<double>(n - t).count(); t = n; }

struct Decoder {
    Leon& o;                                                 // the options
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    Container in;
    const std::string& file;                                 // the container's name, as the messages begin with it
    Metadata m;
    std::atomic<uint32_t> lt_ways{0};
    std::atomic<uint32_t> sum_ways[3] = {{0}, {0}, {0}};     // dna, header, quality: where the rounds' digests were taken
    std::atomic<uint64_t> sum_mismatches{0};
    int dev = 0;
    CtxPtr ctx, hdr_ctx;                                     // header blocks decode on the device too, on a stream of their own
    uint64_t header_blocks_on_device = 384;                  // rounds of at least this many blocks (LEON_HEADER_DEVICE_BLOCKS; tests: 0 = always, a huge number = never)
    std::vector<uint64_t> anchors;
    std::future<void> dict_job;
    std::string out_path;
    OutFile ofd, gzi_fd;                                     // (`-gz-index`: the index beside the file)
    bool rt_asked = false, rt_device = false, qi_device = false, hdr_text_device = false, hdr_on_device = false;
    std::string rt_reason;                                   // why the host formats although the device was asked for
    std::atomic<uint64_t> rt_rounds_on_device{0}, rt_rounds_no_memory{0}, qi_rounds_on_device{0}, qi_rounds_no_memory{0};
    std::atomic<uint64_t> hdr_blocks_fell_back{0};           // `-header-text device`: the blocks whose rounds went to the host decoder all the same
    uint64_t group = 1, dna_rounds = 1;
    uint32_t cores = 0, n_cpu = 1;
    BgzfWriter gz;
    std::unique_ptr<char[]> text;                            // the writing stage's records (never zero-filled)
    uint64_t text_cap = 0;
    double t_read = 0, t_dna = 0, t_hdr = 0, t_qual = 0, t_text = 0, t_write = 0, t_writer_wait = 0;
    RawBytes all_pay_h; std::vector<uint64_t> all_off_h; std::vector<uint32_t> all_reads_h;   // every header block's payload (the device's one call over them)
    std::vector<uint64_t> all_text_h;                        // every block's text size, from the block table (`-header-text device`)
    std::shared_ptr<SymSet> hdr_set = std::make_shared<SymSet>();
    std::shared_ptr<TextSet> hdr_text_set = std::make_shared<TextSet>();
    std::shared_future<void> hdr_symbols;
    std::shared_future<void> host_before, writer_before;     // stage B and stage C of the round before
    std::deque<std::shared_future<void>> pending;            // stage C of the rounds in flight, oldest first
    uint64_t read_index = 0, bases_out = 0;
    uint64_t next_file_off = 0;                              // owned by stage C (one round at a time)
    // Every task started below reads the members above.  A member that a running task reads must outlive that task, so this one, which
    // waits for all tasks, is the LAST member: it is destroyed first, whatever way run() is left.
    struct Drain {
        std::vector<std::shared_future<void>> all;
        ~Drain() { for (auto& f : all) if (f.valid()) f.wait(); }
    } drain;

    explicit Decoder(Leon& leon) : o(leon), in(leon._inputFilename, Container::READ), file(leon._inputFilename) {}
    void run();
    void open_device_and_dictionary();
    void open_output();
    void choose_ways();
    void choose_round_size();
    void gather(const char* grp, const std::vector<uint64_t>& tab, uint64_t g0, uint64_t nb, RawBytes& pay, std::vector<uint64_t>& off);
    void start_header_symbols();
    void stage_a(uint64_t a0);
    void stage_b(RoundPtr R);
    bool inflate_on_device(Round& R);
    void decode_quals(Round& R);
    int decode_header_text(Round& R, bool& host_decoder, uint64_t* need);
    void sum_header_text(Round& R, bool host_decoder);
    void stage_c(RoundPtr R);
    void restore_letters(Round& R);
    void verify_checksums(Round& R);
    uint64_t hdr_len(const Round& R, uint64_t r) const { return m.has_header ? R.hdr_off[r + 1] - R.hdr_off[r] : plan::index_text_len(R.read_index + r); }
    uint64_t record_len(const Round& R, uint64_t r, size_t* hint) const;
    uint64_t text_size(const Round& R) const;
    void check_qual_lengths(const Round& R) const;
    void write_round(Round& R);
    void format_records(const Round& R, const std::vector<uint64_t>& rec_off, const std::vector<uint64_t>& base_at, char* tbase, uint64_t ra, uint64_t rb) const;
    bool write_round_device(Round& R);
    uint64_t bam_bound(const Round& R) const;
    void bam_check(int rc, const char* what) const;
    void write_round_bam_host(Round& R);
    void download_text(const Round& R, const uint8_t* d_txt);
    void round_to_host(Round& R);
    void finish();
    void report();
};

void Decoder::run() {
    m = read_metadata(in, file);
    o._kmerSize = (size_t)m.p.k;
    open_device_and_dictionary();
    open_output();
    choose_ways();
    choose_round_size();
    start_header_symbols();
    for (uint64_t a0 = 0; a0 < m.p.n_blocks; a0 += group * dna_rounds) stage_a(a0);
    finish();
    report();
}

void Decoder::open_device_and_dictionary() {
    const plan::Params& p = m.p;
    dev = device_for(0);
    ctx = make_ctx((uint32_t)p.k, p.tai, dev, (uint32_t)p.n_hash, (uint32_t)p.nbits, (uint32_t)p.rpb);
    if (m.has_header) hdr_ctx = make_ctx((uint32_t)p.k, 1000, device_for(0));
    if (const char* e = getenv("LEON_HEADER_DEVICE_BLOCKS")) header_blocks_on_device = (uint64_t)std::max<long long>(0, atoll(e));
    {
        const std::vector<uint8_t> bloom = in.getBytes(DS_BLOOM_BITS);
        check(ctx.get(), leon_dna_bloom_upload(ctx.get(), bloom.data(), bloom.size()), "leon_dna_bloom_upload");
    }
    // the dictionary stream is one serial chain on a host core (3.7 s at 100 M reads): it runs beside the container reads and
    // the first round's header / quality blocks, and is waited for right before the first DNA blocks go to the device
    const uint32_t W = p.k >= 32 ? 2 : 1;
    anchors.resize(std::max<uint64_t>(p.n_anchors * W, 1));
    {
        // `-c -dict-pieces` wrote the dictionary as independently coded pieces: decoded on the device, at once (k_dict_decode_pieces)
        const bool has_pieces = in.exists(DS_ANCHOR_DICT_PIECES), has_table = in.exists(DS_ANCHOR_DICT_PIECE_TABLE);
        const std::vector<uint64_t> table = has_table ? in.getU64(DS_ANCHOR_DICT_PIECE_TABLE) : std::vector<uint64_t>();
        const std::vector<uint8_t> pieces = has_pieces ? in.getBytes(DS_ANCHOR_DICT_PIECES) : std::vector<uint8_t>();
        if (plan::check_dict_pieces(file, in.exists(DS_ANCHOR_DICT), has_pieces, has_table, table, pieces.size(), p.n_anchors)) {
            const uint64_t n_pieces = table.size() - 2;
            const std::vector<uint64_t> piece_off = plan::prefix_sums(table.data() + 2, n_pieces);
            const auto t0 = std::chrono::steady_clock::now();
            if (leon_anchor_dict_decode_pieces_device(dev, pieces.data(), piece_off.data(), n_pieces, p.n_anchors, (uint32_t)p.k, (uint32_t)table[1], anchors.data()) != LEON_OK)
                throw Exception(file + ": dictionary pieces: " + leon_last_error(nullptr));
            if (o._verbose) std::cout << "dictionary: " << n_pieces << " pieces of " << table[1] << " anchors decoded on the device (k_dict_decode_pieces) in " << seconds_since(t0) << " s\n";
            return;                                              // (no dict_job: nothing to wait for)
        }
    }
    if (o._verbose) std::cout << "dictionary: one stream, decoded on a host thread (leon_host_anchor_dict_decode)\n";
    auto dict = std::make_shared<std::vector<uint8_t>>(in.getBytes(DS_ANCHOR_DICT));
    const uint64_t dsz = dict->size(), n_anchors = p.n_anchors;
    dict->push_back(0);
    uint64_t* out_kmers = anchors.data();
    const uint32_t kk = (uint32_t)p.k;
    dict_job = std::async(std::launch::async, [dict, dsz, n_anchors, kk, out_kmers] {
        check(nullptr, leon_host_anchor_dict_decode(dict->data(), dsz, n_anchors, kk, out_kmers), "leon_host_anchor_dict_decode");
    });
}

void Decoder::open_output() {
    // X.fastq.leon -> X.fastq.d (/root/reference/scripts/simple_test.sh:54,62)
    std::string stem = file;
    if (ends_with(stem, ".leon")) stem.resize(stem.size() - 5);
    // `-gz`: X.fastq.d.gz, BGZF written under a temporary name and renamed at the very end
    o._outputFilename = stem + (o._bam ? ".d.bam" : o._gz ? ".d.gz" : ".d");
    out_path = o._gz ? o._outputFilename + ".tmp" : o._outputFilename;
    ofd.fd = ::open(out_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (ofd.fd < 0) throw Exception("cannot write " + o._outputFilename);
    ofd.path = out_path;
    gz.fd = ofd.fd; gz.device = dev; gz.out_name = &o._outputFilename;
    gz.records = o._gzRecords; gz.index = o._gzIndex; gz.matches = o._gzMatches;
    if (o._bam) {                                            // the BAM header: what the first call finds in front of its records
        uint64_t n = 0;
        gz.carry.resize(64);
        check(nullptr, leon_bam_header(gz.carry.data(), gz.carry.size(), &n), "leon_bam_header");
        gz.carry.resize(n);
    }
    if (o._gzIndex) {                                        // X.fastq.d.gz.gzi, under a temporary name like the file it belongs to
        gzi_fd.fd = ::open((o._outputFilename + ".gzi.tmp").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (gzi_fd.fd < 0) throw Exception("cannot write " + o._outputFilename + ".gzi");
        gzi_fd.path = o._outputFilename + ".gzi.tmp";
    }
    // (read here, not with the rest of the metadata: a table that is refused takes the output file with it, as a failed run does)
    if (m.fastq_out && m.has_header && in.exists(DS_PLUS_LINES)) {
        const std::vector<uint8_t> blob = in.getBytes(DS_PLUS_LINES);
        m.plus = PlusLines::decode(blob.data(), blob.size());
        if (!m.plus.exc.empty() && m.plus.exc.back().read >= m.p.n_reads) throw Exception(file + ": malformed '+'-line table");
    }
}

void Decoder::choose_ways() {
    const uint64_t n_blocks = m.p.n_blocks;
    // `-record-text`: the records formatted on the device, where every '+' line is of one kind
    rt_asked = n_blocks > 0 && device_chosen(parse_choice("-record-text", o._recordText), n_blocks, kRecordTextAutoBlocks);
    if (rt_asked && !o._bam && (!m.plus.exc.empty() || m.plus.def > 1)) rt_reason = "the '+' lines are mixed: exception records in the pluslines table";
    rt_device = rt_asked && rt_reason.empty();
    // `-qual-inflate`: the quality blocks inflated on the device
    qi_device = m.fastq_out && n_blocks > 0 && device_chosen(parse_choice("-qual-inflate", o._qualInflate), n_blocks, kQualInflateAutoBlocks);
    cores = (uint32_t)o._nbCores;
    n_cpu = (uint32_t)(o._nbCores > 0 ? (uint64_t)o._nbCores : usableCpus());
}

// Blocks decoded per round.  A round costs the device ONE block's serial chain whatever the number of blocks in it (up to
// a few thousand: one wave per block), so rounds should be large; up to five are alive at a time (see the stages), each
// ~5 bytes per base in bases, qualities and text: a twentieth of the available RAM each.  Files of more than a few hundred blocks are cut into at least four rounds, so that the host's share of the
// work (header and quality blocks, formatting, writing) of one round runs beside the decoding of the next.
void Decoder::choose_round_size() {
    const uint64_t n_blocks = m.p.n_blocks;
    group = n_blocks ? n_blocks : 1;
    const long pages = sysconf(_SC_AVPHYS_PAGES), page = sysconf(_SC_PAGESIZE);
    const uint64_t avail = pages > 0 && page > 0 ? (uint64_t)pages * (uint64_t)page : (8ull << 30);
    const uint64_t bases_per_block = n_blocks ? std::max<uint64_t>(m.p.total_bases / n_blocks, 1) : 1;
    const uint64_t fit = avail / 20 / 5 / bases_per_block;
    group = std::min<uint64_t>(group, std::max<uint64_t>(fit, 64));
    if (n_blocks >= 800) group = std::min<uint64_t>(group, (n_blocks + 3) / 4);
    if (const char* e = getenv("LEON_DECODE_BLOCKS")) { const long v = atol(e); if (v > 0) group = (uint64_t)v; }   // (tests: several rounds on a small file)
    dna_rounds = n_blocks >= 800 ? 2 : 1;
    if (const char* e = getenv("LEON_DECODE_DNA_ROUNDS")) { const long v = atol(e); if (v > 0) dna_rounds = (uint64_t)v; }   // (tests)
}

// the payloads of blocks [g0, g0 + nb) of one stream, one behind the other, checked against the sizes in their table
void Decoder::gather(const char* grp, const std::vector<uint64_t>& tab, uint64_t g0, uint64_t nb, RawBytes& pay, std::vector<uint64_t>& off) {
    off = plan::prefix_sums(tab.data() + 3 * g0, nb, 3);
    pay.resize(off[nb] + 1);
    for (uint64_t b = 0; b < nb; b++) {
        const std::vector<uint8_t> blk = in.getBytes(Container::blockPath(grp, g0 + b));
        if (blk.size() != tab[3 * (g0 + b)]) throw Exception(file + ": block " + std::to_string(g0 + b) + " of " + grp + " has not the size its table says");
        if (!blk.empty()) memcpy(pay.data() + off[b], blk.data(), blk.size());
    }
}

// Header blocks whose symbols the device decodes: ALL of the file's blocks in ONE device call, started here, beside everything else.
// A header block is one serial chain on one wave (~1.5 s for 50 000 headers) whether the call holds 200 blocks or 2 000, so a call
// per round paid that chain every round (4 x 2.7 s of configuration #3's 20 s); the rounds now only rebuild their blocks' text
// from the symbols, on the host threads.
// `-header-text device`: the text as well, in the same call; it stays on the device and the rounds fetch their blocks' share
void Decoder::start_header_symbols() {
    const uint64_t n_blocks = m.p.n_blocks;
    hdr_text_device = m.has_header && n_blocks > 0 && device_chosen(parse_choice("-header-text", o._headerText), n_blocks, kHeaderTextAutoBlocks);
    hdr_on_device = m.has_header && n_blocks > 0 && (hdr_text_device || group >= header_blocks_on_device);
    if (!hdr_on_device) return;
    all_reads_h.resize(n_blocks);
    for (uint64_t b = 0; b < n_blocks; b++) all_reads_h[b] = (uint32_t)m.tdna[3 * b + 1];
    gather(GROUP_HEADER, m.thdr, 0, n_blocks, all_pay_h, all_off_h);
    leon_dna_ctx* hc = hdr_ctx.get();
    const uint8_t* pay = all_pay_h.data(); const uint64_t* off = all_off_h.data(); const uint32_t* nr = all_reads_h.data();
    if (hdr_text_device) { all_text_h.resize(n_blocks); for (uint64_t b = 0; b < n_blocks; b++) all_text_h[b] = m.thdr[3 * b + 2]; }
    const uint64_t* tb = all_text_h.data();
    const uint8_t* fh = m.first_header.data(); const uint64_t fh_len = m.first_header.size();
    const bool with_text = hdr_text_device;
    auto symbols = hdr_set; auto texts = hdr_text_set;
    hdr_symbols = std::async(std::launch::async, [hc, pay, off, nr, n_blocks, symbols, texts, with_text, tb, fh, fh_len] {
        const int rc = with_text ? leon_header_decode_text(hc, pay, off, nr, tb, n_blocks, fh, fh_len, &texts->h)
                                 : leon_header_decode_symbols(hc, pay, off, nr, n_blocks, &symbols->h);
        check(hc, rc, "header blocks");
    }).share();
    drain.all.push_back(hdr_symbols);
}

// ------------------------------------------------------------------------------------------------ stage A
// one device call's blocks [a0, a1): its rounds are cut, their stage B started, the DNA blocks decoded, their stage C started
void Decoder::stage_a(uint64_t a0) {
    const uint64_t n_blocks = m.p.n_blocks, a1 = std::min(n_blocks, a0 + group * dna_rounds), na = a1 - a0;
    auto tl = std::chrono::steady_clock::now();
    while (pending.size() > dna_rounds) { pending.front().get(); pending.pop_front(); }   // (their errors, and those of their stage B, surface here)
    lap(tl, t_writer_wait);
    // the host part: the DNA payloads of the call, and every round's header and quality payloads
    auto G = std::make_shared<DnaGroup>();
    RawBytes pay; std::vector<uint64_t> off;
    std::vector<uint32_t> a_reads(na); std::vector<uint64_t> a_bases(na);
    uint64_t ga_reads = 0, ga_bases = 0;
    for (uint64_t b = 0; b < na; b++) { a_reads[b] = (uint32_t)m.tdna[3 * (a0 + b) + 1]; a_bases[b] = m.tdna[3 * (a0 + b) + 2]; ga_reads += a_reads[b]; ga_bases += a_bases[b]; }
    gather(GROUP_DNA, m.tdna, a0, na, pay, off);
    bool g_device = rt_device;
    if (g_device && (!G->d_bases.try_alloc(dev, ga_bases + 64) || !G->d_lens.try_alloc(dev, (ga_reads + 1) * 4))) {
        G->release_device();                                 // no room: this call's rounds are formatted on the host
        g_device = false;
        rt_rounds_no_memory += (na + group - 1) / group;
    }
    if (!g_device) G->bases.resize(ga_bases + 1);
    G->lens.reset(new uint32_t[ga_reads + 1]);
    std::vector<std::pair<RoundPtr, std::shared_future<void>>> rounds;
    uint64_t base0 = 0, read0 = 0;
    for (uint64_t g0 = a0; g0 < a1; g0 += group) {
        const uint64_t g1 = std::min(a1, g0 + group), nb = g1 - g0;
        auto R = std::make_shared<Round>();
        R->nb = nb; R->blk_reads.assign(a_reads.begin() + (g0 - a0), a_reads.begin() + (g1 - a0)); R->blk_bases.assign(a_bases.begin() + (g0 - a0), a_bases.begin() + (g1 - a0));
        uint64_t g_reads = 0, g_bases = 0;
        for (uint64_t b = 0; b < nb; b++) { g_reads += R->blk_reads[b]; g_bases += R->blk_bases[b]; }
        R->read_index = read_index; R->g_reads = g_reads; R->g_bases = g_bases;
        R->dna = G; R->base0 = base0; R->read0 = read0; R->file_base0 = bases_out;
        R->on_device = g_device;
        R->last = g1 == n_blocks;
        if (g_device) G->rounds_left++;
        if (m.has_header && !hdr_on_device) gather(GROUP_HEADER, m.thdr, g0, nb, R->pay_h, R->off_h);
        R->block0 = g0;
        if (m.fastq_out) gather(GROUP_QUAL, m.tqual, g0, nb, R->pay_q, R->off_q);
        R->hdr_off.assign(g_reads + 1, 0); R->qual_off.assign(g_reads + 1, 0);
        R->hdr_text_bytes = 64;
        if (m.has_header) for (uint64_t b = 0; b < nb; b++) R->hdr_text_bytes += m.thdr[3 * (g0 + b) + 2];
        std::shared_future<void> before = host_before;
        std::shared_future<void> host_job = std::async(std::launch::async, [this, R, before] {
            if (before.valid()) before.wait();
            stage_b(R);
        }).share();
        drain.all.push_back(host_job);
        host_before = host_job;
        rounds.emplace_back(R, host_job);
        base0 += g_bases; read0 += g_reads; read_index += g_reads; bases_out += g_bases;
    }
    lap(tl, t_read);
    // the device part
    if (dict_job.valid()) dict_job.get();
    if (g_device)
        check(ctx.get(), leon_dna_decode_blocks_device(ctx.get(), anchors.data(), m.p.n_anchors, pay.data(), off.data(), a_reads.data(), a_bases.data(), na,
                                                       G->d_bases.as<uint8_t>(), ga_bases, G->d_lens.as<uint32_t>(), G->lens.get()), "leon_dna_decode_blocks_device");
    else
        check(ctx.get(), leon_dna_decode_blocks(ctx.get(), anchors.data(), m.p.n_anchors, pay.data(), off.data(), a_reads.data(), a_bases.data(), na, G->bases.data(), ga_bases,
                                                G->lens.get()), "leon_dna_decode_blocks");
    lap(tl, t_dna);
    for (auto& rh : rounds) {
        RoundPtr R = rh.first;
        std::shared_future<void> host_job = rh.second, before = writer_before;
        std::shared_future<void> writer = std::async(std::launch::async, [this, R, host_job, before] {
            host_job.get();                                  // (a failed stage B fails this round's stage C with its message)
            if (before.valid()) before.get();                // file order; a failure before this round stops the rounds after it
            stage_c(R);
        }).share();
        drain.all.push_back(writer);
        pending.push_back(writer);
        writer_before = writer;
    }
}

// ------------------------------------------------------------------------------------------------ stage B
// `-qual-inflate device`: false when the device has no memory for the round (nothing done: the host threads inflate it)
bool Decoder::inflate_on_device(Round& R) {
    const uint64_t nb = R.nb, g_bases = R.g_bases;
    DeviceMem d_q, d_off;
    if (!d_q.try_alloc(dev, g_bases + 64) || !d_off.try_alloc(dev, (R.g_reads + 1) * 8)) return false;
    const int rc = leon_qual_inflate_blocks_device(dev, R.pay_q.data(), R.off_q.data(), R.blk_reads.data(), R.blk_bases.data(), nb, nullptr,
                                                   d_q.as<uint8_t>(), g_bases, d_off.as<uint64_t>(), nullptr);
    if (rc == LEON_E_HIP && std::string(leon_last_error(nullptr)).find("out of memory") != std::string::npos) return false;   // (its temporaries)
    check(nullptr, rc, "leon_qual_inflate_blocks_device");
    // the reads' offsets come to the host: the check that a read's quality and sequence lengths agree is the writing stage's
    check(nullptr, leon_device_download(dev, R.qual_off.data(), d_off.get(), (R.g_reads + 1) * 8), "leon_device_download");
    if (m.has_sums) {                                        // digested where they were inflated
        R.sum_qual.assign(nb, 0);
        sums_on_device(dev, d_q.get(), g_bases, plan::prefix_sums(R.blk_bases.data(), nb).data(), nb, R.sum_qual.data());
        sum_ways[2] |= ON_DEVICE;
    }
    if (R.on_device) R.d_qual = std::move(d_q);
    else {
        R.qual.resize(g_bases + 1);
        check(nullptr, leon_device_download(dev, R.qual.data(), d_q.get(), g_bases), "leon_device_download");
    }
    qi_rounds_on_device++;
    return true;
}

void Decoder::decode_quals(Round& R) {
    const uint64_t nb = R.nb, g_bases = R.g_bases;
    if (qi_device) {
        if (inflate_on_device(R)) return;
        qi_rounds_no_memory++;
    }
    R.qual.resize(g_bases + 1);
    check(nullptr, leon_host_qual_decode_blocks(R.pay_q.data(), R.off_q.data(), R.blk_reads.data(), R.blk_bases.data(), nb, R.qual.data(), g_bases, R.qual_off.data(), cores),
          "leon_host_qual_decode_blocks");
    if (m.has_sums) {
        R.sum_qual.assign(nb, 0);
        sums_on_host(R.qual.data(), g_bases, plan::prefix_sums(R.blk_bases.data(), nb).data(), nb, cores, R.sum_qual.data());
        sum_ways[2] |= ON_HOST;
    }
}

// The round's header text into R.hdr, by the first way that takes it: fetched from the device's text set, rebuilt from the device's
// symbols, or decoded from the payloads by the host decoder (`host_decoder`: the ways before it are not to be tried, or declined).
int Decoder::decode_header_text(Round& R, bool& host_decoder, uint64_t* need) {
    const uint64_t nb = R.nb;
    const uint8_t* fh = m.first_header.data(); const uint64_t fh_len = m.first_header.size();
    if (hdr_text_device && !host_decoder) {
        const int rc = leon_header_text_fetch(hdr_text_set->h, R.block0, nb, R.hdr.data(), R.hdr.size(), R.hdr_off.data(), need);
        if (rc != LEON_E_STATE) return rc;
        host_decoder = true;                                 // the kernel declined a block of the round: the host decoder, from the payloads
        hdr_blocks_fell_back += nb;
    }
    if (hdr_on_device && !host_decoder) {
        const int rc = leon_header_text_from_symbols(hdr_set->h, R.block0, nb, R.blk_reads.data(), fh, fh_len, R.hdr.data(), R.hdr.size(), R.hdr_off.data(), need, cores);
        if (rc != LEON_E_STATE) return rc;
        host_decoder = true;
    }
    if (hdr_on_device)
        return leon_host_header_decode_blocks(all_pay_h.data(), all_off_h.data() + R.block0, R.blk_reads.data(), nb, fh, fh_len, R.hdr.data(), R.hdr.size(), R.hdr_off.data(), need, cores);
    return leon_host_header_decode_blocks(R.pay_h.data(), R.off_h.data(), R.blk_reads.data(), nb, fh, fh_len, R.hdr.data(), R.hdr.size(), R.hdr_off.data(), need, cores);
}

// `-checksum`: the header text digested where it lies: in the device's set under `-header-text device` (its blocks' shares follow one
// another, sized by the block table), else the round's host buffer, its blocks cut at the reads' offsets
void Decoder::sum_header_text(Round& R, bool host_decoder) {
    const uint64_t nb = R.nb;
    R.sum_hdr.assign(nb, 0);
    const uint8_t* dh = R.d_hdr; const uint64_t* dho = nullptr; uint64_t dsz = R.d_hdr_size;
    bool in_set = R.hdr_in_set;
    if (!in_set && hdr_text_device && !host_decoder) in_set = leon_header_text_device_ptr(hdr_text_set->h, R.block0, nb, &dh, &dho, &dsz) == LEON_OK;
    std::vector<uint64_t> boff(nb + 1, 0);
    if (in_set) {
        boff = plan::prefix_sums(m.thdr.data() + 3 * R.block0 + 2, nb, 3);
        if (boff[nb] != dsz) in_set = false;
    }
    if (in_set) { sums_on_device(dev, dh, dsz, boff.data(), nb, R.sum_hdr.data()); sum_ways[1] |= ON_DEVICE; return; }
    if (R.hdr_in_set) throw Exception(file + ": the header block table does not add up");
    uint64_t r = 0;
    for (uint64_t b = 0; b < nb; b++) { boff[b] = R.hdr_off[r]; r += R.blk_reads[b]; }
    boff[nb] = R.hdr_off[r];
    sums_on_host(R.hdr.data(), boff[nb], boff.data(), nb, cores, R.sum_hdr.data());
    sum_ways[1] |= ON_HOST;
}

// a round's header blocks and, beside or behind them, its quality blocks
void Decoder::stage_b(RoundPtr Rp) {
    Round& R = *Rp;
    auto th = std::chrono::steady_clock::now();
    const uint64_t nb = R.nb;
    // while the first round waits for the device's header symbols the host threads have nothing to do: the quality blocks go then
    std::future<void> quals_beside;
    WaitFor wait_for_quals{quals_beside};
    if (m.fastq_out && hdr_on_device && hdr_symbols.valid() && hdr_symbols.wait_for(std::chrono::seconds(0)) != std::future_status::ready)
        quals_beside = std::async(std::launch::async, [this, Rp] { decode_quals(*Rp); });
    if (m.has_header) {
        uint64_t need = 0;
        R.hdr.resize(R.hdr_text_bytes);                       // from the block table (a wrong entry only costs the second call below)
        // The symbols of every header block come from ONE device call over the whole file (start_header_symbols); a round rebuilds its
        // blocks' text from them.  Files of a few hundred blocks: the host threads alone are quicker (10 M headers in 200
        // blocks: 0.62 s against 1.27 s).  A set whose symbols did not fit the device buffer (free text in every header)
        // sends the rounds to the host decoder, from the same payloads.
        bool host_decoder = !hdr_on_device;
        if (hdr_on_device) hdr_symbols.get();
        // `-record-text device` beside `-header-text device`: the round's text is used where it lies, nothing is fetched
        if (R.on_device && hdr_text_device) {
            const int rc0 = leon_header_text_device_ptr(hdr_text_set->h, R.block0, nb, &R.d_hdr, &R.d_hdr_off, &R.d_hdr_size);
            if (rc0 == LEON_OK) R.hdr_in_set = true;
            else if (rc0 == LEON_E_STATE) { host_decoder = true; hdr_blocks_fell_back += nb; }   // the kernel declined a block of the round
            else check(nullptr, rc0, "header blocks");
        }
        int rc = R.hdr_in_set ? LEON_OK : decode_header_text(R, host_decoder, &need);
        if (rc == LEON_E_OVERFLOW) { R.hdr.resize(need + 1); rc = decode_header_text(R, host_decoder, &need); }
        check(nullptr, rc, "header blocks");
        if (m.has_sums) sum_header_text(R, host_decoder);
    }
    lap(th, t_hdr);
    if (quals_beside.valid()) quals_beside.get();
    else if (m.fastq_out) decode_quals(R);
    lap(th, t_qual);
    R.pay_h = RawBytes(); R.pay_q = RawBytes();               // (the payloads are not needed any more)
}

// ------------------------------------------------------------------------------------------------ stage C
// the round's share of the letter tables put back where its bases lie
void Decoder::restore_letters(Round& R) {
    const plan::LetterSlice s = plan::clip_letters(m.lt_runs, m.lt_pos, R.file_base0, R.file_base0 + R.g_bases);
    const uint8_t* bytes = m.lt_bytes.data() + s.first_pos;
    if (R.on_device) {
        check(nullptr, leon_letters_apply_device(dev, R.d_bases(), R.g_bases, s.runs.data(), s.runs.size() / 2, s.pos.data(), bytes, s.pos.size()), "leon_letters_apply_device");
        lt_ways |= ON_DEVICE;
    } else {
        check(nullptr, leon_host_letters_apply(const_cast<uint8_t*>(R.bases()), R.g_bases, s.runs.data(), s.runs.size() / 2, s.pos.data(), bytes, s.pos.size(), cores),
              "leon_host_letters_apply");
        lt_ways |= ON_HOST;
    }
}

// the restored bases digested where the decoder left them (the headers' and qualities' digests are stage B's), then all three compared
// with the container's
void Decoder::verify_checksums(Round& R) {
    const uint64_t nb = R.nb;
    const std::vector<uint64_t> boff = plan::prefix_sums(R.blk_bases.data(), nb);
    std::vector<uint32_t> sum_dna(nb, 0);
    if (R.on_device) { sums_on_device(dev, R.d_bases(), R.g_bases, boff.data(), nb, sum_dna.data()); sum_ways[0] |= ON_DEVICE; }
    else { sums_on_host(R.bases(), R.g_bases, boff.data(), nb, cores, sum_dna.data()); sum_ways[0] |= ON_HOST; }
    // the smallest failing block first (the rounds come in file order), its streams in the order dna, header, quality
    const char* const names[3] = {"dna", "header", "quality"};
    const std::vector<uint32_t>* got[3] = {&sum_dna, m.has_header ? &R.sum_hdr : nullptr, m.has_qual && m.fastq_out ? &R.sum_qual : nullptr};
    for (uint64_t b = 0; b < nb; b++)
        for (int st = 0; st < 3; st++) {
            if (!got[st]) continue;
            if (got[st]->size() != nb) throw Exception(std::string("checksum: the ") + names[st] + " digests of block " + std::to_string(R.block0 + b) + " were not taken");
            const uint64_t stored = m.tsum[1 + 3 * (R.block0 + b) + st];
            if (stored == (*got[st])[b]) continue;
            char hex[64];
            snprintf(hex, sizeof hex, "(stored 0x%08llx, restored 0x%08x)", (unsigned long long)stored, (unsigned)(*got[st])[b]);
            const std::string msg = std::string("checksum: ") + names[st] + " block " + std::to_string(R.block0 + b) + " does not match what was compressed " + hex;
            if (!o._ignoreChecksum) throw Exception(msg);
            std::cerr << "WARNING: " << msg << std::endl;
            sum_mismatches++;
        }
}

// read r of the round as text; *hint walks the '+' lines' exceptions forwards
uint64_t Decoder::record_len(const Round& R, uint64_t r, size_t* hint) const {
    const uint64_t hl = hdr_len(R, r);
    uint64_t extra = 0;
    if (!m.plus.trivial()) {
        const PlusLines::Exc* e = m.plus.exc.empty() ? nullptr : m.plus.find(R.read_index + r, hint);
        extra = plan::plus_extra_len(e ? e->kind : m.plus.def, hl, e ? e->text.size() : 0);
    }
    return plan::record_text_len(hl, R.lens()[r], m.wrap, m.fastq_out, extra);
}

// the size of the round's text: where the next round's begins.  Two closed forms spare the common cases a loop over the reads.
uint64_t Decoder::text_size(const Round& R) const {
    const uint64_t g_reads = R.g_reads, g_bases = R.g_bases, wrap = m.wrap;
    if (R.on_device) {                                       // ('+' lines of one kind; the header text may lie on the device: its size is known all the same)
        uint64_t hdr_total = 0, seq_text = wrap ? 0 : g_bases + g_reads;
        if (m.has_header) hdr_total = R.hdr_in_set ? R.d_hdr_size : R.hdr_off[g_reads] - R.hdr_off[0];
        else for (uint64_t r = 0; r < g_reads; r++) hdr_total += hdr_len(R, r);
        if (wrap) for (uint64_t r = 0; r < g_reads; r++) seq_text += plan::seq_text_len(R.lens()[r], wrap);
        return plan::records_text_len(g_reads, hdr_total, seq_text, g_bases, m.fastq_out, m.plus.def);
    }
    if (m.has_header && !wrap && m.plus.exc.empty())         // (the decoder has checked that the lengths add up to the block table's bases)
        return plan::records_text_len(g_reads, R.hdr_off[g_reads], g_bases + g_reads, g_bases, m.fastq_out, m.plus.def);
    uint64_t n_text = 0;
    size_t hint = m.plus.lower(R.read_index);
    for (uint64_t r = 0; r < g_reads; r++) n_text += record_len(R, r, &hint);
    return n_text;
}

void Decoder::check_qual_lengths(const Round& R) const {
    if (!m.fastq_out) return;
    for (uint64_t r = 0; r < R.g_reads; r++)
        if (R.qual_off[r + 1] - R.qual_off[r] != R.lens()[r]) throw Exception(file + ": a read's quality and sequence lengths differ");
}

void Decoder::stage_c(RoundPtr Rp) {
    Round& R = *Rp;
    // (`-record-text device`: the call's device buffers go when its last round is written, or has failed)
    struct Left { DnaGroup* g; ~Left() { if (g && --g->rounds_left == 0) g->release_device(); } } left{R.on_device ? R.dna.get() : nullptr};
    if (m.has_letters) restore_letters(R);
    if (m.has_sums) verify_checksums(R);
    if (!o._bam) {                                           // (BAM records are sized by their formatter, and BGZF has no file offsets to plan)
        R.n_text = text_size(R); R.file_off = next_file_off;
        next_file_off += R.n_text;
    }
    if (R.on_device && write_round_device(R)) return;
    if (R.on_device) round_to_host(R);
    if (o._bam) write_round_bam_host(R); else write_round(R);
}

// reads [ra, rb) of the round as records at tbase + rec_off[r]
void Decoder::format_records(const Round& R, const std::vector<uint64_t>& rec_off, const std::vector<uint64_t>& base_at, char* tbase, uint64_t ra, uint64_t rb) const {
    const uint64_t wrap = m.wrap;
    size_t hint = m.plus.lower(R.read_index + ra);
    for (uint64_t r = ra; r < rb; r++) {
        char* w = tbase + rec_off[r];
        *w++ = m.lead;
        if (m.has_header) { const uint64_t hl = R.hdr_off[r + 1] - R.hdr_off[r]; memcpy(w, R.hdr.data() + R.hdr_off[r], hl); w += hl; }
        else { const std::string idx = std::to_string(R.read_index + r); memcpy(w, idx.data(), idx.size()); w += idx.size(); }
        *w++ = '\n';
        const char* seq = reinterpret_cast<const char*>(R.bases()) + base_at[r];
        const uint64_t len = R.lens()[r];
        if (wrap && len > wrap) {
            for (uint64_t o2 = 0; o2 < len; o2 += wrap) { const uint64_t n = std::min<uint64_t>(wrap, len - o2); memcpy(w, seq + o2, n); w += n; *w++ = '\n'; }
        } else { memcpy(w, seq, len); w += len; *w++ = '\n'; }
        if (m.fastq_out) {
            *w++ = '+';
            if (!m.plus.trivial()) {
                const PlusLines::Exc* e = m.plus.exc.empty() ? nullptr : m.plus.find(R.read_index + r, &hint);
                const uint8_t kind = e ? e->kind : m.plus.def;
                if (kind == 1) { const uint64_t hl = R.hdr_off[r + 1] - R.hdr_off[r]; memcpy(w, R.hdr.data() + R.hdr_off[r], hl); w += hl; }
                else if (kind == 2) { memcpy(w, e->text.data(), e->text.size()); w += e->text.size(); }
            }
            *w++ = '\n'; memcpy(w, R.qual.data() + R.qual_off[r], len); w += len; *w++ = '\n';
        }
    }
}

// the writing stage on the host: every read's place in the text is known from the lengths, so a round is formatted by all cores at
// once and written by several (each its own share of the file)
void Decoder::write_round(Round& R) {
    auto tl = std::chrono::steady_clock::now();
    const uint64_t g_reads = R.g_reads;
    std::vector<uint64_t> rec_off(g_reads + 1, 0), base_at(g_reads + 1, 0);
    check_qual_lengths(R);
    size_t hint0 = m.plus.lower(R.read_index);
    for (uint64_t r = 0; r < g_reads; r++) {
        rec_off[r + 1] = rec_off[r] + record_len(R, r, &hint0);
        base_at[r + 1] = base_at[r] + R.lens()[r];
    }
    const uint64_t n_text = rec_off[g_reads];
    if (n_text != R.n_text) throw Exception(file + ": the decoded reads do not add up to their blocks' sizes");
    const uint64_t head = o._gz ? BgzfWriter::HEAD : 0;
    if (head + n_text > text_cap) { text.reset(); text_cap = head + n_text + n_text / 16; text.reset(new char[text_cap]); }
    char* const tbase = text.get() + head;
    const uint32_t n_fmt = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_cpu, g_reads / 4096 + 1));
    std::atomic<bool> write_failed{false};
    auto format_range = [&](uint64_t ra, uint64_t rb) {
        format_records(R, rec_off, base_at, tbase, ra, rb);
        if (o._gz) return;                                    // (compressed below, once the whole round is there)
        // this thread's share of the text goes out as soon as it is formatted
        if (!write_all(ofd.fd, tbase + rec_off[ra], rec_off[rb] - rec_off[ra], R.file_off + rec_off[ra])) write_failed = true;
    };
    if (n_fmt <= 1) format_range(0, g_reads);
    else {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < n_fmt; t++) th.emplace_back(format_range, g_reads * t / n_fmt, g_reads * (t + 1) / n_fmt);
        for (auto& t : th) t.join();
    }
    if (write_failed) throw Exception("cannot write " + o._outputFilename);
    if (o._gz) gz.from_host(reinterpret_cast<uint8_t*>(tbase), n_text, rec_off, R.last);
    lap(tl, t_text);
}

// The writing stage of `-record-text device`: the round's records formatted by the device from the bases (and, under `-header-text
// device`, the header text) that are there already; the finished text comes back in pinned pieces, each written where it landed.
// false: no device memory for the round's buffers (nothing written): the caller formats it on the host.
bool Decoder::write_round_device(Round& R) {
    auto tl = std::chrono::steady_clock::now();
    const uint64_t g_reads = R.g_reads, g_bases = R.g_bases, n_text = o._bam ? bam_bound(R) : R.n_text;   // (`-bam`: room enough; the call says what it took)
    check_qual_lengths(R);
    DeviceMem d_text, d_qual, d_hdr, d_hoff, d_rec;
    auto upload = [&](void* d, const void* src, uint64_t n) { check(nullptr, leon_device_upload(dev, d, src, n), "leon_device_upload"); };
    const uint64_t head = o._gz ? BgzfWriter::HEAD : 0;       // `-gz`: room for the carry right in front of the text
    if (!d_text.try_alloc(dev, head + n_text + 64)) return false;
    if (o._gzRecords && !d_rec.try_alloc(dev, (g_reads + 1) * 8)) return false;       // `-gz-records`: the records' offsets stay on the device
    uint8_t* const d_txt = d_text.as<uint8_t>() + head;
    if (m.fastq_out && !R.d_qual) {
        if (!d_qual.try_alloc(dev, g_bases + 64)) return false;
        upload(d_qual.get(), R.qual.data(), g_bases);
    }
    const uint8_t* const quals = R.d_qual ? R.d_qual.as<uint8_t>() : d_qual.as<uint8_t>();
    const uint8_t* hp = nullptr; const uint64_t* ho = nullptr;
    uint64_t hb = 0;
    if (m.has_header && R.hdr_in_set) { hp = R.d_hdr; ho = R.d_hdr_off; hb = R.d_hdr_size; }
    else if (m.has_header) {                                 // decoded on the host (`-header-text host`, or a block the kernel declined): up it goes
        hb = R.hdr_off[g_reads] - R.hdr_off[0];
        if (!d_hdr.try_alloc(dev, hb + 64) || !d_hoff.try_alloc(dev, (g_reads + 1) * 8)) return false;
        upload(d_hdr.get(), R.hdr.data() + R.hdr_off[0], hb);
        upload(d_hoff.get(), R.hdr_off.data(), (g_reads + 1) * 8);
        hp = d_hdr.as<uint8_t>(); ho = d_hoff.as<uint64_t>();
    }
    leon_record_layout lay{};
    lay.struct_size = (uint32_t)sizeof(lay); lay.lead = (uint8_t)m.lead; lay.fastq = m.fastq_out ? 1 : 0; lay.plus_kind = m.fastq_out && m.plus.def == 1 ? 1 : 0;
    lay.wrap = (uint32_t)std::min<uint64_t>(m.wrap, 0xFFFFFFFFull); lay.first_read_index = R.read_index; lay.hdr_bytes = hb;
    uint64_t size = 0;
    if (o._bam) {
        bam_check(leon_records_bam_device(dev, &lay, R.d_bases(), R.dna->d_lens.as<uint32_t>() + R.read0, g_reads, g_bases, hp, ho, m.fastq_out ? quals : nullptr, d_txt,
                                          n_text, o._gzRecords ? d_rec.as<uint64_t>() : nullptr, &size), "leon_records_bam_device");
    } else {
        const int rc = leon_records_format_device(dev, &lay, R.d_bases(), R.dna->d_lens.as<uint32_t>() + R.read0, g_reads, g_bases, hp, ho, quals, d_txt, n_text,
                                                  o._gzRecords ? d_rec.as<uint64_t>() : nullptr, &size);
        if (rc == LEON_E_OVERFLOW || (rc == LEON_OK && size != n_text)) throw Exception(file + ": the decoded reads do not add up to their blocks' sizes");
        check(nullptr, rc, "leon_records_format_device");
    }
    R.d_qual.reset();
    if (o._gz) gz.from_device(d_txt, size, o._gzRecords ? d_rec.as<uint64_t>() : nullptr, g_reads, R.last);    // one call instead of the downloads
    else download_text(R, d_txt);
    rt_rounds_on_device++;
    lap(tl, t_text);
    return true;
}

// `-bam`: room for the round's records without looking at the names: a record is 36 bytes, its header's bytes and at most 5 more (a
// "*", two NULs, the tag of a comment -- its separator is not written), a nybble and a quality byte per base
uint64_t Decoder::bam_bound(const Round& R) const {
    const uint64_t g = R.g_reads;
    const uint64_t hdr_total = !m.has_header ? 20 * g : R.hdr_in_set ? R.d_hdr_size : R.hdr_off[g] - R.hdr_off[0];
    return 41 * g + hdr_total + R.g_bases + (R.g_bases + g) / 2 + 1;
}

// a read that BAM cannot hold ends the run in the formatter's words: "<file>: -bam: read N: ..."
void Decoder::bam_check(int rc, const char* what) const {
    if (rc == LEON_E_INVALID) {
        const std::string why = leon_last_error(nullptr);
        const size_t at = why.find(": read ");
        if (at != std::string::npos) throw Exception(file + ": -bam: " + why.substr(at + 2));
    }
    if (rc == LEON_E_OVERFLOW) throw Exception(file + ": the decoded reads do not add up to their blocks' sizes");
    check(nullptr, rc, what);
}

// the writing stage of `-bam` on the host: the records of leon_host_records_bam, compressed where `-gz` compresses the text
void Decoder::write_round_bam_host(Round& R) {
    auto tl = std::chrono::steady_clock::now();
    const uint64_t g_reads = R.g_reads, head = BgzfWriter::HEAD, cap = bam_bound(R);
    check_qual_lengths(R);
    if (head + cap > text_cap) { text.reset(); text_cap = head + cap + cap / 16; text.reset(new char[text_cap]); }
    uint8_t* const tbase = reinterpret_cast<uint8_t*>(text.get()) + head;
    leon_record_layout lay{};
    lay.struct_size = (uint32_t)sizeof(lay); lay.lead = (uint8_t)m.lead; lay.fastq = m.fastq_out ? 1 : 0;
    lay.first_read_index = R.read_index; lay.hdr_bytes = m.has_header ? R.hdr_off[g_reads] - R.hdr_off[0] : 0;
    std::vector<uint64_t> rec_off(g_reads + 1, 0);
    uint64_t size = 0;
    bam_check(leon_host_records_bam(&lay, R.bases(), R.lens(), g_reads, R.g_bases, m.has_header ? R.hdr.data() + R.hdr_off[0] : nullptr,
                                    m.has_header ? R.hdr_off.data() : nullptr, m.fastq_out ? R.qual.data() + R.qual_off[0] : nullptr, tbase, cap, rec_off.data(), &size,
                                    n_cpu), "leon_host_records_bam");
    gz.from_host(tbase, size, rec_off, R.last);
    lap(tl, t_text);
}

// the text comes back in pinned pieces, each written where it landed; a download keeps up to three copies in flight (PCIe's
// rate), the page cache takes more writers than that: four downloads side by side, each its own quarter of the text
void Decoder::download_text(const Round& R, const uint8_t* d_txt) {
    const uint64_t n_text = R.n_text, piece = 16ull << 20, n_pieces = (n_text + piece - 1) / piece;
    const uint32_t n_dl = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, n_pieces / 4));
    std::vector<int> dl_rc(n_dl, LEON_OK);
    std::vector<std::string> dl_err(n_dl);
    auto download = [&](uint32_t i) {
        const uint64_t a = n_pieces * i / n_dl * piece, b = std::min(n_text, n_pieces * (i + 1) / n_dl * piece);
        FileSink out{ofd.fd, R.file_off + a};
        dl_rc[i] = leon_device_download_pieces(dev, d_txt + a, b - a, FileSink::piece, &out);
        if (dl_rc[i] != LEON_OK) dl_err[i] = leon_last_error(nullptr);       // (the message is the calling thread's)
    };
    {
        std::vector<std::thread> th;
        for (uint32_t i = 1; i < n_dl; i++) th.emplace_back(download, i);
        download(0);
        for (auto& t : th) t.join();
    }
    for (uint32_t i = 0; i < n_dl; i++) {
        if (dl_rc[i] == LEON_E_SINK) throw Exception("cannot write " + o._outputFilename);
        if (dl_rc[i] != LEON_OK) throw Exception("leon_device_download_pieces: " + dl_err[i]);
    }
}

// ... and a round that found no device memory for its text: its bases (and header text) come to the host after all
void Decoder::round_to_host(Round& R) {
    R.own_bases.resize(R.g_bases + 1);
    check(nullptr, leon_device_download(dev, R.own_bases.data(), R.d_bases(), R.g_bases), "leon_device_download");
    if (R.hdr_in_set) {
        uint64_t need = 0;
        R.hdr.resize(R.d_hdr_size + 1);
        check(nullptr, leon_header_text_fetch(hdr_text_set->h, R.block0, R.nb, R.hdr.data(), R.hdr.size(), R.hdr_off.data(), &need), "header blocks");
        R.hdr_in_set = false;
    }
    if (R.d_qual) {                                          // (`-qual-inflate device`: so do its qualities)
        R.qual.resize(R.g_bases + 1);
        check(nullptr, leon_device_download(dev, R.qual.data(), R.d_qual.get(), R.g_bases), "leon_device_download");
        R.d_qual.reset();
    }
    rt_rounds_no_memory++;
}

// ------------------------------------------------------------------------------------------------ the end
void Decoder::finish() {
    {
        auto tl = std::chrono::steady_clock::now();
        while (!pending.empty()) { pending.front().get(); pending.pop_front(); }
        lap(tl, t_write);
    }
    if (o._bam && !gz.closed) {                               // (a file without a round: the BAM header and the EOF marker)
        std::vector<uint8_t> room(BgzfWriter::HEAD + 64);
        gz.from_host(room.data() + BgzfWriter::HEAD, 0, std::vector<uint64_t>(1, 0), true);
    } else if (o._gz && !gz.closed) {                         // (a file without a round: the EOF marker alone)
        if (!gz.carry.empty()) throw Exception("-gz: text was left over behind the last round");
        (void)gz.compress(nullptr, 0, 0, nullptr, 0, true);
    }
    if (::close(ofd.fd) != 0) { ofd.fd = -1; throw Exception("cannot write " + o._outputFilename); }
    ofd.fd = -1;
    if (read_index != m.p.n_reads) throw Exception("the block tables do not add up to the header's read count");
    if (o._gzIndex) {
        // the .gzi: a little-endian count, then (offset in the file, offset in the text) of every data member but the first
        std::vector<uint64_t> words(1, gz.members ? gz.members - 1 : 0);
        if (gz.gzi.size() != 2 * gz.members) throw Exception("-gz-index: the members' places do not add up");
        if (gz.members) words.insert(words.end(), gz.gzi.begin() + 2, gz.gzi.end());
        std::vector<uint8_t> bytes(words.size() * 8);
        for (size_t i = 0; i < words.size(); i++) for (int b = 0; b < 8; b++) bytes[8 * i + b] = (uint8_t)(words[i] >> (8 * b));
        const bool wrote = write_all(gzi_fd.fd, bytes.data(), bytes.size(), 0);
        const bool closed = ::close(gzi_fd.fd) == 0;
        gzi_fd.fd = -1;
        if (!wrote || !closed) throw Exception("cannot write " + o._outputFilename + ".gzi");
    }
    if (o._gz && std::rename(out_path.c_str(), o._outputFilename.c_str()) != 0) throw Exception("cannot write " + o._outputFilename);
    ofd.keep = true;
    if (o._gzIndex) {
        if (std::rename(gzi_fd.path.c_str(), (o._outputFilename + ".gzi").c_str()) != 0) {
            std::remove(o._outputFilename.c_str());          // neither file is left
            throw Exception("cannot write " + o._outputFilename + ".gzi");
        }
        gzi_fd.keep = true;
    }
}

// "device (kernel), N round(s)[, M round(s) on the host threads for want of device memory]"
std::string rounds_text(const char* kernel, uint64_t on_device, uint64_t no_memory) {
    return std::string("device (") + kernel + "), " + std::to_string(on_device) + " round(s)" +
           (no_memory ? ", " + std::to_string(no_memory) + " round(s) on the host threads for want of device memory" : std::string());
}

void Decoder::report() {
    const uint64_t n_blocks = m.p.n_blocks;
    std::cout << m.p.n_reads << " reads, " << bases_out << " bases decoded from " << n_blocks << " blocks, written to " << o._outputFilename << std::endl;
    if (!o._verbose) return;
    std::cout << "time: " << seconds_since(t_start) << " s (" << (n_blocks + group - 1) / group << " round(s); container reads " << t_read << ", dictionary + DNA blocks on the device " << t_dna
              << "; beside them, a round behind: header blocks " << t_hdr << " + quality blocks " << t_qual << "; another round behind: formatting + writing "
              << t_text << "; waited for them " << t_writer_wait + t_write << ")" << std::endl;
    if (m.has_sums) {
        auto way = [&](int st, bool present) -> std::string { return present ? ways_text(sum_ways[st].load(), "nothing to verify") : "not stored"; };
        std::cout << "checksums: " << n_blocks << " blocks verified (dna: " << way(0, true) << ", header: " << way(1, m.has_header) << ", quality: " << way(2, m.has_qual && m.fastq_out) << ")"
                  << (sum_mismatches.load() ? ", " + std::to_string(sum_mismatches.load()) + " mismatch(es) ignored (-ignore-checksum)" : std::string()) << std::endl;
    }
    if (m.has_letters)
        std::cout << "letters: " << m.lt_runs.size() / 2 << " run(s), " << m.lt_pos.size() << " byte(s) restored (" << ways_text(lt_ways.load(), "nothing to restore") << ")" << std::endl;
    if (m.has_header)
        std::cout << "header text: " << (hdr_text_device ? "device (k_hdr_text), " + std::to_string(hdr_blocks_fell_back.load()) + " of " + std::to_string(n_blocks) + " blocks fell back to the host decoder"
                                                         : hdr_on_device ? std::string("host threads, from symbols decoded on the device") : std::string("host threads"))
                  << std::endl;
    if (!o._bam)
        std::cout << "record text: " << (rt_device ? rounds_text("k_fmt_records", rt_rounds_on_device.load(), rt_rounds_no_memory.load())
                                                   : rt_asked ? "host threads (" + rt_reason + ")" : std::string("host threads"))
                  << std::endl;
    if (m.fastq_out)
        std::cout << "quality blocks: " << (qi_device ? rounds_text("k_qual_inflate", qi_rounds_on_device.load(), qi_rounds_no_memory.load()) : std::string("host threads")) << std::endl;
    if (o._gz)
        std::cout << "output: BGZF on the device (" << (o._gzMatches ? "k_deflate_lz_chunks" : "k_deflate_chunks") << ", k_bgzf_members), " << gz.members << " member(s), " << gz.text << " -> " << gz.file_at << " bytes"
                  << (o._gzRecords ? ", record-aligned" : "")
                  << (o._gzIndex ? ", index " + o._outputFilename + ".gzi (" + std::to_string(gz.members ? gz.members - 1 : 0) + " entries)" : std::string())
                  << (o._bam ? ", records: BAM (" + (rt_device ? rounds_text("k_bam_records", rt_rounds_on_device.load(), rt_rounds_no_memory.load()) : std::string("host threads")) + ")"
                             : std::string())
                  << std::endl;
}

}  // namespace

void Leon::executeDecompression() {
    {
        if (_bam) _gz = true;                                 // -bam turns the BGZF writer on exactly as -gz does
        Decoder d(*this);
        d.run();
    }
    if (_testFile) testDecompressedFile();
}

}  // namespace leon_host
