// bank.hpp -- streaming FASTA / FASTQ reader (plain or gzip), the slice of gatb's Bank (bank/impl/BankFasta [RECALLED]) the
// host mirror needs: sequences in file order, each with comment (header text after '>' / '@'), data and quality.
// Out of the hot path's scope ("build writes own minimal parser"); reads the file once, in batches,
// so the host never holds more than one batch of it.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

namespace leon_host {

// one batch of reads as three blobs + offsets, the shape the C-ABI takes
struct ReadBatch {
    std::string bases, headers, quals;
    std::vector<uint64_t> base_off{0}, header_off{0}, qual_off{0};
    uint64_t size() const { return base_off.size() - 1; }
    void clear() { bases.clear(); headers.clear(); quals.clear(); base_off.assign(1, 0); header_off.assign(1, 0); qual_off.assign(1, 0); }
    struct BatchView view() const;
};

// Where a batch lies, for whoever consumes it (`leon -c`'s pass, leon_compress.cpp): every blob in host memory, in device memory, or
// both; the offsets (n + 1 each, from 0) on the host either way.  A ReadBatch gives `host`, a DeviceBatch (fastq_reader.hpp) `dev`.
struct Blob { const char* host = nullptr; const void* dev = nullptr; uint64_t bytes = 0; };
struct BatchView {
    Blob headers, bases, quals;
    const uint64_t* header_off = nullptr; const uint64_t* base_off = nullptr; const uint64_t* qual_off = nullptr;
    uint64_t n = 0;                               // reads
};
inline BatchView ReadBatch::view() const {
    return BatchView{{headers.data(), nullptr, headers.size()}, {bases.data(), nullptr, bases.size()}, {quals.data(), nullptr, quals.size()},
                     header_off.data(), base_off.data(), qual_off.data(), size()};
}

class Bank {
public:
    // throws leon_host::Exception when the file cannot be opened.  inflate_device >= 0 (`-c -input-inflate device`): a BGZF file is
    // inflated by that device, chunk by chunk; any other file is read as without it, and `verbose` says so in one line
    explicit Bank(const std::string& path, int inflate_device = -1, bool verbose = false);
    // A FASTQ parser over text the caller hands over piece by piece (the device reader's hand-offs): no file is opened,
    // `path` is for the messages.  attach() serves [p, p + n), then the pieces `more` gives (false: the end of the file); position() is
    // how much of the piece being served has been taken; skipped(n): n reads the caller split itself, their '+' lines of the default
    // kind -- the read counter and the '+'-line table stay what they would be had next() read those records too.
    struct Memory {};
    typedef std::function<bool(const char*&, size_t&)> More;
    // fasta: a FASTA parser over such text.  fastaWrap() is the `wrap` the device split is to be called with, given what
    // the parser has noted so far: LEON_FASTA_ANY_WIDTH once fastaLineWidth() is 0 for good, the width once one was seen, else 0;
    // skipped(n, single_max): n regular records the caller split itself, the longest of them that sat on one line.
    Bank(const std::string& path, Memory, bool fasta = false);
    uint64_t fastaWrap() const { return (!wrap_ok_ || single_empty_ || (wrap_seen_ && single_max_ > wrap_)) ? ~0ull : wrap_seen_ ? wrap_ : 0; }
    void skipped(uint64_t n, uint64_t single_max) { n_read_ += n; single_max_ = std::max(single_max_, single_max); }
    void attach(const char* p, size_t n, More more) { data_ = p; buf_pos_ = 0; buf_len_ = n; more_ = std::move(more); }
    size_t position() const { return buf_pos_; }
    void skipped(uint64_t n) { n_read_ += n; }
    uint64_t readsSoFar() const { return n_read_; }
    int plusDefault() const { return plus_default_; }             // 0 bare, 1 the header again; -1: no record seen yet
    bool inflatesOnDevice() const { return bz_ != nullptr; }      // a BGZF file under `-input-inflate device`
    bool isGzip() const { return gz_ != nullptr; }                // gzip input inflated by zlib on the reader's thread
    void dropSource();                                            // the file is read by someone else from here on: closes it, gives its buffers up
    ~Bank();
    Bank(const Bank&) = delete;
    Bank& operator=(const Bank&) = delete;
    bool isFastq();                               // decided by the first record's first byte ('@' or '>')
    // appends up to max_reads reads to batch; returns the number appended (0 at the end of the file)
    uint64_t next(ReadBatch& batch, uint64_t max_reads);
    uint64_t bytesEstimate() const { return file_bytes_; }   // size of the file on disk (compressed size for .gz)
    // FASTA: the width every sequence line but a record's last has when the file wraps its sequences consistently, else 0
    // (sequences on one line, or lines of differing widths); valid once the whole file has been read
    uint64_t fastaLineWidth() const { return (wrap_seen_ && wrap_ok_ && !single_empty_ && single_max_ <= wrap_) ? wrap_ : 0; }
    // FASTQ: what follows the '+' of every record's third line, as PlusLines::decode reads it back; empty when every record
    // has a bare "+" (the usual case; nothing is stored then).  Valid once the whole file has been read.
    std::string plusLines() const;
private:
    friend class BgzfDeviceText;
    bool getline(std::string& line);
    bool view(const char*& p, size_t& n);         // the next line where it lies (in the read buffer when it ends there), else assembled in spill_
    bool refill();                                // the next piece of the text behind data_; false at the end of the file
    struct BgzfSource;                            // BGZF input inflated on the device: chunks of the file, one in flight while the previous is parsed
    BgzfSource* bz_ = nullptr;
    bool memory_ = false;                         // Bank(path, Memory): refill() asks more_
    More more_;
    void* gz_ = nullptr;                          // gzFile (gzip input)
    int fd_ = -1;                                 // plain input: read(2) straight into buf_ (zlib's transparent mode copies every byte once more)
    std::string path_, pending_, spill_;
    bool have_pending_ = false, decided_ = false, fastq_ = false;
    std::vector<char> buf_;
    const char* data_ = nullptr;                  // the piece being served: buf_, or one of the BGZF source's pinned buffers
    size_t buf_pos_ = 0, buf_len_ = 0;
    uint64_t file_bytes_ = 0, n_read_ = 0;
    uint64_t wrap_ = 0;
    bool wrap_seen_ = false, wrap_ok_ = true, single_empty_ = false;
    uint64_t single_max_ = 0;                     // longest sequence that sat on one line: must fit the wrap width too
    int plus_default_ = -1;                       // kind of the first record's '+' line (0 bare, 1 repeats the header); -1: none seen
    std::string plus_exc_;                        // the records that differ from it: varint(read index delta), kind, [varint(length), text]
    uint64_t plus_prev_ = 0;
};

// The text of a BGZF file chunk by chunk (LEON_INPUT_CHUNK_KB of the file at a time), inflated on the device and LEFT there: what
// `-c -input-inflate device` reads through Bank, without the download (the device reader of `-record-parse device`).
// The messages are the ones Bank gives for the same file.
class BgzfDeviceText {
public:
    BgzfDeviceText(const std::string& path, int device);
    ~BgzfDeviceText();
    BgzfDeviceText(const BgzfDeviceText&) = delete;
    BgzfDeviceText& operator=(const BgzfDeviceText&) = delete;
    // the next chunk's text at place(its size), device memory with room for it; returns the size, 0 at the end of the file
    uint64_t next(const std::function<uint8_t*(uint64_t)>& place);
private:
    Bank::BgzfSource* src_;
};

// The '+' lines of a FASTQ file (third line of a record): bare, or the header again (older Illumina / SRA dumps), or -- never
// seen, but `diff` would see it -- any other text.  One default kind + the exceptions.
struct PlusLines {
    uint8_t def = 0;
    struct Exc { uint64_t read; uint8_t kind; std::string text; };
    std::vector<Exc> exc;                         // sorted by read
    bool trivial() const { return def == 0 && exc.empty(); }
    static PlusLines decode(const uint8_t* p, uint64_t n);        // throws leon_host::Exception on a malformed blob
    // kind of read `read`'s line (0 bare, 1 header, 2 text); *hint walks the exceptions forwards over increasing reads
    const Exc* find(uint64_t read, size_t* hint) const {
        size_t i = *hint;
        while (i < exc.size() && exc[i].read < read) i++;
        *hint = i;
        return (i < exc.size() && exc[i].read == read) ? &exc[i] : nullptr;
    }
    size_t lower(uint64_t read) const;            // first exception at or after `read`
};

}  // namespace leon_host
