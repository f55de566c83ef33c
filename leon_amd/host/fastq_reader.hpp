// fastq_reader.hpp -- `leon -c -record-parse device`: the FASTQ file's records split on the device
// (leon_fastq_split_device), batch by batch, the batches left in device memory.  The text goes through in spans -- read from a plain
// file into pinned memory and uploaded, or the chunks of a BGZF file where leon_bgzf_inflate_device leaves them --, what a span's
// last call did not take is carried in front of the next span, device to device.  Whatever the device is not sure about -- the
// file's first record, an irregular record, what is left at the end of the file -- is read by the host parser (Bank over memory):
// every malformed-input message, the read counter and the '+'-line table are its own.
// `-record-parse-fasta`: the same reader in its FASTA mode -- leon_fasta_split_device, no quality blob; the host parser
// gets the text of exactly the records it is to take (its FASTA loop reads ahead into the next record's header line), keeps the
// line-width bookkeeping and says after every hand-off which `wrap` the device is to be called with.
#pragma once
#include "bank.hpp"
#include "leon_internal.hpp"

namespace leon_host {

// one batch of reads in device memory, the shape of ReadBatch; the offsets on the host
struct DeviceBatch {
    int device = 0;
    DeviceMem headers, bases, quals;
    uint64_t header_cap = 0, base_cap = 0;                      // (the qualities have the bases' room)
    bool with_quals = true;                                     // false: a FASTA batch, `quals` stays empty
    uint64_t header_bytes = 0, base_bytes = 0;
    std::vector<uint64_t> header_off{0}, base_off{0};
    uint64_t size() const { return base_off.size() - 1; }
    void clear() { header_bytes = base_bytes = 0; header_off.assign(1, 0); base_off.assign(1, 0); }
    void reserve(uint64_t header_need, uint64_t base_need);      // what the blobs hold is kept
    BatchView view() const {                                     // (good until the next reserve)
        return BatchView{{nullptr, headers.get(), header_bytes}, {nullptr, bases.get(), base_bytes},
                         {nullptr, with_quals ? quals.get() : nullptr, with_quals ? base_bytes : 0}, header_off.data(), base_off.data(), base_off.data(), size()};
    }
};

class FastqDeviceReader {
public:
    // bgzf: the file is BGZF and its members are inflated on `device`; else it is plain text
    // fasta: the file is FASTA (`-record-parse-fasta`)
    FastqDeviceReader(const std::string& path, int device, bool bgzf, bool verbose, bool fasta = false);
    ~FastqDeviceReader();
    FastqDeviceReader(const FastqDeviceReader&) = delete;
    FastqDeviceReader& operator=(const FastqDeviceReader&) = delete;
    // fills `batch` with exactly `want` reads, fewer at the end of the file; returns their number
    uint64_t next(DeviceBatch& batch, uint64_t want);
    const Bank& parser() const { return host_; }                // the '+'-line table of the whole file, once it has been read
    const std::string& firstHeader() const { return first_header_; }
    uint64_t spanBytes() const { return span_bytes_; }
    void report() const;                                         // -verbose: how the records were shared out

private:
    struct Window {                                              // a piece of the text on the device; plain files: its twin in pinned memory
        DeviceMem d;
        char* pinned = nullptr;
        uint64_t cap = 0, len = 0;
    };
    void fit(Window& w, uint64_t need);
    bool load();                                                 // the rest of the window in front of the next span; false: the file has ended
    const char* host_text(uint64_t from, uint64_t n);            // the window's text [from, from + n) in host memory
    // piece: the bytes from pos_ on the parser is given, and nothing behind them; all ones: what the window has left and the spans behind it
    void hand_off(DeviceBatch& batch, uint64_t max_reads, const char* why, uint64_t piece = ~0ull);
    void split(DeviceBatch& batch, uint64_t want);
    void split_fasta(DeviceBatch& batch, uint64_t want);
    void first_fasta_record(DeviceBatch& batch);
    const char* kernel() const { return fasta_ ? "k_fa_split" : "k_fq_split"; }

    std::string path_, first_header_;
    int device_;
    bool verbose_, fasta_, eof_ = false, started_ = false;
    int fd_ = -1;
    std::unique_ptr<BgzfDeviceText> bgzf_;
    uint64_t span_bytes_ = 32ull << 20;                          // LEON_PARSE_SPAN_KB
    Window win_[2];
    int w_ = 0;
    uint64_t pos_ = 0, piece_base_ = 0;                          // the first byte of win_[w_] not taken; where the piece the host parser reads begins
    Bank host_;
    ReadBatch taken_;                                            // a hand-off's records on their way to the device
    std::vector<char> down_;                                     // BGZF: the text a hand-off downloaded
    ScratchMem d_header_off_, d_base_off_;
    std::vector<uint64_t> off_;
    uint64_t n_device_ = 0, n_host_ = 0, n_hand_offs_ = 0;
};

}  // namespace leon_host
