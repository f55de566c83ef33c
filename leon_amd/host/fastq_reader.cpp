#include "fastq_reader.hpp"

#include <fcntl.h>

#include <cerrno>
#include <iostream>

namespace leon_host {

namespace {

const char* const kReasons[] = {"", "its first line does not begin with '@'", "its third line does not begin with '+'", "sequence and quality lengths differ",
                                "a '+' line of another kind", "the text ends inside it"};
const char* const kFastaReasons[] = {"", "text in front of the first header line", "a record without sequence", "an empty sequence line", "a line of another width",
                                     "the first record on more than one line"};
constexpr uint64_t kHandOffReads = 1024;                      // reads the host parser takes before the device is asked again
constexpr uint64_t kCallBytes = 1ull << 31;                    // the most text one call is given (the call refuses 2^32 and more)

void grow(int device, DeviceMem& m, uint64_t cap, uint64_t used, uint64_t want) {
    DeviceMem g;
    g.alloc(device, want + 64);
    if (used) check(nullptr, leon_device_copy(device, g.get(), m.get(), std::min(used, cap)), "leon_device_copy");
    m = std::move(g);
}

}  // namespace

void DeviceBatch::reserve(uint64_t header_need, uint64_t base_need) {
    if (header_need > header_cap) {
        const uint64_t want = header_need + header_need / 4 + 4096;
        grow(device, headers, header_cap, header_bytes, want);
        header_cap = want;
    }
    if (base_need > base_cap) {
        const uint64_t want = base_need + base_need / 4 + 4096;
        grow(device, bases, base_cap, base_bytes, want);
        if (with_quals) grow(device, quals, base_cap, base_bytes, want);
        base_cap = want;
    }
}

FastqDeviceReader::FastqDeviceReader(const std::string& path, int device, bool bgzf, bool verbose, bool fasta)
    : path_(path), device_(device), verbose_(verbose), fasta_(fasta), host_(path, Bank::Memory(), fasta) {
    if (const char* e = getenv("LEON_PARSE_SPAN_KB")) { const long long kb = atoll(e); if (kb >= 1 && kb <= (1ll << 20)) span_bytes_ = (uint64_t)kb << 10; }
    if (bgzf) bgzf_.reset(new BgzfDeviceText(path, device));
    else {
        fd_ = ::open(path.c_str(), O_RDONLY);
        if (fd_ < 0) throw Exception("cannot open " + path);
    }
}
FastqDeviceReader::~FastqDeviceReader() {
    if (fd_ >= 0) ::close(fd_);
    for (Window& w : win_) leon_host_pinned_free(w.pinned);
}

// room for `need` bytes; what the window held is not kept
void FastqDeviceReader::fit(Window& w, uint64_t need) {
    if (need <= w.cap) return;
    const uint64_t want = need + need / 8 + 64;
    w.d.alloc(device_, want);
    if (!bgzf_) {
        leon_host_pinned_free(w.pinned); w.pinned = nullptr; w.cap = 0;
        void* p = nullptr;
        check(nullptr, leon_host_pinned_alloc(device_, want, &p), "leon_host_pinned_alloc");
        w.pinned = static_cast<char*>(p);
    }
    w.cap = want;
}

bool FastqDeviceReader::load() {
    if (eof_) return false;
    Window& cur = win_[w_];
    Window& nxt = win_[w_ ^ 1];
    const uint64_t keep = cur.len - pos_;
    uint64_t got = 0;
    if (bgzf_) {
        got = bgzf_->next([&](uint64_t n_text) {
            fit(nxt, keep + n_text);
            return nxt.d.as<uint8_t>() + keep;
        });
    } else {
        fit(nxt, keep + span_bytes_);
        while (got < span_bytes_) {
            ssize_t n;
            do { n = ::read(fd_, nxt.pinned + keep + got, span_bytes_ - got); } while (n < 0 && errno == EINTR);
            if (n < 0) throw Exception(std::string("read error in ") + path_ + ": " + strerror(errno));
            if (n == 0) break;
            got += (uint64_t)n;
        }
        if (got) check(nullptr, leon_device_upload(device_, nxt.d.as<char>() + keep, nxt.pinned + keep, got), "leon_device_upload");
    }
    if (!got) { eof_ = true; return false; }
    if (keep) {                                                  // the carried tail, device to device
        check(nullptr, leon_device_copy(device_, nxt.d.get(), cur.d.as<char>() + pos_, keep), "leon_device_copy");
        if (!bgzf_) memcpy(nxt.pinned, cur.pinned + pos_, keep);
    }
    nxt.len = keep + got;
    w_ ^= 1; pos_ = 0;
    return true;
}

const char* FastqDeviceReader::host_text(uint64_t from, uint64_t n) {
    Window& w = win_[w_];
    if (!bgzf_) return w.pinned + from;
    down_.resize(n + 1);
    if (n) check(nullptr, leon_device_download(device_, down_.data(), w.d.as<char>() + from, n), "leon_device_download");
    return down_.data();
}

// The host parser reads on from pos_: up to max_reads records, through the window's end into the spans behind it when a record
// asks for that; the device goes on behind the last byte it took.
void FastqDeviceReader::hand_off(DeviceBatch& batch, uint64_t max_reads, const char* why, uint64_t piece) {
    if (verbose_ && n_hand_offs_ < 4) std::cout << "parse: record " << host_.readsSoFar() + 1 << " handed to the host parser (" << why << ")" << std::endl;
    n_hand_offs_++;
    piece_base_ = pos_;
    if (piece != ~0ull) host_.attach(host_text(pos_, piece), piece, nullptr);       // (the parser meets the end of its piece, not the next record)
    else host_.attach(host_text(pos_, win_[w_].len - pos_), win_[w_].len - pos_, [this](const char*& p, size_t& n) {
        pos_ = win_[w_].len;                                    // (the parser asks when it has taken all of the piece)
        if (!load()) return false;
        piece_base_ = 0;
        p = host_text(0, win_[w_].len); n = win_[w_].len;
        return true;
    });
    taken_.clear();
    const uint64_t got = host_.next(taken_, max_reads);
    pos_ = piece != ~0ull ? piece_base_ + piece : piece_base_ + host_.position();
    host_.attach(nullptr, 0, nullptr);
    if (!got) return;
    if (first_header_.empty() && batch.size() == 0 && n_device_ + n_host_ == 0) first_header_.assign(taken_.headers, 0, taken_.header_off[1]);
    batch.reserve(batch.header_bytes + taken_.headers.size(), batch.base_bytes + taken_.bases.size());
    if (!taken_.headers.empty()) check(nullptr, leon_device_upload(device_, batch.headers.as<char>() + batch.header_bytes, taken_.headers.data(), taken_.headers.size()), "leon_device_upload");
    if (!taken_.bases.empty()) {
        check(nullptr, leon_device_upload(device_, batch.bases.as<char>() + batch.base_bytes, taken_.bases.data(), taken_.bases.size()), "leon_device_upload");
        if (!fasta_) check(nullptr, leon_device_upload(device_, batch.quals.as<char>() + batch.base_bytes, taken_.quals.data(), taken_.quals.size()), "leon_device_upload");
    }
    for (uint64_t i = 1; i <= got; i++) {
        batch.header_off.push_back(batch.header_bytes + taken_.header_off[i]);
        batch.base_off.push_back(batch.base_bytes + taken_.base_off[i]);
    }
    batch.header_bytes += taken_.headers.size(); batch.base_bytes += taken_.bases.size();
    n_host_ += got;
}

// one call of the device split on what the window has left, up to `want` reads for the batch
void FastqDeviceReader::split(DeviceBatch& batch, uint64_t want) {
    Window& w = win_[w_];
    const uint64_t need = want - batch.size(), n_text = std::min(w.len - pos_, kCallBytes);
    const uint64_t records_cap = std::min(need, n_text / 4 + 1) + 1;
    const bool to_the_end = n_text == w.len - pos_;               // the call sees all the window has left
    batch.reserve(batch.header_bytes + n_text, batch.base_bytes + n_text);
    uint64_t* const d_ho = static_cast<uint64_t*>(d_header_off_.fit(device_, records_cap * 8));
    uint64_t* const d_bo = static_cast<uint64_t*>(d_base_off_.fit(device_, records_cap * 8));
    leon_fastq_split_result r;
    check(nullptr, leon_fastq_split_device(device_, w.d.as<uint8_t>() + pos_, n_text, 0, need, host_.plusDefault(), batch.headers.as<uint8_t>() + batch.header_bytes, d_ho,
                                           batch.bases.as<uint8_t>() + batch.base_bytes, d_bo, batch.quals.as<uint8_t>() + batch.base_bytes, n_text, records_cap, &r),
          "leon_fastq_split_device");
    if (r.n_records) {
        off_.resize(2 * (r.n_records + 1));
        check(nullptr, leon_device_download(device_, off_.data(), d_ho, (r.n_records + 1) * 8), "leon_device_download");
        check(nullptr, leon_device_download(device_, off_.data() + r.n_records + 1, d_bo, (r.n_records + 1) * 8), "leon_device_download");
        for (uint64_t i = 1; i <= r.n_records; i++) {
            batch.header_off.push_back(batch.header_bytes + off_[i]);
            batch.base_off.push_back(batch.base_bytes + off_[r.n_records + 1 + i]);
        }
        batch.header_bytes += r.header_bytes; batch.base_bytes += r.base_bytes;
        host_.skipped(r.n_records);
        n_device_ += r.n_records;
        pos_ += r.consumed;
    }
    if (r.stop == LEON_FASTQ_IRREGULAR) hand_off(batch, std::min(want - batch.size(), kHandOffReads), kReasons[r.reason]);
    else if (r.stop == LEON_FASTQ_END) {
        if (n_text == kCallBytes && !r.n_records) throw Exception(path_ + ": a record of more than 2 GiB: read this file with -record-parse host");
        // more text behind what is left -- or, at the end of the file, the host parser for what is left: a last record without its
        // newline, blank lines, a record cut short
        if (to_the_end && !load() && pos_ < win_[w_].len) hand_off(batch, want - batch.size(), "the end of the file");
    }
}

// FASTA: one call of the device split on what the window has left, up to `want` reads for the batch, under the `wrap` the host parser's
// bookkeeping asks for.  An irregular record goes to the parser alone, as text[consumed, next_header): whatever it was irregular in, the
// parser's answer moves the mode on (0 -> the width -> any), so a file has at most two such hand-offs.
void FastqDeviceReader::split_fasta(DeviceBatch& batch, uint64_t want) {
    Window& w = win_[w_];
    const uint64_t need = want - batch.size(), n_text = std::min(w.len - pos_, kCallBytes);
    const uint64_t records_cap = std::min(need, n_text / 2 + 1) + 1;
    const bool to_the_end = n_text == w.len - pos_;
    batch.reserve(batch.header_bytes + n_text, batch.base_bytes + n_text);
    uint64_t* const d_ho = static_cast<uint64_t*>(d_header_off_.fit(device_, records_cap * 8));
    uint64_t* const d_bo = static_cast<uint64_t*>(d_base_off_.fit(device_, records_cap * 8));
    leon_fasta_split_result r;
    check(nullptr, leon_fasta_split_device(device_, w.d.as<uint8_t>() + pos_, n_text, 0, need, host_.fastaWrap(), batch.headers.as<uint8_t>() + batch.header_bytes, d_ho,
                                           batch.bases.as<uint8_t>() + batch.base_bytes, d_bo, n_text, records_cap, &r),
          "leon_fasta_split_device");
    if (r.n_records) {
        off_.resize(2 * (r.n_records + 1));
        check(nullptr, leon_device_download(device_, off_.data(), d_ho, (r.n_records + 1) * 8), "leon_device_download");
        check(nullptr, leon_device_download(device_, off_.data() + r.n_records + 1, d_bo, (r.n_records + 1) * 8), "leon_device_download");
        for (uint64_t i = 1; i <= r.n_records; i++) {
            batch.header_off.push_back(batch.header_bytes + off_[i]);
            batch.base_off.push_back(batch.base_bytes + off_[r.n_records + 1 + i]);
        }
        batch.header_bytes += r.header_bytes; batch.base_bytes += r.base_bytes;
        host_.skipped(r.n_records, r.single_max);
        n_device_ += r.n_records;
        pos_ += r.consumed;
    }
    if (r.stop == LEON_FASTA_IRREGULAR) hand_off(batch, 1, kFastaReasons[r.reason], r.next_header - r.consumed);
    else if (r.stop == LEON_FASTA_END) {
        if (n_text == kCallBytes && !r.n_records) throw Exception(path_ + ": a record of more than 2 GiB: read this file with -record-parse host");
        // more text behind what is left -- or, at the end of the file, the host parser for the last record: the end of the file ends it
        if (to_the_end && !load() && pos_ < win_[w_].len) hand_off(batch, want - batch.size(), "the end of the file");
    }
}

// FASTA: the file's first record goes to the host parser, bounded like every other: a call that splits nothing it keeps (any width, one
// record) finds where the record ends, with more of the file loaded until it is whole.  What lies in front of the first header line --
// blank lines, or what the parser refuses -- goes to the parser with it.
void FastqDeviceReader::first_fasta_record(DeviceBatch& batch) {
    uint64_t front = 0;                                          // bytes in front of the first header line
    for (;;) {
        Window& w = win_[w_];
        const uint64_t n_text = std::min(w.len - pos_ - front, kCallBytes);
        batch.reserve(n_text, n_text);
        uint64_t* const d_ho = static_cast<uint64_t*>(d_header_off_.fit(device_, 2 * 8));
        uint64_t* const d_bo = static_cast<uint64_t*>(d_base_off_.fit(device_, 2 * 8));
        leon_fasta_split_result r;
        check(nullptr, leon_fasta_split_device(device_, w.d.as<uint8_t>() + pos_ + front, n_text, 0, 1, LEON_FASTA_ANY_WIDTH, batch.headers.as<uint8_t>(), d_ho,
                                               batch.bases.as<uint8_t>(), d_bo, n_text, 2, &r),
              "leon_fasta_split_device");
        if (r.stop == LEON_FASTA_IRREGULAR && r.next_header < n_text) { front += r.next_header; continue; }      // (R_HEADER: on from the first header line)
        if (r.n_records == 1) { hand_off(batch, 1, "the file's first record", front + r.consumed); return; }
        if (n_text == kCallBytes) throw Exception(path_ + ": a record of more than 2 GiB: read this file with -record-parse host");
        if (!load()) { hand_off(batch, 1, "the file's first record"); return; }     // the file has one record, or none
    }
}

uint64_t FastqDeviceReader::next(DeviceBatch& batch, uint64_t want) {
    batch.device = device_;
    batch.with_quals = !fasta_;
    batch.clear();
    batch.reserve(1, 1);                                         // (every blob is there, also for a batch of empty lines)
    if (!started_) {                                             // the file's first record says which kind the '+' lines are of
        started_ = true;
        if (load()) { if (fasta_) first_fasta_record(batch); else hand_off(batch, 1, "the file's first record"); }
    }
    while (batch.size() < want) {
        if (pos_ == win_[w_].len && !load()) break;
        if (fasta_) split_fasta(batch, want); else split(batch, want);
    }
    return batch.size();
}

void FastqDeviceReader::report() const {
    std::cout << "parse: " << n_device_ << " records split on the device (" << kernel() << "), " << n_host_ << " read by the host parser in " << n_hand_offs_ << " hand-off(s)" << std::endl;
}

}  // namespace leon_host
