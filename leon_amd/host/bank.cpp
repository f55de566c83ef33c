#include "bank.hpp"
#include "leon_host.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <cerrno>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <iostream>

namespace leon_host {

static void put_varint(std::string& s, uint64_t v) { while (v >= 0x80) { s.push_back((char)(v | 0x80)); v >>= 7; } s.push_back((char)v); }

std::string Bank::plusLines() const {
    if (plus_default_ <= 0 && plus_exc_.empty()) return std::string();
    std::string out(1, (char)plus_default_);
    return out + plus_exc_;
}

PlusLines PlusLines::decode(const uint8_t* p, uint64_t n) {
    PlusLines L;
    if (!n) return L;
    if (p[0] > 1) throw Exception("malformed '+'-line table");
    L.def = p[0];
    uint64_t at = 1, read = 0;
    auto varint = [&]() -> uint64_t {
        uint64_t v = 0;
        for (uint32_t sh = 0;; sh += 7) {
            if (at >= n || sh > 63) throw Exception("malformed '+'-line table");
            const uint8_t c = p[at++];
            v |= (uint64_t)(c & 0x7F) << sh;
            if (!(c & 0x80)) return v;
        }
    };
    while (at < n) {
        const uint64_t d = varint();
        if (!L.exc.empty() && d == 0) throw Exception("malformed '+'-line table");
        read += d;
        if (at >= n) throw Exception("malformed '+'-line table");
        const uint8_t kind = p[at++];
        if (kind > 2 || kind == L.def) throw Exception("malformed '+'-line table");
        std::string text;
        if (kind == 2) {
            const uint64_t len = varint();
            if (len > n - at) throw Exception("malformed '+'-line table");
            text.assign(reinterpret_cast<const char*>(p) + at, len);
            at += len;
        }
        L.exc.push_back(Exc{read, kind, std::move(text)});
    }
    return L;
}
size_t PlusLines::lower(uint64_t read) const {
    return (size_t)(std::lower_bound(exc.begin(), exc.end(), read, [](const Exc& e, uint64_t r) { return e.read < r; }) - exc.begin());
}

// ---- BGZF input inflated on the device (`-c -input-inflate device`) ----
// The file in chunks of compressed bytes: the members of a chunk are walked (leon_host_bgzf_members), a member cut short by the chunk's
// end is carried in front of the next chunk, the whole ones are inflated by leon_bgzf_inflate_device and their text is downloaded
// into one of two pinned buffers.  produce() runs on a thread of its own for chunk i + 1 while the parser reads chunk i's text.
struct Bank::BgzfSource {
    std::string path;
    int fd = -1, device = 0;
    uint64_t chunk_bytes = 32ull << 20;                          // LEON_INPUT_CHUNK_KB
    uint64_t base = 0, members_before = 0;                       // the file offset of comp[0], and the members of the file in front of it
    bool at_eof = false;                                         // the file has been read to its end
    std::vector<uint8_t> comp;                                   // the carried tail, then the chunk
    std::vector<uint64_t> member_off;
    std::string fail_later;                                      // a truncated file: thrown once the whole members in front of the cut are served
    void* d_text = nullptr; uint64_t d_cap = 0;
    void* pinned[2] = {nullptr, nullptr}; uint64_t pinned_cap[2] = {0, 0};
    std::future<uint64_t> inflight;                              // the bytes of text in pinned[turn]; 0: the end of the file
    int turn = 0;
    bool started = false, done = false;
    std::function<uint8_t*(uint64_t)> place;                     // set: produce() leaves the text at place(its size), device memory, and downloads nothing

    ~BgzfSource() {
        if (inflight.valid()) { try { inflight.get(); } catch (...) {} }
        leon_device_free(d_text);
        leon_host_pinned_free(pinned[0]); leon_host_pinned_free(pinned[1]);
        if (fd >= 0) ::close(fd);
    }
    // more of the file behind comp; false when nothing was left
    bool read_more() {
        if (at_eof) return false;
        const size_t have = comp.size();
        comp.resize(have + chunk_bytes);
        size_t got_all = 0;
        while (got_all < chunk_bytes) {
            ssize_t got;
            do { got = ::read(fd, comp.data() + have + got_all, chunk_bytes - got_all); } while (got < 0 && errno == EINTR);
            if (got < 0) throw Exception(std::string("read error in ") + path + ": " + strerror(errno));
            if (got == 0) { at_eof = true; break; }
            got_all += (size_t)got;
        }
        comp.resize(have + got_all);
        return got_all != 0;
    }
    // the text of the next members into pinned[t]: its size, 0 at the end of the file
    uint64_t produce(int t) {
        for (;;) {
            if (!fail_later.empty()) throw Exception(fail_later);
            read_more();
            if (comp.empty()) return 0;
            uint64_t n_members = 0, n_text = 0, consumed = 0;
            uint32_t stop = 0;
            for (;;) {
                if (member_off.size() < 2) member_off.resize(1024);
                const int rc = leon_host_bgzf_members(comp.data(), comp.size(), at_eof ? 1 : 0, member_off.data(), member_off.size(), &n_members, &n_text, &consumed, &stop);
                if (rc == LEON_E_OVERFLOW) { member_off.resize(n_members + 1 + n_members / 2); continue; }
                if (rc != LEON_OK && stop != LEON_BGZF_TRUNCATED && stop != LEON_BGZF_FOREIGN) throw Exception(std::string("leon_host_bgzf_members: ") + leon_last_error(nullptr));
                break;
            }
            if (stop == LEON_BGZF_FOREIGN)
                throw Exception(path + ": the bytes at " + std::to_string(base + consumed) + " are no BGZF member, behind members that are: read this file with -input-inflate host");
            if (stop == LEON_BGZF_TRUNCATED) {
                fail_later = path + " is truncated or corrupt (the BGZF member at byte " + std::to_string(base + consumed) + " is cut short)";
                if (!n_members) throw Exception(fail_later);
            }
            if (!n_members) continue;                            // (LEON_BGZF_PARTIAL: the chunk is smaller than its first member -- more of the file)
            uint8_t* dst = nullptr;
            uint64_t dst_cap = n_text;
            if (place) dst = place(n_text);                      // (the device reader: the text stays where it asks for it)
            else {
                if (n_text > d_cap) {
                    leon_device_free(d_text); d_text = nullptr; d_cap = 0;
                    const uint64_t want = n_text + n_text / 8 + 64;
                    if (leon_device_alloc(device, want, &d_text) != LEON_OK) throw Exception(std::string("leon_device_alloc: ") + leon_last_error(nullptr));
                    d_cap = want;
                }
                if (n_text > pinned_cap[t]) {
                    leon_host_pinned_free(pinned[t]); pinned[t] = nullptr; pinned_cap[t] = 0;
                    const uint64_t want = n_text + n_text / 8 + 64;
                    if (leon_host_pinned_alloc(device, want, &pinned[t]) != LEON_OK) throw Exception(std::string("leon_host_pinned_alloc: ") + leon_last_error(nullptr));
                    pinned_cap[t] = want;
                }
                dst = static_cast<uint8_t*>(d_text); dst_cap = d_cap;
            }
            uint64_t got_text = 0;
            const int rc = leon_bgzf_inflate_device(device, comp.data(), consumed, member_off.data(), n_members, dst, dst_cap, &got_text, 0, nullptr);
            if (rc == LEON_E_INVALID) {
                // the call counts members and bytes from the chunk's first: said here as they lie in the file (the host way has zlib's words)
                const std::string why = leon_last_error(nullptr);
                unsigned long long m = 0, at = 0;
                if (sscanf(why.c_str(), "BGZF member %llu (at byte %llu)", &m, &at) == 2)
                    throw Exception(std::string("read error in ") + path + ": BGZF member " + std::to_string(members_before + m) + " (at byte " + std::to_string(base + at) + ") does not decode");
                throw Exception(std::string("read error in ") + path + ": " + why);
            }
            if (rc != LEON_OK) throw Exception(std::string("leon_bgzf_inflate_device: ") + leon_last_error(nullptr));
            // (pieces below the size at which the download is staged: straight into the pinned buffer)
            for (uint64_t a = 0; !place && a < got_text; a += 32ull << 20) {
                const uint64_t m = std::min<uint64_t>(32ull << 20, got_text - a);
                if (leon_device_download(device, static_cast<char*>(pinned[t]) + a, static_cast<const char*>(d_text) + a, m) != LEON_OK)
                    throw Exception(std::string("leon_device_download: ") + leon_last_error(nullptr));
            }
            comp.erase(comp.begin(), comp.begin() + (ptrdiff_t)consumed);
            base += consumed; members_before += n_members;
            if (got_text) return got_text;                       // (nothing but empty members: on to the next chunk)
        }
    }
    // the next piece of text: where it lies and its size; 0 at the end of the file.  The piece before it is given up.
    uint64_t next(const char*& p) {
        if (done) return 0;
        if (!started) { started = true; inflight = std::async(std::launch::async, [this] { return produce(0); }); turn = 0; }
        const uint64_t got = inflight.get();                     // (the producer's exceptions surface here)
        if (!got) { done = true; return 0; }
        const int mine = turn;
        turn ^= 1;
        { const int t = turn; inflight = std::async(std::launch::async, [this, t] { return produce(t); }); }
        p = static_cast<const char*>(pinned[mine]);
        return got;
    }
};

Bank::Bank(const std::string& path, int inflate_device, bool verbose) : path_(path) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) throw Exception("cannot open " + path);
    file_bytes_ = (uint64_t)st.st_size;
    // gzip input (magic 1f 8b) goes through zlib; anything else is read as it is
    fd_ = ::open(path.c_str(), O_RDONLY);
    if (fd_ < 0) throw Exception("cannot open " + path);
    unsigned char magic[2] = {0, 0};
    const ssize_t got = ::pread(fd_, magic, 2, 0);
    const bool gzip = got == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (inflate_device >= 0) {
        // BGZF: the file's first bytes are a BGZF member, or the beginning of one (a file cut inside its first member ends as such)
        bool bgzf = false;
        if (gzip) {
            std::vector<uint8_t> head(65536);
            const ssize_t n = ::pread(fd_, head.data(), head.size(), 0);
            uint64_t off[2], n_members = 0, n_text = 0, consumed = 0;
            uint32_t stop = 0;
            (void)leon_host_bgzf_members(head.data(), (uint64_t)std::max<ssize_t>(n, 0), 0, off, 2, &n_members, &n_text, &consumed, &stop);
            bgzf = n_members > 0 || stop == LEON_BGZF_PARTIAL;
        }
        if (bgzf) {
            bz_ = new BgzfSource();
            bz_->path = path; bz_->fd = fd_; bz_->device = inflate_device;
            fd_ = -1;
            if (const char* e = getenv("LEON_INPUT_CHUNK_KB")) { const long long kb = atoll(e); if (kb >= 1 && kb <= (4ll << 20)) bz_->chunk_bytes = (uint64_t)kb << 10; }
            if (verbose) std::cout << "input: BGZF members inflated on the device (k_bgzf_inflate), chunks of " << bz_->chunk_bytes << " bytes" << std::endl;
            return;
        }
        if (verbose) std::cout << "input: read on the host (" << path << (gzip ? " is gzip, but not BGZF" : " is not gzip") << ")" << std::endl;
    }
    buf_.resize(4 << 20);                                         // (the BGZF source serves its pinned buffers instead)
    data_ = buf_.data();
    if (gzip) {
        ::close(fd_); fd_ = -1;
        gz_ = gzopen(path.c_str(), "rb");
        if (!gz_) throw Exception("cannot open " + path);
        gzbuffer((gzFile)gz_, 1 << 20);
    }
}
Bank::Bank(const std::string& path, Memory, bool fasta) : memory_(true), path_(path), decided_(true), fastq_(!fasta) {}

BgzfDeviceText::BgzfDeviceText(const std::string& path, int device) : src_(new Bank::BgzfSource()) {
    src_->path = path; src_->device = device;
    src_->fd = ::open(path.c_str(), O_RDONLY);
    if (src_->fd < 0) { delete src_; throw Exception("cannot open " + path); }
    if (const char* e = getenv("LEON_INPUT_CHUNK_KB")) { const long long kb = atoll(e); if (kb >= 1 && kb <= (4ll << 20)) src_->chunk_bytes = (uint64_t)kb << 10; }
}
BgzfDeviceText::~BgzfDeviceText() { delete src_; }
uint64_t BgzfDeviceText::next(const std::function<uint8_t*(uint64_t)>& place) {
    src_->place = place;
    return src_->produce(0);
}
void Bank::dropSource() {
    delete bz_; bz_ = nullptr;
    if (gz_) gzclose((gzFile)gz_);
    gz_ = nullptr;
    if (fd_ >= 0) ::close(fd_);
    fd_ = -1;
    std::vector<char>().swap(buf_);
    data_ = nullptr; buf_pos_ = buf_len_ = 0;
    memory_ = true; more_ = nullptr;                             // (a read from here on finds the end of the text)
}
Bank::~Bank() { delete bz_; if (gz_) gzclose((gzFile)gz_); if (fd_ >= 0) ::close(fd_); }

// the next piece of the file's text behind data_ (buf_pos_ = 0, buf_len_ its size); false at the end of the file
bool Bank::refill() {
    long got;
    if (memory_) {
        const char* p = nullptr; size_t n = 0;
        if (!more_ || !more_(p, n)) return false;
        data_ = p; buf_pos_ = 0; buf_len_ = n;
        return true;
    }
    if (bz_) {
        const char* p = nullptr;
        const uint64_t n = bz_->next(p);
        if (!n) return false;
        data_ = p; buf_pos_ = 0; buf_len_ = (size_t)n;
        return true;
    }
    if (fd_ >= 0) {
        do { got = (long)::read(fd_, buf_.data(), buf_.size()); } while (got < 0 && errno == EINTR);
        if (got < 0) throw Exception(std::string("read error in ") + path_ + ": " + strerror(errno));
        if (got == 0) return false;
    } else {
        got = gzread((gzFile)gz_, buf_.data(), (unsigned)buf_.size());
        if (got < 0) { int e = 0; throw Exception(std::string("read error in ") + path_ + ": " + gzerror((gzFile)gz_, &e)); }
        if (got == 0) {
            // end of the data -- or of a TRUNCATED .gz, which zlib reports as 0 bytes + Z_BUF_ERROR after handing out
            // what it could inflate: compressing that part and calling it success would lose the rest silently
            int e = 0;
            const char* msg = gzerror((gzFile)gz_, &e);
            if (e != Z_OK && e != Z_STREAM_END) throw Exception(path_ + " is truncated or corrupt (" + (msg && *msg ? msg : "unexpected end of file") + ")");
            return false;
        }
    }
    buf_pos_ = 0; buf_len_ = (size_t)got;
    return true;
}

// one line without its terminator ("\n" or "\r\n"); false at the end of the file
bool Bank::getline(std::string& line) {
    line.clear();
    bool any = false;
    for (;;) {
        if (buf_pos_ == buf_len_ && !refill()) break;
        const char* p = data_ + buf_pos_;
        const char* nl = (const char*)memchr(p, '\n', buf_len_ - buf_pos_);
        any = true;
        if (nl) { line.append(p, (size_t)(nl - p)); buf_pos_ += (size_t)(nl - p) + 1; break; }
        line.append(p, buf_len_ - buf_pos_);
        buf_pos_ = buf_len_;
    }
    if (!line.empty() && line.back() == '\r') line.pop_back();
    return any;
}

bool Bank::isFastq() {
    if (!decided_) {
        std::string l;
        while (getline(l)) {
            if (l.empty()) continue;
            pending_ = l; have_pending_ = true;
            fastq_ = l[0] == '@';
            if (l[0] != '@' && l[0] != '>') throw Exception(path_ + " is neither FASTA nor FASTQ (first record starts with '" + l.substr(0, 1) + "')");
            break;
        }
        decided_ = true;
    }
    return fastq_;
}

// the next line without its terminator, not copied when it ends inside the read buffer (the usual case: a megabyte of
// buffer, lines of a few hundred bytes); valid until the next call
bool Bank::view(const char*& p, size_t& n) {
    if (have_pending_) { have_pending_ = false; p = pending_.data(); n = pending_.size(); return true; }
    if (buf_pos_ < buf_len_) {
        const char* s = data_ + buf_pos_;
        const char* nl = (const char*)memchr(s, '\n', buf_len_ - buf_pos_);
        if (nl) {
            p = s; n = (size_t)(nl - s);
            buf_pos_ += n + 1;
            if (n && p[n - 1] == '\r') n--;
            return true;
        }
    }
    if (!getline(spill_)) return false;                         // crosses a refill (or the file ends without a newline)
    p = spill_.data(); n = spill_.size();
    return true;
}

uint64_t Bank::next(ReadBatch& b, uint64_t max_reads) {
    isFastq();
    uint64_t n = 0;
    const char* p; size_t len;
    while (n < max_reads) {
        if (!view(p, len)) break;
        if (len == 0) continue;
        if (fastq_) {
            if (p[0] != '@') throw Exception("malformed FASTQ record " + std::to_string(n_read_ + 1) + " in " + path_);
            const size_t hdr_at = b.headers.size(), hdr_len = len - 1;
            b.headers.append(p + 1, len - 1);
            if (!view(p, len)) throw Exception("truncated FASTQ record in " + path_);
            const size_t seq_len = len;
            b.bases.append(p, len);
            if (!view(p, len)) throw Exception("truncated FASTQ record in " + path_);
            if (len == 0 || p[0] != '+') throw Exception("malformed FASTQ record " + std::to_string(n_read_ + 1) + " in " + path_);
            {   // the text after the '+': nothing, the header again, or something else
                // (a bare '+' under an empty header is both "bare" and "the header again": whichever the file's default is)
                const int kind = len == 1 ? (hdr_len == 0 && plus_default_ == 1 ? 1 : 0)
                                          : (len - 1 == hdr_len && memcmp(p + 1, b.headers.data() + hdr_at, hdr_len) == 0) ? 1 : 2;
                if (plus_default_ < 0) plus_default_ = kind == 2 ? 0 : kind;
                if (kind != plus_default_) {
                    put_varint(plus_exc_, n_read_ - plus_prev_); plus_prev_ = n_read_;
                    plus_exc_.push_back((char)kind);
                    if (kind == 2) { put_varint(plus_exc_, len - 1); plus_exc_.append(p + 1, len - 1); }
                }
            }
            if (!view(p, len)) throw Exception("truncated FASTQ record in " + path_);
            if (len != seq_len) throw Exception("FASTQ record " + std::to_string(n_read_ + 1) + " of " + path_ + ": quality and sequence lengths differ");
            b.quals.append(p, len);
        } else {
            if (p[0] != '>') throw Exception("FASTA data before the first header in " + path_);
            b.headers.append(p + 1, len - 1);
            uint64_t n_lines = 0, last_len = 0;
            while (view(p, len)) {                                   // sequence lines up to the next header
                if (len && p[0] == '>') { pending_.assign(p, len); have_pending_ = true; break; }
                // wrapped sequences: every line but a record's last must have the same width, the last one 1..width
                if (n_lines) {
                    if (!wrap_seen_) { wrap_seen_ = true; wrap_ = last_len; }
                    if (last_len != wrap_ || wrap_ == 0) wrap_ok_ = false;
                }
                last_len = len; n_lines++;
                b.bases.append(p, len);
            }
            if (n_lines && last_len == 0) wrap_ok_ = false;          // an empty last line would not come back
            if (wrap_seen_ && n_lines && last_len > wrap_) wrap_ok_ = false;
            if (n_lines == 0) single_empty_ = true;
            if (n_lines == 1) single_max_ = std::max<uint64_t>(single_max_, last_len);
        }
        b.header_off.push_back(b.headers.size());
        b.base_off.push_back(b.bases.size());
        b.qual_off.push_back(b.quals.size());
        n++; n_read_++;
    }
    return n;
}

}  // namespace leon_host
