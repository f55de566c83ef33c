// leon_internal.hpp -- what leon_host.cpp (options), leon_compress.cpp (-c) and leon_decompress.cpp (-d) share; not part of the tool's
// public face (leon_host.hpp).
#pragma once
#include "leon_host.hpp"

#include "leon_container.hpp"
#include "leon_plan.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace leon_host {

// threads this process may keep busy: the logical CPUs, capped by the container's CPU quota (cgroup v2 cpu.max)
inline uint64_t usableCpus() {
    uint64_t n = std::max(1u, std::thread::hardware_concurrency());
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64] = {0};
        long long period = 0;
        if (fscanf(f, "%63s %lld", q, &period) == 2 && std::string(q) != "max" && period > 0)
            n = std::min<uint64_t>(n, (uint64_t)std::max<long long>(1, (atoll(q) + period - 1) / period));
        fclose(f);
    }
    return n;
}

inline void check(leon_dna_ctx* ctx, int rc, const char* what) {
    if (rc != LEON_OK) throw Exception(std::string(what) + ": " + leon_last_error(ctx));
}
inline bool ends_with(const std::string& s, const std::string& suffix) {
    return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}
inline double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

struct CtxDeleter { void operator()(leon_dna_ctx* c) const { if (c) leon_dna_ctx_destroy(c); } };
typedef std::unique_ptr<leon_dna_ctx, CtxDeleter> CtxPtr;

inline CtxPtr make_ctx(uint32_t k, uint64_t tai, int device, uint32_t n_hash = 7, uint32_t block_nbits = 12, uint32_t rpb = Leon::READ_PER_BLOCK,
                       uint32_t flags = 0, uint32_t dict_piece_anchors = 0) {
    leon_dna_cfg cfg = {};
    cfg.struct_size = sizeof(cfg);
    cfg.flags = flags; cfg.dict_piece_anchors = dict_piece_anchors;
    cfg.kmer_size = k; cfg.reads_per_block = rpb;
    cfg.bloom_n_hash = n_hash; cfg.bloom_block_nbits = block_nbits; cfg.bloom_tai = tai; cfg.device_id = device;
    leon_dna_ctx* c = nullptr;
    check(nullptr, leon_dna_ctx_create(&cfg, &c), "leon_dna_ctx_create");
    return CtxPtr(c);
}

inline int device_for(int gpu_index) {
    // LEON_SHARE_GPU=1 lets a multi-GPU run rehearse on fewer devices (ranks wrap around); otherwise -gpus must fit
    static const char* share = getenv("LEON_SHARE_GPU");
    static const int n_dev = [] { int n = 0; return leon_device_count(&n) == LEON_OK ? n : 0; }();
    if (n_dev <= 0) throw Exception("no HIP device: the DNA encode path has no CPU fallback");
    if (gpu_index >= n_dev && !(share && share[0] == '1')) throw Exception("-gpus " + std::to_string(gpu_index + 1) + " asked, " + std::to_string(n_dev) + " device(s) present");
    return gpu_index % n_dev;
}

// ---------------------------------------------------------------------------------------------- options
// `-header-text`, `-record-text`, `-qual-inflate` (leon_decompress.cpp says what each chooses): not given, or `host`; `device`; `auto`
enum class Choice { Host, Device, Auto };
inline Choice parse_choice(const char* flag_name, const std::string& value) {
    if (value.empty() || value == "host") return Choice::Host;
    if (value == "device") return Choice::Device;
    if (value == "auto") return Choice::Auto;
    throw Exception(std::string("option ") + flag_name + ": '" + value + "': expected host, device or auto");
}
// the device when asked for, or under `auto` for files of at least auto_blocks blocks
inline bool device_chosen(Choice c, uint64_t n_blocks, uint64_t auto_blocks) {
    return c == Choice::Device || (c == Choice::Auto && n_blocks >= auto_blocks);
}
// `-c -record-parse host|device`: who cuts the FASTQ text into records; no `auto`
inline bool record_parse_on_device(const std::string& value) {
    if (value.empty() || value == "host") return false;
    if (value == "device") return true;
    throw Exception("option -record-parse: '" + value + "': expected host or device");
}
// `-c -input-inflate`: which device inflates a BGZF input (k_bgzf_inflate), or -1: the file is read on the host, as
// without the option.  `auto` chooses the device for files of at least kInputInflateAutoBytes (DESIGN.md 8 has the runs behind it);
// LEON_INPUT_INFLATE_AUTO_KB in the environment overrides that size, so that a test's small file takes the device way under `auto`.
constexpr uint64_t kInputInflateAutoBytes = 64ull << 20;
inline int input_inflate_device(const std::string& value, const std::string& path) {
    const Choice c = parse_choice("-input-inflate", value);
    if (c == Choice::Host) return -1;
    if (c == Choice::Auto) {
        uint64_t least = kInputInflateAutoBytes;
        if (const char* e = getenv("LEON_INPUT_INFLATE_AUTO_KB")) { const long long kb = atoll(e); if (kb >= 0) least = (uint64_t)kb << 10; }
        struct stat st;
        if (::stat(path.c_str(), &st) != 0 || (uint64_t)st.st_size < least) return -1;   // (a file that is not there: the reader says so)
    }
    return device_for(0);
}

// Which encoder writes the quality blocks.  The default is zlib itself on the host threads (leon_host_qual_encode_blocks: compress2 at
// its default level, the bytes upstream writes [RECALLED] and the one stream of the file a third-party library can pin byte for byte).
// `-qual-deflate device` hands them to the device's deflate (leon_qual_deflate_blocks_device), which looks for runs only -- zlib's
// Z_RLE strategy -- and is tens of times faster than zlib's default strategy on all the host's cores; its blocks inflate to the same
// text but are not zlib's bytes.  `-qual-deflate auto` lets a sample decide (the first reads' lines, up to 256 KB, through zlib both
// ways: the device takes the stream unless that would cost more than 2 % -- where the lines resemble one another the default
// strategy's matches against earlier lines win).  Without the flag, LEON_QUAL_DEFLATE=auto|device|host in the environment is the
// tests' hook for the same choice.  The container records who wrote the blocks (layout::P_QUAL_ENCODER).
inline Choice qual_encoder_choice(const std::string& flag) {
    const char* e = flag.empty() ? getenv("LEON_QUAL_DEFLATE") : flag.c_str();
    const char* what = flag.empty() ? "LEON_QUAL_DEFLATE=" : "option -qual-deflate: ";
    if (!e || !*e || !strcmp(e, "host")) return Choice::Host;
    if (!strcmp(e, "auto")) return Choice::Auto;
    if (!strcmp(e, "device")) return Choice::Device;
    throw Exception(std::string(what) + "'" + e + "': expected host, device or auto");
}

// ---------------------------------------------------------------------------------------------- device memory
// one device allocation, freed when its owner goes
class DeviceMem {
public:
    DeviceMem() = default;
    DeviceMem(DeviceMem&& o) noexcept : p_(o.release()) {}
    DeviceMem& operator=(DeviceMem&& o) noexcept { if (this != &o) reset(o.release()); return *this; }
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    ~DeviceMem() { leon_device_free(p_); }
    void reset(void* p = nullptr) { leon_device_free(p_); p_ = p; }
    void* release() { void* p = p_; p_ = nullptr; return p; }
    void* get() const { return p_; }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }
    // false: the device has no memory for it (what was held is gone either way)
    bool try_alloc(int device, uint64_t bytes) { reset(); return leon_device_alloc(device, bytes, &p_) == LEON_OK; }
    void alloc(int device, uint64_t bytes) { reset(); check(nullptr, leon_device_alloc(device, bytes, &p_), "leon_device_alloc"); }
private:
    void* p_ = nullptr;
};
// a device buffer that is used again and again: grown (by an eighth more than asked, and 64 bytes) when a use does not fit
struct ScratchMem {
    DeviceMem mem;
    uint64_t cap = 0;
    void* fit(int device, uint64_t need) {
        if (need > cap) {
            mem.reset(); cap = 0;
            const uint64_t want = need + need / 8 + 64;
            mem.alloc(device, want);
            cap = want;
        }
        return mem.get();
    }
};

// ---------------------------------------------------------------------------------------------- the output file
// n bytes at file_off of fd, however many calls that takes; false: the file system refused
inline bool write_all(int fd, const void* bytes, uint64_t n, uint64_t file_off) {
    for (uint64_t done = 0; done < n;) {
        const ssize_t got = ::pwrite(fd, static_cast<const char*>(bytes) + done, (size_t)std::min<uint64_t>(n - done, 1ull << 30), (off_t)(file_off + done));
        if (got <= 0) return false;
        done += (uint64_t)got;
    }
    return true;
}
// a leon_piece_sink that puts every piece where it belongs in the file: `at` is where offset 0 of the call's bytes lies
struct FileSink {
    int fd; uint64_t at;
    static int piece(void* user, uint64_t offset, const void* bytes, uint64_t n) {
        const FileSink* o = static_cast<const FileSink*>(user);
        return write_all(o->fd, bytes, n, o->at + offset) ? 0 : 1;
    }
};

// ---------------------------------------------------------------------------------------------- block checksums
// (`-c -checksum`, verified by `-d`: DESIGN.md 4.11): zlib's CRC-32 per read block and stream, taken where the bytes lie
// -- leon_crc32_segments_device for bytes in device memory, leon_host_crc32_segments on the host threads for the rest.
// block_off: nb + 1 offsets into the bytes, one segment per block; sums: nb words.
inline void sums_on_device(int device, const void* d_bytes, uint64_t n_bytes, const uint64_t* block_off, uint64_t nb, uint32_t* sums) {
    check(nullptr, leon_crc32_segments_device(device, static_cast<const uint8_t*>(d_bytes), n_bytes, block_off, nb, sums), "leon_crc32_segments_device");
}
inline void sums_on_host(const void* bytes, uint64_t n_bytes, const uint64_t* block_off, uint64_t nb, uint32_t cores, uint32_t* sums) {
    check(nullptr, leon_host_crc32_segments(static_cast<const uint8_t*>(bytes), n_bytes, block_off, nb, cores, sums), "leon_host_crc32_segments");
}
// every rpb-th of a batch's per-read offsets (and the last): the batch's blocks
inline std::vector<uint64_t> block_offsets(const uint64_t* off, uint64_t n_reads, uint64_t rpb) {
    std::vector<uint64_t> b;
    for (uint64_t r = 0; r < n_reads; r += rpb) b.push_back(off[r]);
    b.push_back(off[n_reads]);
    return b;
}

// where the rounds of `-d` did a piece of work, for -verbose: bits gathered over the rounds
enum : uint32_t { ON_DEVICE = 1, ON_HOST = 2 };
inline const char* ways_text(uint32_t ways, const char* none) {
    return ways == ON_DEVICE ? "device" : ways == ON_HOST ? "host threads" : ways ? "device and host threads" : none;
}

}  // namespace leon_host
