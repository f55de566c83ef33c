// device_call.h -- what the STATELESS device calls share: calls that take a device_id instead of a context, work on a stream of
// their own and report through leon_last_error(NULL).  Each such call lives in the file of its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/leon_dna.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

namespace leon {

void set_create_error(const std::string& msg);                   // capi.hip: the message behind leon_last_error(NULL)

// the two ways a call without a context fails: with words of its own, or with a HIP call's
inline int dev_fail(int code, const std::string& msg) { set_create_error(msg); return code; }
inline std::string hip_failure(const char* call, hipError_t e) { return std::string(call) + ": " + hipGetErrorString(e); }
#define DEVCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return leon::dev_fail(LEON_E_HIP, leon::hip_failure(#call, e_)); } while (0)

inline const bool g_trace_alloc = getenv("LEON_TRACE_ALLOC") != nullptr;   // measurement aid: device allocations of 1 ms or more on stderr

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    size_t slack = 8;                                            // grown to bytes + bytes / slack + 256
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        auto t0 = std::chrono::steady_clock::now();
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / slack + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); leon_device_trim(); e = hipMalloc(&p, want); }   // (the k-mer counter's parked buffers: kmer_kernels.hip)
        if (e == hipSuccess) cap = want;
        if (g_trace_alloc) {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms >= 1.0) fprintf(stderr, "[leon alloc] %.1f MB in %.1f ms\n", want / 1e6, ms);
        }
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return (T*)p; }
};
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy&) = delete; NoCopy& operator=(const NoCopy&) = delete; };
// a device buffer with an owner -- a call's scope, a context (ctx.h), a set a call hands out: released when the owner goes.
// (DevBuf itself has no destructor: the stateless calls' parked scratch lives as long as the process and must not be freed at exit.)
struct OwnBuf : DevBuf, NoCopy {
    // `bytes` and no slack (tables of gigabytes, sized once); nothing kept on failure
    hipError_t exactly(size_t bytes) { release(); const hipError_t e = hipMalloc(&p, bytes); if (e == hipSuccess) cap = bytes; else p = nullptr; return e; }
    void swap(OwnBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(slack, o.slack); }
    ~OwnBuf() { release(); }
};

// a stream with an owner -- a stateless call (it runs beside calls on the contexts' streams), a context: waited for and destroyed
// when the owner goes
struct CallStream : NoCopy {
    hipStream_t s = nullptr;
    operator hipStream_t() const { return s; }
    ~CallStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};
inline int dev_stream(CallStream& st) { DEVCHK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking)); return LEON_OK; }
// the call `who` goes to its device ...
inline int dev_select(const char* who, int device_id) {
    if (hipSetDevice(device_id) != hipSuccess) { (void)hipGetLastError(); return dev_fail(LEON_E_NO_DEVICE, std::string(who) + ": no such HIP device"); }
    return LEON_OK;
}
// ... and opens its stream there
inline int dev_open(const char* who, int device_id, CallStream& st) {
    if (const int rc = dev_select(who, device_id)) return rc;
    return dev_stream(st);
}

}  // namespace leon
