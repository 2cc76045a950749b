// Host side only: the library's status convention and the owners of what the host code takes from the HIP runtime.  Every device
// buffer, pinned word, event and stream of mj_capi.hip is held by one of these move-only types and released by its destructor, so
// an early return can neither leak nor leave a freed address behind.  A call that can fail builds into locals and moves them into
// the pool as its last step (include/mortal_amd.h: a call that returns an error leaves the pool as it was before the call).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>

namespace {

thread_local std::string g_err;
int fail(const std::string& msg) {
    g_err = msg;
    return -1;
}
#define HIP_OK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// reset() releases now, the destructor at the latest; move assignment swaps, so what the target held goes with the source.  hipFree
// synchronises: a call's temporaries go at its return, behind the stream synchronise that ends the call.
template <class T> class DevBuf {  // device memory
    T* h_ = nullptr;
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(h_, o.h_); return *this; }
    ~DevBuf() { reset(); }
    int alloc(size_t count) { reset(); HIP_OK(hipMalloc(&h_, count * sizeof(T))); return 0; }  // `count` elements; the library's status
    T* get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() { if (h_) hipFree(h_); h_ = nullptr; }
};
template <class T> class PinnedBuf {  // pinned host memory
    T* h_ = nullptr;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(h_, o.h_); return *this; }
    ~PinnedBuf() { reset(); }
    int alloc(size_t count) { reset(); HIP_OK(hipHostMalloc(&h_, count * sizeof(T))); return 0; }
    T* get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() { if (h_) hipHostFree(h_); h_ = nullptr; }
};
class Event {
    hipEvent_t h_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Event& operator=(Event&& o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Event() { reset(); }
    int create() { reset(); HIP_OK(hipEventCreate(&h_)); return 0; }  // with timing (EventTimer)
    int create_no_timing() { reset(); HIP_OK(hipEventCreateWithFlags(&h_, hipEventDisableTiming)); return 0; }
    hipEvent_t get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() { if (h_) hipEventDestroy(h_); h_ = nullptr; }
};
class Stream {
    hipStream_t h_ = nullptr;
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Stream() { reset(); }
    int create_non_blocking() { reset(); HIP_OK(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking)); return 0; }
    hipStream_t get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() { if (h_) hipStreamDestroy(h_); h_ = nullptr; }
};

}  // namespace
