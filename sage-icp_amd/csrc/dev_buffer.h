// Owners of what the host side holds on a device: device memory (hipMalloc) and pinned host memory (hipHostMalloc), one
// block each; streams; events.  Each releases what it holds in its destructor, is moved (the source is left empty) but
// never copied, and does nothing when it holds nothing.  The caller decides how much memory to hold (the growth policies
// stay at the call sites: capacities reach the kernels) and when a stream or an event is created; the owner only
// allocates, keeps a prefix when asked, and releases.
//
// What a handle that holds several of them (Scratch, Prep, sageicp_map, sageicp_pipeline: capi_internal.h, prep.h,
// capi_pipeline.hip) keeps when it goes:
//  - its device is made current before anything is released;
//  - every stream of the handle has been waited for before a buffer that its work may touch is freed and before an
//    event recorded on it is destroyed: the handle's destructor body waits, then the members go in reverse order of
//    declaration, whatever that is (a one-call stream has no handle around it: declared after the buffers its work
//    uses, it goes first);
//  - the pipeline's worker thread is joined (Prefetch, prefetch.h: declared after the Preps) before either Prep goes;
//  - a handle that never created its stream releases nothing and calls nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace sageicp {

struct DeviceMemory {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void *p) { return hipFree(p); }
};

template <unsigned Flags>
struct PinnedMemory {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static hipError_t release(void *p) { return hipHostFree(p); }
};

template <typename T, typename Memory>
class Buffer {
public:
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p_(o.p_), n_(o.n_) {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            n_ = o.n_;
            o.p_ = nullptr;
            o.n_ = 0;
        }
        return *this;
    }
    ~Buffer() { reset(); }

    T *data() const { return p_; }
    size_t capacity() const { return n_; }      // elements
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (p_) (void)Memory::release(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // exactly n elements, the contents dropped: the old block is freed before the new one is allocated, so the
    // peak is the larger of the two.  On failure the owner is empty.
    hipError_t reserve(size_t n) {
        reset();
        void *p = nullptr;
        const hipError_t e = Memory::alloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p);
        n_ = n;
        return hipSuccess;
    }
    // exactly n elements, the first `keep` (at most what is held now) copied over on `s`: the new block is
    // allocated, the copy finished, then the old block freed.  On failure the owner keeps its old block.
    hipError_t grow(size_t n, size_t keep, hipStream_t s) {
        void *p = nullptr;
        hipError_t e = Memory::alloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        keep = std::min(keep, std::min(n, n_));
        if (keep) e = hipMemcpyAsync(p, p_, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)Memory::release(p);
            return e;
        }
        reset();
        p_ = static_cast<T *>(p);
        n_ = n;
        return hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
using DevBuf = Buffer<T, DeviceMemory>;
template <typename T, unsigned Flags = hipHostMallocDefault>
using PinnedBuf = Buffer<T, PinnedMemory<Flags>>;

// A stream, created on the current device into an empty owner: the destructor waits for it, then destroys it.
class OwnedStream {
public:
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    OwnedStream &operator=(const OwnedStream &) = delete;
    OwnedStream(OwnedStream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    OwnedStream &operator=(OwnedStream &&o) noexcept {
        if (this != &o) {
            reset();
            s_ = std::exchange(o.s_, nullptr);
        }
        return *this;
    }
    ~OwnedStream() { reset(); }

    hipError_t create() { return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority); }
    // on the CUs of `mask` only (one bit per CU, `words` words)
    hipError_t create(uint32_t words, const uint32_t *mask) { return hipExtStreamCreateWithCUMask(&s_, words, mask); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }

private:
    void reset() {
        if (!s_) return;
        (void)hipStreamSynchronize(s_);
        (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    hipStream_t s_ = nullptr;
};

// An event, created on the current device into an empty owner, for timing (hipEventDefault) or for ordering only
// (hipEventDisableTiming): the destructor destroys it.
class OwnedEvent {
public:
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent &) = delete;
    OwnedEvent &operator=(const OwnedEvent &) = delete;
    OwnedEvent(OwnedEvent &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    OwnedEvent &operator=(OwnedEvent &&o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~OwnedEvent() { reset(); }

    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e_, flags); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }

private:
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    hipEvent_t e_ = nullptr;
};

}  // namespace sageicp
