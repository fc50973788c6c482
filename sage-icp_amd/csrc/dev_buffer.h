// Owners of the host side's device memory (hipMalloc) and pinned host memory (hipHostMalloc): one block each,
// freed by the destructor, moved but never copied.  The caller decides how much to hold (the growth policies stay
// at the call sites: capacities reach the kernels); the owner only allocates, keeps a prefix when asked, and frees.
// Beside them, the owner of a one-call stream.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

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

// The stream of one call, created on the current device: the destructor waits for it, then destroys it.  Declared
// after the buffers its work uses, it goes first, so no buffer is freed under a copy or a kernel still running.
class OwnedStream {
public:
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    OwnedStream &operator=(const OwnedStream &) = delete;
    ~OwnedStream() {
        if (!s_) return;
        (void)hipStreamSynchronize(s_);
        (void)hipStreamDestroy(s_);
    }

    hipError_t create() { return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    hipStream_t get() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace sageicp
