// Owners of device and pinned host memory: the only place in csrc/ that allocates (but for the raw
// pointers msd_dev_alloc / msd_dev_free and ingest.hip's pinned entry points hand across the C
// boundary).  A plan or cache holds its buffers as members; destroying it frees them.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/msdsp.h"

namespace msd {

int hip_fail(hipError_t e, const char *what);

// n elements of device memory, on the device current at alloc (the caller's DeviceGuard)
template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }

  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }

    // a new block of n elements, contents undefined; a block held before is freed without a
    // synchronize (the caller knows that no work in flight uses it)
    int alloc(size_t n, const char *what) {
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), sizeof(T) * n);
        if (e != hipSuccess) return p_ = nullptr, hip_fail(e, what);
        n_ = n;
        return MSD_OK;
    }
    // alloc and a blocking copy of n host elements
    int upload(const T *host, size_t n, const char *what) {
        if (int rc = alloc(n, what)) return rc;
        const hipError_t e = n ? hipMemcpy(p_, host, sizeof(T) * n, hipMemcpyHostToDevice) : hipSuccess;
        return e == hipSuccess ? MSD_OK : hip_fail(e, what);
    }
    int zero() {
        const hipError_t e = n_ ? hipMemset(p_, 0, sizeof(T) * n_) : hipSuccess;
        return e == hipSuccess ? MSD_OK : hip_fail(e, "hipMemset");
    }
    // at least n elements, contents not kept; the stream is drained before an old block goes
    int grow(size_t n, hipStream_t sync_before_free, const char *what) {
        if (n <= n_) return MSD_OK;
        const hipError_t e = p_ ? hipStreamSynchronize(sync_before_free) : hipSuccess;
        return e == hipSuccess ? alloc(n, what) : hip_fail(e, what);
    }
};

// the same for pinned host memory, in bytes
class PinBuf {
    void *p_ = nullptr;
    size_t bytes_ = 0;

  public:
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() {
        if (p_) (void)hipHostFree(p_);
    }

    void *get() const { return p_; }
    size_t bytes() const { return bytes_; }

    int alloc(size_t bytes, const char *what) {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr, bytes_ = 0;
        const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return p_ = nullptr, hip_fail(e, what);
        bytes_ = bytes;
        return MSD_OK;
    }
    // at least `bytes`, contents not kept; the caller has waited for the copies that use the old block
    int grow(size_t bytes, const char *what) { return bytes <= bytes_ ? MSD_OK : alloc(bytes, what); }
};

}  // namespace msd
