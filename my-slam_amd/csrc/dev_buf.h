// dev_buf.h -- host-only.  The one owning buffer type of the matcher-side handles (orbm_matcher and its grid slots,
// orbv_vocabulary, orbk_database, the stereo scratch): a device block (DevBuf) or a page-locked host block (PinBuf) whose pointer
// and byte capacity change only together.  A handle's advertised capacities are derived from its buffers, so no call can run on a
// block smaller than the handle claims.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/orbx.h"

typedef int (*dev_fail_fn)(int code, const char *fmt, ...);    // a subsystem's mfail / vfail / kfail: sets its *_last_error text

template <class T, bool kPinned = false>
class DevBuf {
    T *p_ = nullptr;
    size_t bytes_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; bytes_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t bytes() const { return bytes_; }
    size_t count() const { return bytes_ / sizeof(T); }
    // The one growth rule.  A buffer that already holds `bytes` stays as it is; otherwise free, then allocate (peak memory is one
    // block; the content is NOT kept).  On failure the buffer is empty (NULL, capacity 0) and the call returns ORBX_E_HIP through
    // `fail`, naming `what`: the next call grows again.  The caller has synchronised whatever may still use the old block.
    int grow(size_t bytes, dev_fail_fn fail, const char *what)
    {
        if (bytes <= bytes_) return ORBX_OK;
        reset();
        void *p = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();       // reported here, not by the next launch check
            return fail(ORBX_E_HIP, "%s: allocating %zu bytes: %s", what, bytes, hipGetErrorString(e));
        }
        p_ = static_cast<T *>(p); bytes_ = bytes;
        return ORBX_OK;
    }
};
template <class T> using PinBuf = DevBuf<T, true>;
