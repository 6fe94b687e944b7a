// dev_buf.h -- host-only.  The owning types of every handle (orbx_extractor, orbm_matcher and its grid slots, orbv_vocabulary,
// orbk_database, the stereo scratch): a device block (DevBuf) or a page-locked host block (PinBuf) whose pointer and byte capacity
// change only together, and move-only owners of a stream, an event and an instantiated graph (DevStream, DevEvent, DevGraphExec).
// A handle's advertised capacities are derived from its buffers, so no call can run on a block smaller than the handle claims, and a
// handle's destructor is its members' destructors: nothing is freed from a hand-written list.
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

// A stream, an event or an instantiated graph with one owner: empty by default, destroyed by reset() and by the destructor.
template <class H, hipError_t (*kDestroy)(H)>
class DevHandle {
protected:
    H h_ = nullptr;
public:
    DevHandle() = default;
    explicit DevHandle(H h) : h_(h) {}
    DevHandle(const DevHandle &) = delete;
    DevHandle &operator=(const DevHandle &) = delete;
    DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevHandle &operator=(DevHandle &&o) noexcept
    {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~DevHandle() { reset(); }
    void reset()
    {
        if (h_) (void)kDestroy(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }
protected:
    // what create() of the owners below shares: on failure the owner is empty and the call returns ORBX_E_HIP through `fail`
    template <class Create> int create_with(Create create, dev_fail_fn fail, const char *what)
    {
        reset();
        const hipError_t e = create(&h_);
        if (e == hipSuccess) return ORBX_OK;
        h_ = nullptr;
        (void)hipGetLastError();
        return fail(ORBX_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }
};
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {
    int create(dev_fail_fn fail, const char *what) { return create_with([](hipStream_t *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }, fail, what); }
};
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
    int create(unsigned flags, dev_fail_fn fail, const char *what) { return create_with([flags](hipEvent_t *e) { return hipEventCreateWithFlags(e, flags); }, fail, what); }
};
// a graph is instantiated from a capture, which may fail without being an error: the owner takes what the capture gave (or nothing)
struct DevGraphExec : DevHandle<hipGraphExec_t, hipGraphExecDestroy> { using DevHandle::DevHandle; };
