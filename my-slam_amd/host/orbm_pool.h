// orbm_pool.h -- the thread-local pool of GPU matcher handles behind the adapters (ORBmatcher.h, MapPointDescriptors.h, NewMapPoints.h).
// The reference builds a matcher on the stack at every call site, so a handle (device buffers + a stream) and its marshalling
// buffers are taken from the pool and go back to it; handles are not re-entrant, threads never share one.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/orbm.h"

namespace ORB_SLAM2 {
namespace orbm_detail {
struct Scratch {                                 // marshalling buffers: they stay with the pooled handle, so a call allocates nothing once warm
    std::vector<uint8_t> u8_, in_, has_, desc_;
    std::vector<float> f0_, f1_, f2_, f3_, f4_, f5_, f6_, g0_, g1_, g2_, g3_;
    std::vector<uint8_t> v8_, w8_, desc2_;
    std::vector<int32_t> i0_, i1_, i2_, j0_, j1_, j2_, obs_, match_;
    std::vector<orbx_keypoint> kp_, kp2_;
};
struct PooledHandle {
    orbm_matcher *m = nullptr; Scratch *s = nullptr;
    unsigned long gridFrame = ~0ul; const void *gridKeys = nullptr; int gridN = -1; int gridKind = -1;   // which frame's (0) / key frame's (1) grid the handle holds
};
struct HandlePool {                              // one per thread: handles are not re-entrant, threads never share one
    std::vector<PooledHandle> idle;
    ~HandlePool() { for (auto &h : idle) { orbm_destroy(h.m); delete h.s; } }
    static HandlePool &tls() { static thread_local HandlePool p; return p; }
};
inline int &pool_device() { static int d = 0; return d; }
inline int &pool_max_descriptors() { static int n = 8192; return n; }
inline int &pool_max_pairs() { static int n = 1 << 22; return n; }

// a handle for the length of one call, for adapter code outside ORB_SLAM2::ORBmatcher (which leases in its constructor)
struct Lease {
    PooledHandle h;
    Lease() { auto &pool = HandlePool::tls(); if (!pool.idle.empty()) { h = pool.idle.back(); pool.idle.pop_back(); } }
    ~Lease() { if (h.m) HandlePool::tls().idle.push_back(h); }
    Lease(const Lease &) = delete;
    Lease &operator=(const Lease &) = delete;
    bool ready(std::string *err)
    {
        if (h.m) return true;
        if (orbm_create(&h.m, pool_device(), pool_max_descriptors(), pool_max_descriptors(), pool_max_pairs()) != ORBX_OK) {
            if (err) *err = orbm_last_error();
            h.m = nullptr;
            return false;
        }
        h.s = new Scratch();
        return true;
    }
};
}  // namespace orbm_detail
}  // namespace ORB_SLAM2
