// orbk_internal.h -- the keyframe database handle, shared by orbk.hip (kernels, C ABI) and orbk_workspace.cc (host-only: growth)
#pragma once
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/orbk.h"
#include "dev_buf.h"

int kfail(int code, const char *fmt, ...);
#define KHIP(expr)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return kfail(ORBX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define KTRY(expr)                            \
    do {                                      \
        int ktry_ = (expr);                   \
        if (ktry_ != ORBX_OK) return ktry_;   \
    } while (0)

struct KSlotDev { long long off; int32_t len; int32_t pad; };   // len 0: erased (or an empty BowVector)

struct KState {                   // KeyFrame::mnLoopQuery .. mRelocScore; scores read 0.0f before their first write (orbk.h)
    uint64_t loop_q = 0, reloc_q = 0;
    int loop_w = 0, reloc_w = 0;
    float loop_s = 0.0f, reloc_s = 0.0f;
};
struct KSlot { uint64_t id; long long off; int len; bool live; KState *st; };
struct KPending {
    bool active = false;
    uint64_t qid = 0;
    int min_common = 0;
    float min_score = 0.0f;
    std::vector<uint64_t> ids;
    std::vector<float> si;
};

struct orbk_database {
    int device = 0, nwords = 0;
    mutable std::mutex mu;
    std::unordered_map<uint64_t, KState> state;        // by id: outlives membership (erase, clear, re-add)
    std::unordered_map<uint64_t, int> slot_of;         // live ids
    std::vector<KSlot> slots;                          // add order; erased slots stay until the next compaction
    long long tail = 0, live_entries = 0;
    int nlive = 0;
    KPending pending[2];
    // device arena
    DevBuf<int32_t> d_ids; DevBuf<double> d_vals; DevBuf<KSlotDev> d_slots;
    long long cap_entries() const { return (long long)std::min(d_ids.count(), d_vals.count()); }
    int cap_slots() const { return (int)d_slots.count(); }
    // per-query I/O: [query ids | query vals | counter | records], one copy in and one copy out
    DevBuf<uint8_t> d_io; PinBuf<uint8_t> h_io;
    size_t cap_io() const { return std::min(d_io.bytes(), h_io.bytes()); }
    int rec_hint = 0;                                  // records copied back with the counter (grows with the last count)
    hipStream_t stream = nullptr;
};

static inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
int orbk_ensure_io(orbk_database *db, size_t bytes);
int orbk_make_room(orbk_database *db, int n);
// orbk.hip: queues k_kfdb_compact (one wave per plan entry: source offset, destination offset, length) on s
hipError_t orbk_launch_compact(const int32_t *src_ids, const double *src_vals, int32_t *dst_ids, double *dst_vals,
                               const long long *d_plan, int nplan, hipStream_t s);
