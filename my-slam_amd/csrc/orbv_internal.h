// orbv_internal.h -- the vocabulary handle, shared by orbv.hip (loader, kernel, C ABI) and orbv_workspace.cc (host-only: growth)
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/orbv.h"
#include "dev_buf.h"

int vfail(int code, const char *fmt, ...);
#define VHIP(expr)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return vfail(ORBX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define VTRY(expr)                            \
    do {                                      \
        int vtry_ = (expr);                   \
        if (vtry_ != ORBX_OK) return vtry_;   \
    } while (0)

struct orbv_vocabulary {
    int k = 0, L = 0, scoring = 0, weighting = 0, device = 0;
    std::vector<int32_t> parent, child_off, child_ids, word_of;   // per node (child lists in push order)
    std::vector<uint8_t> desc;                                   // nnodes x 32
    std::vector<double> weight;
    int nwords = 0;
    // device copies
    DevBuf<int32_t> d_child_off, d_child_ids, d_word_of;
    DevBuf<uint8_t> d_desc;
    DevBuf<double> d_weight;
    // staging, all three sized for cap_feat() features
    DevBuf<uint8_t> d_feat;
    DevBuf<int32_t> d_out_i;       // [cap] word | [cap] node | [cap] weight (double): one block, one copy back
    PinBuf<uint8_t> h_pin;         // pinned: [cap * 32] features in, [cap * 16] results out
    hipStream_t stream = nullptr;
    size_t cap_feat() const { return std::min(std::min(d_feat.bytes() / 32, d_out_i.bytes() / 16), h_pin.bytes() / 48); }
};
int orbv_ensure_feat(orbv_vocabulary *v, size_t n);     // staging for n features; synchronises the handle's stream before it grows
