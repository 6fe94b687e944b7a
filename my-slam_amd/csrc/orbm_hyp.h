// orbm_hyp.h -- the frame the hypothesis kernels share (k_sim3_hypotheses, k_pnp_hypotheses, k_init_hypotheses) and the argument
// checks of the batched solver calls (those three, orbm_init_check_rt, orbm_pose_optimization_batch, orbm_optimize_sim3_batch).
//
// The frame: B problems in CSR form.  Problem p owns the correspondences off[p] .. off[p + 1] (n of them) and the hypotheses
// hyp_off[p] .. hyp_off[p + 1]; hypothesis h of problem p owns the W = ceil(n / 32) mask words from
// mask_off[p] + (h - hyp_off[p]) * W, bit i of the row = correspondence i is an inlier.  One wave per hypothesis by flat index h,
// M_THREADS / 64 waves to a workgroup; a wave finds its problem with a binary search over hyp_off, so the waves of a workgroup read
// the arrays of one problem except at a problem's end.  The lanes stride over the correspondences 64 at a time; a ballot is 64 bits
// of the mask row and its popcount adds to the count.  A kernel keeps what is its own: the n <= 0 zero-fill of its output width,
// the gather, the solve and the output stores.
#pragma once
#include <cstdint>
#include "orbm_internal.h"

#ifdef __HIPCC__
struct HypFrame {
    int h, p, n, W;             // flat hypothesis index, its problem, the problem's correspondences and mask words per hypothesis
    long long c0;               // the problem's first correspondence
    uint32_t *mk;               // the hypothesis's mask row
};

// A kernel opens with
//     const long long hl = hyp_wave_index(WAVES);             // WAVES = its waves to a workgroup
//     if (hl >= hyp_off[n_problems]) return;                  // whole waves leave
//     const HypFrame f = hyp_frame(n_problems, off, hyp_off, mask_off, masks, hl);
// The early return stays in the kernel: inside the helper (a flag in the frame, or a bool beside it) the same code compiles to
// another register allocation and schedule.
__device__ __forceinline__ long long hyp_wave_index(int waves) { return (long long)blockIdx.x * waves + (threadIdx.x >> 6); }

__device__ __forceinline__ HypFrame hyp_frame(int n_problems, const int32_t *off, const int32_t *hyp_off, const int64_t *mask_off,
                                              uint32_t *masks, long long hl)
{
    const int h = __builtin_amdgcn_readfirstlane((int)hl);      // uniform: the search and the frame stay in scalar registers
    int lo = 0, hi = n_problems - 1;            // the last p with hyp_off[p] <= h (problems without hypotheses are stepped over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hyp_off[mid] <= h) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
    const long long c0 = off[p];
    const int n = off[p + 1] - off[p];
    const int W = (n + 31) >> 5;
    return {h, p, n, W, c0, masks + mask_off[p] + (long long)(h - hyp_off[p]) * W};
}

// The 64 correspondences from `base` on: lane 0 writes their one or two mask words (the second only inside the row), every lane
// gets the number of inliers among them.  inl is an int as __ballot takes one (a bool parameter costs a conversion that moves
// k_init_hypotheses to another register allocation).
__device__ __forceinline__ int hyp_vote(const HypFrame &f, int inl, int base, int lane)
{
    const unsigned long long b = __ballot(inl);
    const int count = __popcll(b);
    if (lane == 0) {
        f.mk[base >> 5] = (uint32_t)b;
        if ((base >> 5) + 1 < f.W) f.mk[(base >> 5) + 1] = (uint32_t)(b >> 32);
    }
    return count;
}
#endif

// -------------------------------------------------------------------------------------------------
// argument checks.  An entry point runs them in this order: problem count; n_problems == 0 is OK; NULL of the offset arrays and
// the per-problem struct; the CSR check (entry [0], monotone offsets, the mask_off recurrence; no hypothesis is OK; capacity); NULL
// of the rest; the per-problem content; the handle.
// -------------------------------------------------------------------------------------------------
template <class... P> static inline bool any_null(const P *...p) { return (... || !p); }
template <class... P> static inline bool misaligned(uintptr_t mask, const P *...p) { return ((... | (uintptr_t)p) & mask) != 0; }

static inline int check_problem_count(int n_problems)
{
    if (n_problems < 0) return mfail(ORBX_E_INVALID, "n_problems=%d", n_problems);
    if (n_problems > (1 << 24)) return mfail(ORBX_E_CAPACITY, "request beyond 2^24 problems");
    return ORBX_OK;
}

// off alone (orbm_pose_optimization_batch, orbm_optimize_sim3_batch): yields total = off[n_problems], at most 2^28 `noun`
static inline int check_off_csr(int n_problems, const int32_t *off, const char *noun, int &total)
{
    if (off[0] != 0) return mfail(ORBX_E_INVALID, "off[0] must be 0");
    for (int p = 0; p < n_problems; p++)
        if (off[p + 1] < off[p]) return mfail(ORBX_E_INVALID, "off not monotone at %d", p);
    total = off[n_problems];
    if (total > (1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 %s", noun);
    return ORBX_OK;
}

// the three arrays of a hypothesis call: yields the totals, at most 2^total_log2 `noun` / 2^hyp_log2 hypotheses / 2^29 mask words.
// H == 0 comes back as OK before the capacity is looked at: the caller returns OK then.
static inline int check_hyp_csr(int n_problems, const int32_t *off, const int32_t *hyp_off, const int64_t *mask_off, int total_log2,
                                const char *noun, int hyp_log2, int &total, int &H, int64_t &MW)
{
    if (off[0] != 0 || hyp_off[0] != 0 || mask_off[0] != 0) return mfail(ORBX_E_INVALID, "off[0], hyp_off[0] and mask_off[0] must be 0");
    for (int p = 0; p < n_problems; p++) {
        if (off[p + 1] < off[p]) return mfail(ORBX_E_INVALID, "off not monotone at %d", p);
        if (hyp_off[p + 1] < hyp_off[p]) return mfail(ORBX_E_INVALID, "hyp_off not monotone at %d", p);
        const int64_t W = ((int64_t)off[p + 1] - off[p] + 31) / 32;
        if (mask_off[p + 1] != mask_off[p] + W * ((int64_t)hyp_off[p + 1] - hyp_off[p]))
            return mfail(ORBX_E_INVALID, "mask_off[%d] is not mask_off[%d] + hypotheses * ceil(n / 32)", p + 1, p);
    }
    total = off[n_problems]; H = hyp_off[n_problems]; MW = mask_off[n_problems];
    if (H == 0) return ORBX_OK;
    if (total > (1 << total_log2) || H > (1 << hyp_log2) || MW > (1ll << 29))
        return mfail(ORBX_E_CAPACITY, "request beyond 2^%d %s / 2^%d hypotheses / 2^29 mask words", total_log2, noun, hyp_log2);
    return ORBX_OK;
}
