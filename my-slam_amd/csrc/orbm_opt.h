// orbm_opt.h -- what the optimizer drivers (orbm_lba.hip, orbm_eg.hip) share on the device side: the fixed reduction trees, the
// event profile behind the *_split calls and the frame of the passes lm_optimize (orbp_lm_body.h) drives
#pragma once
#include "orbm_internal.h"

// inside a wave: the butterfly over the lane bits 0, 1, ..., 5 of DESIGN.md section 21; all 64 lanes end with the same bits
__device__ __forceinline__ double opt_wave_sum(double a)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
    return a;
}
// One workgroup of RT threads, all of it: the butterfly, the RT / 64 wave totals into sh, then pairwise (at 1024: 8, 4, 2, 1)
template <int RT> __device__ __forceinline__ double opt_block_sum(double a, double *sh)
{
    a = opt_wave_sum(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    for (int s = RT / 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}
// The maximum: the same butterfly and wave results, then thread 0 alone walks them; the value is the workgroup's in thread 0 only
template <int RT> __device__ __forceinline__ double opt_block_max(double a, double *sh)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a = fmax(a, __shfl_xor(a, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < RT / 64; w++) a = fmax(a, sh[w]);
    return a;
}
inline unsigned opt_blocks(long long n, int per) { return (unsigned)std::max<long long>((n + per - 1) / per, 1); }   // at least one

// The event profile behind the *_split variants of the optimiser calls: events on the call's stream between the groups of launches.
// An event follows each group, so a group's time runs from the end of the group before it (or from the event that opens a batch,
// recorded when the host comes back from a synchronisation) to its own end: the idle time until the host has enqueued it counts
// into it.  Elapsed times are read after the synchronisation that was due anyway; nothing else about the call changes.
struct SplitProf {
    enum { NEV = 32 };
    bool on = false;
    hipEvent_t ev[NEV];
    int grp[NEV], n = 0, made = 0;
    double *ms = nullptr;
    int32_t *count = nullptr;
    void start(double *ms_, int32_t *count_, int ngroups)
    {
        ms = ms_; count = count_;
        for (int g = 0; g < ngroups; g++) { ms[g] = 0; count[g] = 0; }
        for (made = 0; made < NEV; made++)
            if (hipEventCreate(&ev[made]) != hipSuccess) return;
        on = true;
    }
    ~SplitProf() { for (int i = 0; i < made; i++) (void)hipEventDestroy(ev[i]); }
    // before a group (opens a batch if none is open) and after a group's launches
    void pre(hipStream_t s) { if (on && n == 0 && hipEventRecord(ev[0], s) == hipSuccess) { grp[0] = -1; n = 1; } }
    void post(int g, hipStream_t s) { if (on && n > 0 && n < NEV && hipEventRecord(ev[n], s) == hipSuccess) grp[n++] = g; }
    void drain()                            // after a synchronisation of the stream
    {
        for (int i = 1; i < n; i++) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) { ms[grp[i]] += (double)t; count[grp[i]]++; }
        }
        n = 0;
    }
};
#define SPLIT_GROUP(prof, g, s, ...) do { (prof).pre(s); __VA_ARGS__; (prof).post(g, s); } while (0)

// "The passes of a problem" for lm_optimize as kernel launches on the handle's stream: the part that does not depend on the
// problem.  Local to the file that includes it, as the drivers' own contexts are: the library exports nothing of it.
namespace {
struct OptGpu {
    orbm_matcher *m = nullptr;
    hipStream_t s = nullptr;
    double *pin = nullptr, *out = nullptr;  // the one small block a trial hands back: 64 bytes, page-locked and on the device
    int cur = 0, status = ORBX_OK;          // [cur]: the estimates, [1 - cur] a trial's; a failed launch or copy ends the loop
    SplitProf prof;                         // through the driver's stop() and comes back as the call's status
    int read_back(int group)                // after the driver's reduce launch: copy, synchronise
    {
        MHIPCHK(hipGetLastError());
        MHIPCHK(hipMemcpyAsync(pin, out, 64, hipMemcpyDeviceToHost, s));
        prof.post(group, s);
        MHIPCHK(hipStreamSynchronize(s));
        prof.drain();
        return ORBX_OK;
    }
    // the end of a call: the results, back to back at dev, home in one copy into the arena; the outputs are written at orbm_sync
    int download(std::initializer_list<void *> host, std::initializer_list<size_t> parts, const void *dev, int group)
    {
        MTRY(orbm_d2h_split(m, host.begin(), parts.begin(), (int)host.size(), dev, s));
        prof.post(group, s);
        MTRY(orbm_sync(m, s));
        prof.drain();
        return ORBX_OK;
    }
    void accept() { cur ^= 1; }
    void reject() {}
};
}   // namespace
