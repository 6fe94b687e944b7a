// orbm_prof.h -- the event profile behind the *_split variants of the optimiser calls (orbm_lba.hip, orbm_eg.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Events on the call's stream between the groups of launches.  An event follows each group, so a group's time runs from the end of the group before it (or from the event that opens a batch, recorded when the host comes back
// from a synchronisation) to its own end: the idle time until the host has enqueued it counts into it.  Elapsed times are read
// after the synchronisation that was due anyway; nothing else about the call changes.
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
    void pre(hipStream_t s)                 // before a group: opens a batch if none is open
    {
        if (on && n == 0 && hipEventRecord(ev[0], s) == hipSuccess) { grp[0] = -1; n = 1; }
    }
    void post(int g, hipStream_t s)         // after a group's launches
    {
        if (on && n > 0 && n < NEV && hipEventRecord(ev[n], s) == hipSuccess) grp[n++] = g;
    }
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
