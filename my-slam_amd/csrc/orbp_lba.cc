// orbp_lba.cc -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778 of WChen09/My-SLAM, on g2o) over the flat problem of
// include/orbp.h: orbp_local_bundle_adjustment.  The arithmetic of an edge, of a point's 3x3 block and the Schur terms
// (csrc/orbp_lba_body.h) and the Levenberg loop (csrc/orbp_lm_body.h) are the text orbm_lba.hip runs as well; csrc/orbp_lba_host.h
// owns the order of the sums (edge order, as g2o's active edges are sorted by id) and the dense Cholesky of the reduced system,
// for this file and orbp_ba.cc; this file owns the two rounds, the two flagging passes and the argument checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_internal.h"
#include "orbp_lba_body.h"
#include "orbp_lba_host.h"

int orbp_lba_check(const orbp_lba_problem *p, const float *Tcw_local, const float *xw, const unsigned char *erase, char *text, int text_size)
{
#define LBA_BAD(...) do { snprintf(text, (size_t)text_size, __VA_ARGS__); return ORBX_E_INVALID; } while (0)
    if (!p) LBA_BAD("local_bundle_adjustment: NULL problem");
    if (p->n_local < 0 || p->n_fixed < 0 || p->n_points < 0)
        LBA_BAD("local_bundle_adjustment: negative count (n_local=%d n_fixed=%d n_points=%d)", p->n_local, p->n_fixed, p->n_points);
    const long long nkf = (long long)p->n_local + p->n_fixed;
    if (nkf > (1 << 24) || p->n_points > (1 << 26)) LBA_BAD("local_bundle_adjustment: beyond 2^24 key frames / 2^26 points");
    if (!p->edge_off) LBA_BAD("local_bundle_adjustment: NULL edge_off");
    if (p->n_local > 0 && (!p->local_fixed || !Tcw_local)) LBA_BAD("local_bundle_adjustment: NULL local_fixed or Tcw_local");
    if (nkf > 0 && (!p->Tcw || !p->cam)) LBA_BAD("local_bundle_adjustment: NULL Tcw or cam");
    if (p->n_points > 0 && !xw) LBA_BAD("local_bundle_adjustment: NULL xw");
    if (p->edge_off[0] != 0) LBA_BAD("local_bundle_adjustment: edge_off[0] must be 0");
    for (int i = 0; i < p->n_points; i++)
        if (p->edge_off[i + 1] < p->edge_off[i]) LBA_BAD("local_bundle_adjustment: edge_off not monotone at %d", i);
    const int ne = p->edge_off[p->n_points];
    if (ne > (1 << 28)) LBA_BAD("local_bundle_adjustment: beyond 2^28 edges");
    if (ne > 0 && (!p->edge_kf || !p->obs || !p->u_right || !p->inv_sigma2 || !erase)) LBA_BAD("local_bundle_adjustment: NULL edge array");
    for (long long i = 0; i < 16 * nkf; i++)
        if (!std::isfinite(p->Tcw[i])) LBA_BAD("local_bundle_adjustment: pose of key frame %d is not finite", (int)(i / 16));
    for (long long i = 0; i < 5 * nkf; i++)
        if (!std::isfinite(p->cam[i])) LBA_BAD("local_bundle_adjustment: calibration of key frame %d is not finite", (int)(i / 5));
    for (long long i = 0; i < 3ll * p->n_points; i++)
        if (!std::isfinite(xw[i])) LBA_BAD("local_bundle_adjustment: point %d is not finite", (int)(i / 3));
    std::vector<int32_t> seen((size_t)nkf, -1);
    for (int pt = 0; pt < p->n_points; pt++)
        for (int e = p->edge_off[pt]; e < p->edge_off[pt + 1]; e++) {
            const int k = p->edge_kf[e];
            if (k < 0 || k >= nkf) LBA_BAD("local_bundle_adjustment: edge %d: key frame %d outside [0, %lld)", e, k, nkf);
            if (seen[k] == pt) LBA_BAD("local_bundle_adjustment: edge %d: point %d holds key frame %d twice", e, pt, k);
            seen[k] = pt;
            if (!std::isfinite(p->obs[2 * (size_t)e]) || !std::isfinite(p->obs[2 * (size_t)e + 1]) || !std::isfinite(p->u_right[e]) ||
                !std::isfinite(p->inv_sigma2[e]))
                LBA_BAD("local_bundle_adjustment: observation of edge %d is not finite", e);
        }
#undef LBA_BAD
    return ORBX_OK;
}

// every read of `stop`, on both paths; the probe of tests/test_lba_stop.py (orbp_internal.h) runs just before it
static thread_local void (*lba_stop_probe)(void *) = nullptr;
static thread_local void *lba_stop_probe_arg = nullptr;
extern "C" void orbp_lba_set_stop_probe(void (*fn)(void *), void *arg) { lba_stop_probe = fn; lba_stop_probe_arg = arg; }
bool orbp_lba_read_stop(const volatile uint8_t *stop)
{
    if (lba_stop_probe) lba_stop_probe(lba_stop_probe_arg);
    return stop && *stop;
}


extern "C" int orbp_local_bundle_adjustment(const orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase,
                                            const volatile uint8_t *stop, orbp_lba_stats *stats)
{
    char text[200];
    if (orbp_lba_check(p, Tcw_local, xw, erase, text, (int)sizeof text) != ORBX_OK) {
        orbp_set_error(text);
        return ORBX_E_INVALID;
    }
    if (orbp_lba_read_stop(stop)) return ORBP_LBA_STOPPED;      // :655-657
    LbaHost h;
    h.prepare(p, xw, stop);

    orbp_lba_stats st;
    memset(&st, 0, sizeof st);
    LmRun run = {0, 0, 0, 0};
    h.robust = LBA_KERNEL_LBA;
    h.activate();                                               // :659
    if (h.n_active > 0) {
        lm_optimize(h, 5, run);                                 // :660
        st.iterations[0] = run.iterations; st.trials[0] = run.trials; st.lambda = run.lambda; st.chi2 = run.chi2;
    }
    if (!orbp_lba_read_stop(stop)) {                            // :662-709
        st.second_round = 1;
        for (int e = 0; e < h.E; e++)
            if (h.flagged(e)) { h.level[e] = 1; st.n_level1++; }
        h.robust = LBA_KERNEL_NONE;
        h.activate();                                           // :706
        if (h.n_active > 0) {
            lm_optimize(h, 10, run);                            // :707
            st.iterations[1] = run.iterations; st.trials[1] = run.trials; st.lambda = run.lambda; st.chi2 = run.chi2;
        }
    }
    for (int e = 0; e < h.E; e++) erase[e] = h.flagged(e) ? 1 : 0;      // :715-743
    for (int k = 0; k < h.K; k++) se3_to_Tcw(h.est[k], Tcw_local + 16 * (size_t)k);    // :762-768
    for (size_t i = 0; i < h.xw.size(); i++) xw[i] = (float)h.xw[i];                       // :771-777
    if (stats) *stats = st;
    return ORBP_LBA_DONE;
}
