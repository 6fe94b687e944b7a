// orbp_ba.cc -- Optimizer::BundleAdjustment (src/Optimizer.cc:49-237 of WChen09/My-SLAM, on g2o) over the flat problem of
// include/orbp.h: orbp_bundle_adjustment.  One optimize(n_iterations) of the graph LocalBundleAdjustment also builds: the edges,
// Huber and the Schur terms are csrc/orbp_lba_body.h, the Levenberg loop csrc/orbp_lm_body.h, the sums in edge order and the dense
// Cholesky csrc/orbp_lba_host.h.  This file owns the call's semantics: no entry check of `stop`, the robust switch, the one round.
#include <cstdio>
#include <cstring>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_internal.h"
#include "orbp_lba_body.h"
#include "orbp_lba_host.h"

static_assert(ORBP_BA_MAX_ITERATIONS == LM_MAX_ITERATIONS, "lm_optimize's loop bound is the bound of n_iterations");

int orbp_ba_check(const orbp_lba_problem *p, int n_iterations, const float *Tcw_local, const float *xw, char *text, int text_size)
{
    // there is no erase output: the check only asks that it is not NULL where there are edges
    static const unsigned char no_erase = 0;
    if (orbp_lba_check(p, Tcw_local, xw, &no_erase, text, text_size) != ORBX_OK) {
        if (!strncmp(text, "local_", 6)) memmove(text, text + 6, strlen(text + 6) + 1);     // "bundle_adjustment: ..."
        return ORBX_E_INVALID;
    }
    if (n_iterations < 0 || n_iterations > ORBP_BA_MAX_ITERATIONS) {
        snprintf(text, (size_t)text_size, "bundle_adjustment: n_iterations %d outside [0, %d]", n_iterations, ORBP_BA_MAX_ITERATIONS);
        return ORBX_E_INVALID;
    }
    return ORBX_OK;
}

extern "C" int orbp_bundle_adjustment(const orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local, float *xw,
                                      const volatile uint8_t *stop, orbp_ba_stats *stats)
{
    char text[200];
    if (orbp_ba_check(p, n_iterations, Tcw_local, xw, text, (int)sizeof text) != ORBX_OK) {
        orbp_set_error(text);
        return ORBX_E_INVALID;
    }
    LbaHost h;
    h.prepare(p, xw, stop);
    h.robust = robust ? LBA_KERNEL_BA : LBA_KERNEL_NONE;        // :129-134, :158-163
    LmRun run = {0, 0, 0, 0};
    h.activate();                                               // :187
    if (h.n_active > 0) lm_optimize(h, n_iterations, run);      // :188
    for (int k = 0; k < h.K; k++) se3_to_Tcw(h.est[k], Tcw_local + 16 * (size_t)k);    // :193-210
    for (int pt = 0; pt < h.P; pt++)                            // :213-235; a point without edges is vbNotIncludedMP
        if (p->edge_off[pt + 1] > p->edge_off[pt])
            for (int j = 0; j < 3; j++) xw[3 * (size_t)pt + j] = (float)h.xw[3 * (size_t)pt + j];
    if (stats) *stats = {run.iterations, run.trials, run.lambda, run.chi2};
    return 0;
}
