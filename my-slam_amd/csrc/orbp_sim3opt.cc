// orbp_sim3opt.cc -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241 of WChen09/My-SLAM, on g2o) for one 7-dof vertex over flat
// arrays: orbp_optimize_sim3 and orbp_sim3_from_rts (include/orbp.h).  Both point vertices of every correspondence are fixed
// (:1121, :1129), so the graph is one VertexSim3Expmap, one dense 7x7 system and a sum over the edges.  The arithmetic of a pair, the
// 7x7 solve and the Levenberg loop are csrc/orbp_sim3opt_body.h, the text the kernel of orbm_sim3opt.hip runs as well; this file owns
// the order of the sums (edge order, as g2o's active edges are sorted by id: e12 of pair 0, e21 of pair 0, e12 of pair 1, ...) and
// the two flagging passes.
#include <cmath>
#include <cstdio>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_internal.h"
#include "orbp_sim3opt_body.h"

namespace {
int s3o_fail(const char *text)
{
    orbp_set_error(text);
    return ORBX_E_INVALID;
}

struct Sim3OptProblem {
    int n;
    const float *x1c, *x2c, *obs1, *obs2, *inv_sigma2_1, *inv_sigma2_2;
    S3oCam cam1, cam2;
    double huber_delta;
    bool fix_scale;
    const uint8_t *removed;        // optimizer.removeEdge() (:1197-1198): not in the active set of the second optimize()

    void system(const S3oSim &T, double *sys) const
    {
        S3oSim e[S3O_NLIN], inv[S3O_NLIN];
        for (int k = 0; k < S3O_NLIN; k++) s3o_lin_entry(T, k, fix_scale, e[k], inv[k]);
        for (int v = 0; v < S3O_NSYS; v++) sys[v] = 0;
        double J[14];
        for (int i = 0; i < n; i++)
            if (!removed[i])
                s3o_pair<true>(e, inv, cam1, cam2, x1c + 3 * (size_t)i, x2c + 3 * (size_t)i, obs1 + 2 * (size_t)i, obs2 + 2 * (size_t)i,
                               inv_sigma2_1[i], inv_sigma2_2[i], huber_delta, sys, J, 1);
    }
    double chi2(const S3oSim &T) const
    {
        S3oSim e, inv;
        s3o_lin_entry(T, 0, fix_scale, e, inv);
        double sum[1] = {0};
        for (int i = 0; i < n; i++)
            if (!removed[i])
                s3o_pair<false>(&e, &inv, cam1, cam2, x1c + 3 * (size_t)i, x2c + 3 * (size_t)i, obs1 + 2 * (size_t)i, obs2 + 2 * (size_t)i,
                                inv_sigma2_1[i], inv_sigma2_2[i], huber_delta, sum, nullptr, 0);
        return sum[0];
    }
    bool bad(const S3oSim &T, const S3oSim &Tinv, int i, float th2) const
    {
        return s3o_pair_bad(T, Tinv, cam1, cam2, x1c + 3 * (size_t)i, x2c + 3 * (size_t)i, obs1 + 2 * (size_t)i, obs2 + 2 * (size_t)i,
                            inv_sigma2_1[i], inv_sigma2_2[i], th2);
    }
};
}   // namespace

extern "C" int orbp_sim3_from_rts(const float *R, const float *t, float s, double *out)
{
    if (!R || !t || !out) return s3o_fail("orbp_sim3_from_rts: NULL argument");
    double Rd[9];
    for (int i = 0; i < 9; i++) Rd[i] = R[i];          // Converter::toMatrix3d
    S3oSim S;
    quat_from_R(Rd, S);                            // Sim3(const Matrix3d &, ...) (sim3.h:64-67): Quaterniond(R), not normalised
    out[0] = S.qx; out[1] = S.qy; out[2] = S.qz; out[3] = S.qw;
    for (int i = 0; i < 3; i++) out[4 + i] = t[i];     // Converter::toVector3d
    out[7] = s;
    return 0;
}

extern "C" int orbp_optimize_sim3(int n, const float *x1c, const float *x2c, const float *obs1, const float *obs2,
                                  const float *inv_sigma2_1, const float *inv_sigma2_2, const float *K1, const float *K2, float th2,
                                  int fix_scale, double *S12, uint8_t *flags)
{
    if (n < 0 || !K1 || !K2 || !S12) return s3o_fail("orbp_optimize_sim3: n >= 0 and non-NULL K1, K2, S12");
    if (n > 0 && (!x1c || !x2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !flags))
        return s3o_fail("orbp_optimize_sim3: NULL correspondence array");
    for (int i = 0; i < 8; i++)
        if (!std::isfinite(S12[i])) return s3o_fail("orbp_optimize_sim3: S12 is not finite");
    Sim3OptProblem P;
    P.n = n;
    P.x1c = x1c; P.x2c = x2c; P.obs1 = obs1; P.obs2 = obs2; P.inv_sigma2_1 = inv_sigma2_1; P.inv_sigma2_2 = inv_sigma2_2;
    P.cam1 = {K1[0], K1[1], K1[2], K1[3]};
    P.cam2 = {K2[0], K2[1], K2[2], K2[3]};
    P.huber_delta = (float)std::sqrt(th2);             // const float deltaHuber = sqrt(th2) (:1095)
    P.fix_scale = fix_scale != 0;
    P.removed = flags;
    for (int i = 0; i < n; i++) flags[i] = 0;
    S3oSim est = {{S12[0], S12[1], S12[2], S12[3]}, S12[4], S12[5], S12[6], S12[7]};
    S3oSim err_est = est;
    // a problem without edges optimises nothing (sparse_optimizer.cpp: optimize() returns on an empty active set)
    if (n > 0) s3o_optimize(P, est, err_est, P.fix_scale, 5);                      // :1182
    int n_bad = 0;
    {
        // :1186-1203: every edge holds the error of the estimate the optimiser last evaluated, a rejected trial's included
        const S3oSim inv = s3o_inverse(err_est);
        for (int i = 0; i < n; i++) { flags[i] = P.bad(err_est, inv, i, th2); n_bad += flags[i]; }
    }
    const int more = n_bad > 0 ? 10 : 5;               // :1205-1209
    if (n - n_bad < 10) return 0;                      // :1211-1212: g2oS12 stays as it came
    s3o_optimize(P, est, err_est, P.fix_scale, more);  // :1216-1217, the removed pairs are out of the graph
    int n_in = 0;
    const S3oSim inv = s3o_inverse(err_est);
    for (int i = 0; i < n; i++) {
        if (flags[i]) continue;
        if (P.bad(err_est, inv, i, th2)) flags[i] = 1;
        else n_in++;
    }
    S12[0] = est.qx; S12[1] = est.qy; S12[2] = est.qz; S12[3] = est.qw;
    S12[4] = est.t0; S12[5] = est.t1; S12[6] = est.t2; S12[7] = est.s;
    return n_in;
}
