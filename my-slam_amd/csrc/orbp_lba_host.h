// orbp_lba_host.h -- "the passes of a problem" for lm_optimize (orbp_lm_body.h) on the host, shared by orbp_lba.cc
// (Optimizer::LocalBundleAdjustment) and orbp_ba.cc (Optimizer::BundleAdjustment): the sums in edge order, as g2o's active edges
// are sorted by id, and the dense Cholesky of the reduced system.  prepare() sets the graph up from the flat problem.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../include/orbp.h"
#include "orbp_internal.h"
#include "orbp_lba_body.h"

namespace {
// upper-triangle positions of the diagonal entries
const int DIAG6[6] = {0, 6, 11, 15, 18, 20};
const int DIAG3[3] = {0, 3, 5};

struct LbaHost {
    const orbp_lba_problem *p;
    const volatile uint8_t *stop_flag;
    int K, NK, P, E;                        // local key frames, all key frames, points, edges
    std::vector<LbaSe3> est, est_backup;
    std::vector<LbaCam> cam;
    std::vector<uint8_t> kf_free, kf_active, pt_active, level;
    std::vector<int32_t> edge_pt;
    std::vector<double> xw, xw_backup, err, blk, Hpp, bp, Hll, bl, Dinv, Db, S, bs, xp, xl, Y;
    int robust = LBA_KERNEL_LBA;            // LBA_KERNEL_*
    int n_active = 0;

    // the graph of the flat problem: estimates as Converter::toSE3Quat / toVector3d give them, every edge at level 0
    void prepare(const orbp_lba_problem *pr, const float *xw_in, const volatile uint8_t *stop_)
    {
        p = pr; stop_flag = stop_;
        K = p->n_local; NK = p->n_local + p->n_fixed; P = p->n_points; E = p->edge_off[p->n_points];
        est.resize(NK); cam.resize(NK); kf_free.assign(NK, 0); kf_active.assign(NK, 0);
        for (int k = 0; k < NK; k++) {
            est[k] = se3_from_Tcw(p->Tcw + 16 * (size_t)k);
            const float *c = p->cam + 5 * (size_t)k;
            cam[k] = {c[0], c[1], c[2], c[3], c[4]};
            kf_free[k] = k < K && !p->local_fixed[k];
        }
        xw.resize(3 * (size_t)P);
        for (size_t i = 0; i < xw.size(); i++) xw[i] = xw_in[i];    // Converter::toVector3d
        pt_active.assign(P, 0); level.assign(E, 0); edge_pt.resize(E);
        int max_deg = 0;
        for (int pt = 0; pt < P; pt++) {
            for (int e = p->edge_off[pt]; e < p->edge_off[pt + 1]; e++) edge_pt[e] = pt;
            max_deg = std::max(max_deg, p->edge_off[pt + 1] - p->edge_off[pt]);
        }
        err.assign(3 * (size_t)E, 0.); blk.assign(LBA_NBLK * (size_t)E, 0.);
        Hpp.resize(21 * (size_t)K); bp.resize(6 * (size_t)K); Hll.resize(6 * (size_t)P); bl.resize(3 * (size_t)P);
        Dinv.resize(9 * (size_t)P); Db.resize(3 * (size_t)P); S.resize(36 * (size_t)K * K); bs.resize(6 * (size_t)K);
        xp.assign(6 * (size_t)K, 0.); xl.assign(3 * (size_t)P, 0.); Y.resize(18 * (size_t)max_deg);
    }
    bool stop() const { return orbp_lba_read_stop(stop_flag); }
    bool stereo(int e) const { return !(p->u_right[e] < 0); }
    void activate()                         // initializeOptimization(0): the level-0 edges and the vertices that have one
    {
        std::fill(kf_active.begin(), kf_active.end(), 0);
        std::fill(pt_active.begin(), pt_active.end(), 0);
        n_active = 0;
        for (int e = 0; e < E; e++)
            if (!level[e]) {
                n_active++;
                pt_active[edge_pt[e]] = 1;
                if (kf_free[p->edge_kf[e]]) kf_active[p->edge_kf[e]] = 1;
            }
    }
    double errors()                         // computeActiveErrors + activeRobustChi2, in edge order
    {
        double chi = 0, pc[3];
        for (int e = 0; e < E; e++)
            if (!level[e]) {
                const int k = p->edge_kf[e];
                lba_edge_error(est[k], cam[k], &xw[3 * (size_t)edge_pt[e]], p->obs + 2 * (size_t)e, p->u_right[e], pc, &err[3 * (size_t)e]);
                chi += lba_edge_robust_chi2(&err[3 * (size_t)e], (double)p->inv_sigma2[e], stereo(e), robust);
            }
        return chi;
    }
    void linearize(bool first, bool with_errors, double &chi, double &maxdiag)
    {
        if (with_errors) chi = errors();
        std::fill(Hpp.begin(), Hpp.end(), 0.); std::fill(bp.begin(), bp.end(), 0.);
        std::fill(Hll.begin(), Hll.end(), 0.); std::fill(bl.begin(), bl.end(), 0.);
        for (int e = 0; e < E; e++) {
            if (level[e]) continue;
            const int k = p->edge_kf[e], pt = edge_pt[e];
            double *b = &blk[LBA_NBLK * (size_t)e];
            lba_edge_blocks(est[k], cam[k], &xw[3 * (size_t)pt], &err[3 * (size_t)e], (double)p->inv_sigma2[e], stereo(e), robust,
                            kf_free[k] != 0, b);
            for (int i = 0; i < 6; i++) Hll[6 * (size_t)pt + i] += b[LBA_HLL + i];
            for (int i = 0; i < 3; i++) bl[3 * (size_t)pt + i] += b[LBA_BL + i];
            if (kf_free[k]) {
                for (int i = 0; i < 21; i++) Hpp[21 * (size_t)k + i] += b[LBA_HPP + i];
                for (int i = 0; i < 6; i++) bp[6 * (size_t)k + i] += b[LBA_BP + i];
            }
        }
        if (!first) return;
        maxdiag = 0;                        // computeLambdaInit: the poses, then the points
        for (int k = 0; k < K; k++)
            if (kf_active[k])
                for (int j = 0; j < 6; j++) maxdiag = std::fmax(std::fabs(Hpp[21 * (size_t)k + DIAG6[j]]), maxdiag);
        for (int pt = 0; pt < P; pt++)
            if (pt_active[pt])
                for (int j = 0; j < 3; j++) maxdiag = std::fmax(std::fabs(Hll[6 * (size_t)pt + DIAG3[j]]), maxdiag);
    }
    // S = U^T U on the upper triangle of the n x n row-major S, then U^T y = b, U x = y.  False where a pivot is not positive or
    // not finite (the reference: Eigen's sparse LDL^T inside g2o::LinearSolverEigen reporting NumericalIssue)
    static bool cholesky_solve(double *A, int n, const double *b, double *x)
    {
        for (int j = 0; j < n; j++) {
            double d = A[(size_t)j * n + j];
            for (int k = 0; k < j; k++) d -= A[(size_t)k * n + j] * A[(size_t)k * n + j];
            if (!(d > 0) || !std::isfinite(d)) return false;
            d = std::sqrt(d);
            A[(size_t)j * n + j] = d;
            for (int i = j + 1; i < n; i++) {
                double s = A[(size_t)j * n + i];
                for (int k = 0; k < j; k++) s -= A[(size_t)k * n + j] * A[(size_t)k * n + i];
                A[(size_t)j * n + i] = s / d;
            }
        }
        for (int i = 0; i < n; i++) {
            double s = b[i];
            for (int k = 0; k < i; k++) s -= A[(size_t)k * n + i] * x[k];
            x[i] = s / A[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; i--) {
            double s = x[i];
            for (int k = i + 1; k < n; k++) s -= A[(size_t)i * n + k] * x[k];
            x[i] = s / A[(size_t)i * n + i];
        }
        return true;
    }
    void trial(double lambda, double &chi, double &scale, bool &ok)
    {
        est_backup = est; xw_backup = xw;   // push
        const int n = 6 * K;
        // setLambda, then _Hschur = _Hpp and _bschur = _b (block_solver.hpp:373-374, :436)
        std::fill(S.begin(), S.end(), 0.);
        for (int k = 0; k < K; k++) {
            if (!kf_active[k]) {
                for (int a = 0; a < 6; a++) { S[(size_t)(6 * k + a) * n + 6 * k + a] = 1.; bs[6 * k + a] = 0; }
                continue;
            }
            int u = 0;
            for (int a = 0; a < 6; a++)
                for (int b = a; b < 6; b++, u++) S[(size_t)(6 * k + a) * n + 6 * k + b] = Hpp[21 * (size_t)k + u] + (a == b ? lambda : 0.);
            for (int a = 0; a < 6; a++) bs[6 * k + a] = bp[6 * (size_t)k + a];
        }
        for (int pt = 0; pt < P; pt++) {    // :381-432, landmark by landmark
            if (!pt_active[pt]) continue;
            double *D = &Dinv[9 * (size_t)pt], *db = &Db[3 * (size_t)pt];
            lba_point_dinv(&Hll[6 * (size_t)pt], &bl[3 * (size_t)pt], lambda, D, db);
            const int e0 = p->edge_off[pt], e1 = p->edge_off[pt + 1];
            for (int e = e0; e < e1; e++)
                if (!level[e] && kf_free[p->edge_kf[e]]) lba_mul_WD(&blk[LBA_NBLK * (size_t)e + LBA_HPL], D, &Y[18 * (size_t)(e - e0)]);
            for (int a = e0; a < e1; a++) {
                const int i = p->edge_kf[a];
                if (level[a] || !kf_free[i]) continue;
                double v[6], M[36];
                lba_mul_Wd(&blk[LBA_NBLK * (size_t)a + LBA_HPL], db, v);
                for (int r = 0; r < 6; r++) bs[6 * i + r] -= v[r];
                for (int b = a; b < e1; b++) {
                    const int j = p->edge_kf[b];
                    if (level[b] || !kf_free[j]) continue;
                    const int lo = i <= j ? a : b, hi = i <= j ? b : a, r0 = 6 * p->edge_kf[lo], c0 = 6 * p->edge_kf[hi];
                    lba_mul_YWt(&Y[18 * (size_t)(lo - e0)], &blk[LBA_NBLK * (size_t)hi + LBA_HPL], M);
                    for (int r = 0; r < 6; r++)
                        for (int c = (lo == hi ? r : 0); c < 6; c++) S[(size_t)(r0 + r) * n + c0 + c] -= M[6 * r + c];
                }
            }
        }
        ok = n == 0 || cholesky_solve(S.data(), n, bs.data(), xp.data());
        scale = 0;
        if (ok) {
            for (int pt = 0; pt < P; pt++) {    // :461-481
                double *x = &xl[3 * (size_t)pt];
                x[0] = x[1] = x[2] = 0;
                if (!pt_active[pt]) continue;
                double cl[3] = {bl[3 * (size_t)pt], bl[3 * (size_t)pt + 1], bl[3 * (size_t)pt + 2]};
                for (int e = p->edge_off[pt]; e < p->edge_off[pt + 1]; e++)
                    if (!level[e] && kf_free[p->edge_kf[e]]) lba_sub_Wtx(&blk[LBA_NBLK * (size_t)e + LBA_HPL], &xp[6 * (size_t)p->edge_kf[e]], cl);
                const double *D = &Dinv[9 * (size_t)pt];
                for (int i = 0; i < 3; i++) x[i] = D[3 * i] * cl[0] + D[3 * i + 1] * cl[1] + D[3 * i + 2] * cl[2];
            }
            for (int k = 0; k < K; k++)         // computeScale: the poses, then the points
                if (kf_active[k])
                    for (int j = 0; j < 6; j++) scale += lm_scale_term(xp[6 * (size_t)k + j], bp[6 * (size_t)k + j], lambda);
            for (int pt = 0; pt < P; pt++)
                if (pt_active[pt])
                    for (int j = 0; j < 3; j++) scale += lm_scale_term(xl[3 * (size_t)pt + j], bl[3 * (size_t)pt + j], lambda);
            for (int k = 0; k < K; k++)         // update
                if (kf_active[k]) est[k] = lba_pose_oplus(est[k], &xp[6 * (size_t)k]);
            for (int pt = 0; pt < P; pt++)
                if (pt_active[pt])
                    for (int j = 0; j < 3; j++) xw[3 * (size_t)pt + j] += xl[3 * (size_t)pt + j];
        }
        chi = errors();
    }
    void accept() {}
    void reject() { est = est_backup; xw = xw_backup; }
    bool flagged(int e) const               // e->chi2() > 5.991 / 7.815 || !e->isDepthPositive() (:680, :696, :723, :738)
    {
        return lba_chi2(&err[3 * (size_t)e], (double)p->inv_sigma2[e]) > lba_chi2_threshold(stereo(e)) ||
               !lba_depth_positive(est[p->edge_kf[e]], &xw[3 * (size_t)edge_pt[e]]);
    }
};
}   // namespace
