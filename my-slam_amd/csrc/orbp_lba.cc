// orbp_lba.cc -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778 of WChen09/My-SLAM, on g2o) over the flat problem of
// include/orbp.h: orbp_local_bundle_adjustment.  The arithmetic of an edge, of a point's 3x3 block, the Schur terms and the Levenberg
// loop are csrc/orbp_lba_body.h, the text the kernels of orbm_lba.hip run as well; this file owns the order of the sums (edge order,
// as g2o's active edges are sorted by id), the dense Cholesky of the reduced system, the two flagging passes and the argument checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_internal.h"
#include "orbp_lba_body.h"

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
    bool robust = true;
    int n_active = 0;

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
                    for (int j = 0; j < 6; j++) scale += lba_scale_term(xp[6 * (size_t)k + j], bp[6 * (size_t)k + j], lambda);
            for (int pt = 0; pt < P; pt++)
                if (pt_active[pt])
                    for (int j = 0; j < 3; j++) scale += lba_scale_term(xl[3 * (size_t)pt + j], bl[3 * (size_t)pt + j], lambda);
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
    h.p = p; h.stop_flag = stop;
    h.K = p->n_local; h.NK = p->n_local + p->n_fixed; h.P = p->n_points; h.E = p->edge_off[p->n_points];
    h.est.resize(h.NK); h.cam.resize(h.NK); h.kf_free.assign(h.NK, 0); h.kf_active.assign(h.NK, 0);
    for (int k = 0; k < h.NK; k++) {
        h.est[k] = lba_se3_from_Tcw(p->Tcw + 16 * (size_t)k);
        const float *c = p->cam + 5 * (size_t)k;
        h.cam[k] = {c[0], c[1], c[2], c[3], c[4]};
        h.kf_free[k] = k < h.K && !p->local_fixed[k];
    }
    h.xw.resize(3 * (size_t)h.P);
    for (size_t i = 0; i < h.xw.size(); i++) h.xw[i] = xw[i];   // Converter::toVector3d
    h.pt_active.assign(h.P, 0); h.level.assign(h.E, 0); h.edge_pt.resize(h.E);
    int max_deg = 0;
    for (int pt = 0; pt < h.P; pt++) {
        for (int e = p->edge_off[pt]; e < p->edge_off[pt + 1]; e++) h.edge_pt[e] = pt;
        max_deg = std::max(max_deg, p->edge_off[pt + 1] - p->edge_off[pt]);
    }
    h.err.assign(3 * (size_t)h.E, 0.); h.blk.assign(LBA_NBLK * (size_t)h.E, 0.);
    h.Hpp.resize(21 * (size_t)h.K); h.bp.resize(6 * (size_t)h.K); h.Hll.resize(6 * (size_t)h.P); h.bl.resize(3 * (size_t)h.P);
    h.Dinv.resize(9 * (size_t)h.P); h.Db.resize(3 * (size_t)h.P); h.S.resize(36 * (size_t)h.K * h.K); h.bs.resize(6 * (size_t)h.K);
    h.xp.assign(6 * (size_t)h.K, 0.); h.xl.assign(3 * (size_t)h.P, 0.); h.Y.resize(18 * (size_t)max_deg);

    orbp_lba_stats st;
    memset(&st, 0, sizeof st);
    LbaRun run = {0, 0, 0, 0};
    h.robust = true;
    h.activate();                                               // :659
    if (h.n_active > 0) {
        lba_optimize(h, 5, run);                                // :660
        st.iterations[0] = run.iterations; st.trials[0] = run.trials; st.lambda = run.lambda; st.chi2 = run.chi2;
    }
    if (!orbp_lba_read_stop(stop)) {                            // :662-709
        st.second_round = 1;
        for (int e = 0; e < h.E; e++)
            if (h.flagged(e)) { h.level[e] = 1; st.n_level1++; }
        h.robust = false;
        h.activate();                                           // :706
        if (h.n_active > 0) {
            lba_optimize(h, 10, run);                           // :707
            st.iterations[1] = run.iterations; st.trials[1] = run.trials; st.lambda = run.lambda; st.chi2 = run.chi2;
        }
    }
    for (int e = 0; e < h.E; e++) erase[e] = h.flagged(e) ? 1 : 0;      // :715-743
    for (int k = 0; k < h.K; k++) lba_se3_to_Tcw(h.est[k], Tcw_local + 16 * (size_t)k);    // :762-768
    for (size_t i = 0; i < h.xw.size(); i++) xw[i] = (float)h.xw[i];                       // :771-777
    if (stats) *stats = st;
    return ORBP_LBA_DONE;
}
