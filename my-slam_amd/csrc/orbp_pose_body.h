// orbp_pose_body.h -- the arithmetic of Optimizer::PoseOptimization (src/Optimizer.cc:239-451 of WChen09/My-SLAM, on g2o), one text
// for the host solver (orbp_pose.cc, plain C++) and for the kernel (orbm_pose.hip).  SE3Quat and RobustKernelHuber are
// orbp_se3_body.h.  Restated here from Thirdparty/g2o/g2o:
//   EdgeSE3ProjectXYZOnlyPose        computeError types/types_six_dof_expmap.h:153-157, linearizeOplus .cpp:266-288
//   EdgeStereoSE3ProjectXYZOnlyPose  computeError .h:184-188 with cam_project's float invz .cpp:290-306, linearizeOplus .cpp:335-364
//   constructQuadraticForm           core/base_unary_edge.hpp:43-72
//   LinearSolverDense                Eigen's LDLT of the 6 x 6 system: lm_ldlt_solve<6> (orbp_lm_body.h)
//   OptimizationAlgorithmLevenberg   core/optimization_algorithm_levenberg.cpp:66-170 (with this fork's _nBad stop :157-164), driven
//                                    by SparseOptimizer::optimize(10) (core/sparse_optimizer.cpp:354-420)
//
// Everything is fp64 and uses + - * / sqrt alone (the build's -ffp-contract=off keeps them unfused), except se3_exp (sin, cos) and
// the one float division of the stereo error.  Every per-edge quantity is therefore the same on host and device; a side owns the
// order of its sums over the edges and nothing else.
//
// A side is a context with
//   ctx.system(T, robust, sys)   computeActiveErrors + linearizeOplus + constructQuadraticForm at T over the edges that are not
//                                flagged: sys[POSE_NSYS], the robust chi2 of those edges in sys[POSE_CHI]
//   ctx.chi2(T, robust)          computeActiveErrors + activeRobustChi2
//   ctx.flag(est, err_est)       the flagging pass over all edges (pose_edge_is_outlier), the number of outliers
// Edge state without per-edge storage: g2o leaves the errors of a rejected trial on the edges and the flagging pass reads them.  The
// errors of all active edges are always those at the estimate computeActiveErrors last saw, and an inactive edge is recomputed at
// the final estimate before it is read, so one extra estimate (err_est) stands for the per-edge store.  A side may still keep a
// PoseEdge between two passes at one estimate, as the host does: what it keeps is what pose_edge_error would give anew.
#pragma once
#include <stdint.h>
#include "orbp_lm_body.h"
#include "orbp_se3_body.h"

// always inlined on the host as well: its passes call these per edge, and g++ -O2 leaves pose_edge_error out of line otherwise
#if defined(__HIPCC__)
#define POSE_HD SE3_HD
#else
#define POSE_HD static inline __attribute__((always_inline))
#endif

#define POSE_NSYS 28            // 21 upper-triangle entries of H (row-major), 6 of b, the robust chi2
#define POSE_B0 21
#define POSE_CHI 27

struct PoseCam { double fx, fy, cx, cy, bf; };
// the flat problem: orbp_pose_optimization's arrays (include/orbp.h); outlier is read as "not in the active set"
struct PoseEdges { const float *obs, *u_right, *inv_sigma2, *xw; uint8_t *outlier; };
// an edge as orbp_pose_optimization builds it (pose_edge_load), then the point in the camera frame and the error at one estimate
// (pose_edge_error)
struct PoseEdge { bool stereo; double o0, o1, o2, info, x0, x1, x2, pc0, pc1, pc2, e0, e1, e2; };

POSE_HD void pose_edge_load(PoseEdge &e, const PoseEdges &E, long long i)
{
    const float ur = E.u_right ? E.u_right[i] : -1.0f;
    e.stereo = E.u_right && ur >= 0;
    e.o0 = E.obs[2 * i]; e.o1 = E.obs[2 * i + 1]; e.o2 = e.stereo ? (double)ur : 0.0;
    e.info = E.inv_sigma2[i];
    e.x0 = E.xw[3 * i]; e.x1 = E.xw[3 * i + 1]; e.x2 = E.xw[3 * i + 2];
}
POSE_HD void pose_edge_error(PoseEdge &e, const Se3 &T, const PoseCam &cam)
{
    quat_rotate(T, e.x0, e.x1, e.x2, e.pc0, e.pc1, e.pc2);
    e.pc0 += T.t0; e.pc1 += T.t1; e.pc2 += T.t2;
    if (!e.stereo) {
        e.e0 = e.o0 - (e.pc0 / e.pc2 * cam.fx + cam.cx);
        e.e1 = e.o1 - (e.pc1 / e.pc2 * cam.fy + cam.cy);
        e.e2 = 0;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        const float invz = __fdiv_rn(1.0f, (float)e.pc2);      // the correctly rounded quotient the host's division is
#else
        const float invz = 1.0f / (float)e.pc2;
#endif
        const double u = e.pc0 * invz * cam.fx + cam.cx;
        e.e0 = e.o0 - u;
        e.e1 = e.o1 - (e.pc1 * invz * cam.fy + cam.cy);
        e.e2 = e.o2 - (u - cam.bf * invz);
    }
}
// chi2() with information = inv_sigma2 * I; not LocalBundleAdjustment's association (lba_chi2)
POSE_HD double pose_chi2(const PoseEdge &e) { return (e.e0 * e.e0 + e.e1 * e.e1 + e.e2 * e.e2) * e.info; }

// One active edge with its error: its robust chi2 into acc[SYSTEM ? POSE_CHI : 0] and, with SYSTEM, b -= rho' J^T Omega e and
// H += J^T (rho' Omega) J on the upper triangle, from the same error.  The deltas are const float deltaMono / deltaStereo (:270-271).
// Written out per row count so the compiler sees fixed trip counts; the sums keep the order 0 + row0 + row1 (+ row2).
template <bool SYSTEM>
POSE_HD void pose_edge_sums(const PoseEdge &e, const PoseCam &cam, bool robust, double *acc)
{
    const double c2 = pose_chi2(e);
    double rho0 = c2, w = 1.0;
    if (robust) huber(c2, e.stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991), rho0, w);
    acc[SYSTEM ? POSE_CHI : 0] += rho0;
    if (!SYSTEM) return;
    // the edge by value: on the host acc may alias it for all the compiler knows
    const bool stereo = e.stereo;
    const double info = e.info, e0 = e.e0, e1 = e.e1, e2 = e.e2;
    const double x = e.pc0, y = e.pc1, invz = 1.0 / e.pc2, invz_2 = invz * invz;
    const double fx = cam.fx, fy = cam.fy, bf = cam.bf;
    double J[3][6];
    J[0][0] = x * y * invz_2 * fx; J[0][1] = -(1 + (x * x * invz_2)) * fx; J[0][2] = y * invz * fx;
    J[0][3] = -invz * fx; J[0][4] = 0; J[0][5] = x * invz_2 * fx;
    J[1][0] = (1 + y * y * invz_2) * fy; J[1][1] = -x * y * invz_2 * fy; J[1][2] = -x * invz * fy;
    J[1][3] = 0; J[1][4] = -invz * fy; J[1][5] = y * invz_2 * fy;
    const double wi = w * info;
    double wJ[3][6];
    for (int r = 0; r < 6; r++) { wJ[0][r] = J[0][r] * wi; wJ[1][r] = J[1][r] * wi; }
    if (!stereo) {
        int u = 0;
        for (int r = 0; r < 6; r++) {
            const double g = J[0][r] * info * e0 + J[1][r] * info * e1;
            acc[POSE_B0 + r] -= w * g;
            for (int c = r; c < 6; c++, u++) acc[u] += wJ[0][r] * J[0][c] + wJ[1][r] * J[1][c];
        }
    } else {
        J[2][0] = J[0][0] - bf * y * invz_2; J[2][1] = J[0][1] + bf * x * invz_2; J[2][2] = J[0][2];
        J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - bf * invz_2;
        for (int r = 0; r < 6; r++) wJ[2][r] = J[2][r] * wi;
        int u = 0;
        for (int r = 0; r < 6; r++) {
            const double g = J[0][r] * info * e0 + J[1][r] * info * e1 + J[2][r] * info * e2;
            acc[POSE_B0 + r] -= w * g;
            for (int c = r; c < 6; c++, u++) acc[u] += wJ[0][r] * J[0][c] + wJ[1][r] * J[1][c] + wJ[2][r] * J[2][c];
        }
    }
}
// The flagging pass (:384-440) reads an outlier of the last round at the final estimate and every other edge at the estimate the
// optimiser last evaluated (err_est); the float chi2 against 5.991 / 7.815
POSE_HD bool pose_edge_is_outlier(const PoseEdge &e) { return (float)pose_chi2(e) > (e.stereo ? 7.815f : 5.991f); }

// The Levenberg loop for the one 6-dof vertex, in the shape of s3o_optimize (orbp_sim3opt_body.h).  err_est follows the estimate the
// errors on the active edges were last computed at: a rejected trial restores the vertex, not the edges.  The bounds are fixed: at
// most 10 iterations of at most 10 trials.
template <class Ctx>
POSE_HD void pose_optimize(Ctx &ctx, bool robust, Se3 &est, Se3 &err_est)
{
    double lambda = 0, ni = 2;
    int lm_bad = 0;
    for (int it = 0; it < 10; it++) {
        double sys[POSE_NSYS], x[6];
        // right after an accepted step the chi2 summed here is the one the trial summed: same edges, same estimate, same order
        ctx.system(est, robust, sys);
        err_est = est;
        double current = sys[POSE_CHI], temp = current;
        const double ini = current;
        if (it == 0) {
            const double mx = fmax(fabs(sys[20]), fmax(fabs(sys[18]), fmax(fabs(sys[15]), fmax(fabs(sys[11]), fmax(fabs(sys[6]), fmax(fabs(sys[0]), 0.0))))));
            lambda = 1e-5 * mx; ni = 2; lm_bad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const Se3 backup = est;
            const bool ok2 = lm_ldlt_solve<6>(sys, lambda, sys + POSE_B0, x);
            est = se3_mul(se3_exp(x), est);     // VertexSE3Expmap::oplusImpl
            temp = ctx.chi2(est, robust);
            err_est = est;
            if (!ok2) temp = 1.7976931348623157e308;
            rho = current - temp;
            double scale = 0;
            for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + sys[POSE_B0 + j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(temp)) {
                const double t = 2 * rho - 1;
                double alpha = 1. - t * t * t;          // pow(2 rho - 1, 3) as two multiplications on both sides
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                current = temp;
            } else {
                lambda *= ni;
                ni *= 2;
                est = backup;                           // err_est stays at the trial, as the edges do in g2o
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) break;
        if ((ini - current) * 1e3 < ini) lm_bad++; else lm_bad = 0;
        if (lm_bad >= 3) break;
    }
}

// The four rounds over n >= 3 edges, none of them flagged: the final estimate in est, the number of outliers returned
template <class Ctx>
POSE_HD int pose_rounds(Ctx &ctx, int n, const Se3 &init, Se3 &est)
{
    Se3 err_est = est = init;
    int n_bad = 0;
    for (int round = 0; round < 4; round++) {
        est = init;                             // every round restarts from pFrame->mTcw (:375)
        // setRobustKernel(0) after the third round (:435-436); optimize() returns on an empty active set
        if (n - n_bad > 0) pose_optimize(ctx, round < 3, est, err_est);
        n_bad = ctx.flag(est, err_est);
        if (n < 10) break;                      // optimizer.edges().size() < 10 (:443-444)
    }
    return n_bad;
}
