// orbp_sim3opt_body.h -- the per-pair arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241 of WChen09/My-SLAM, on g2o),
// one text for the host solver (orbp_sim3opt.cc, plain C++) and for the kernel (orbm_sim3opt.hip): g2o::Sim3 (types/sim3.h), the
// computeError of EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ (types/types_seven_dof_expmap.h:138-145, 160-167), the numeric
// Jacobian g2o falls back to because both linearizeOplus are commented out (:147, :169; core/base_binary_edge.hpp:130-205),
// RobustKernelHuber (core/robust_kernel_impl.cpp:78-91) and one edge's constructQuadraticForm (base_binary_edge.hpp:55-120).
//
// Everything is fp64 and uses + - * / sqrt alone (the build's -ffp-contract=off keeps them unfused), except s3o_exp, which calls
// sin, cos and exp of the side it is compiled for.  A numeric perturbation never reaches sin or cos (its theta is 1e-9 or 0), and
// reaches exp only with +-1e-9 or 0.
#pragma once
#include <math.h>
#include <stdint.h>
#include "orbp_lm_body.h"
#include "orbp_se3_body.h"

#if defined(__HIPCC__)
#define S3O_HD __host__ __device__ __forceinline__
#define S3O_UNROLL _Pragma("unroll")
#define S3O_NO_UNROLL _Pragma("unroll 1")
#else
#define S3O_HD static inline
#define S3O_UNROLL
#define S3O_NO_UNROLL
#endif

#define S3O_NSYS 36             // 28 upper-triangle entries of H (row-major), 7 of b, the robust chi2
#define S3O_B0 28
#define S3O_CHI 35
#define S3O_NLIN 15             // the estimate, then +delta and -delta along each of the 7 axes

// g2o::Sim3: r (Eigen's coefficient order x, y, z, w; never normalised), t, s
struct S3oSim : Quat { double t0, t1, t2, s; };
struct S3oCam { double fx, fy, cx, cy; };

// Sim3::map (sim3.h:144-146): s * (r * xyz) + t
S3O_HD void s3o_map(const S3oSim &S, double x0, double x1, double x2, double &o0, double &o1, double &o2)
{
    double r0, r1, r2;
    quat_rotate(S, x0, x1, x2, r0, r1, r2);
    o0 = S.s * r0 + S.t0; o1 = S.s * r1 + S.t1; o2 = S.s * r2 + S.t2;
}
// Sim3::operator* (sim3.h:266-272): nothing is normalised
S3O_HD S3oSim s3o_mul(const S3oSim &a, const S3oSim &b)
{
    S3oSim r;
    quat_mul(a, b, r);
    s3o_map(a, b.t0, b.t1, b.t2, r.t0, r.t1, r.t2);
    r.s = a.s * b.s;
    return r;
}
// Sim3::inverse (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
S3O_HD S3oSim s3o_inverse(const S3oSim &a)
{
    S3oSim r;
    r.qx = -a.qx; r.qy = -a.qy; r.qz = -a.qz; r.qw = a.qw;
    const double f = -1. / a.s;
    quat_rotate(r, f * a.t0, f * a.t1, f * a.t2, r.t0, r.t1, r.t2);
    r.s = 1. / a.s;
    return r;
}
// Sim3(const Vector7d &) (sim3.h:70-142): omega, upsilon, sigma; four branches on eps = 1e-5.  The small-angle branches take
// R = I + Omega + Omega * Omega (no 1/2) and Quaterniond(R) of that matrix, which is not a rotation
S3O_HD S3oSim s3o_exp(const double *u)
{
    const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
    const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
    double O2[9], R[9];
    S3O_UNROLL
    for (int i = 0; i < 3; i++)
        S3O_UNROLL
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    S3oSim S;
    S.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.; B = 1. / 6.;
            S3O_UNROLL
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) + O[i]) + O2[i];
        } else {
            const double theta2 = theta * theta, sn = sin(theta), cs = cos(theta);
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
            const double a = sn / theta, b = (1 - cs) / (theta * theta);
            S3O_UNROLL
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) + a * O[i]) + b * O2[i];
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
            S3O_UNROLL
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) + O[i]) + O2[i];
        } else {
            const double sn = sin(theta), cs = cos(theta);
            const double ra = sn / theta, rb = (1 - cs) / (theta * theta);
            S3O_UNROLL
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) + ra * O[i]) + rb * O2[i];
            const double a = S.s * sn, b = S.s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    quat_from_R(R, S);
    double W[9];
    S3O_UNROLL
    for (int i = 0; i < 9; i++) W[i] = (A * O[i] + B * O2[i]) + C * (i % 4 == 0);
    S.t0 = W[0] * u[3] + W[1] * u[4] + W[2] * u[5];
    S.t1 = W[3] * u[3] + W[4] * u[4] + W[5] * u[5];
    S.t2 = W[6] * u[3] + W[7] * u[4] + W[8] * u[5];
    return S;
}
// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): update[6] = 0 under _fix_scale, then Sim3(update) * estimate
S3O_HD S3oSim s3o_oplus(const S3oSim &est, const double *update, bool fix_scale)
{
    double u[7];
    S3O_UNROLL
    for (int j = 0; j < 6; j++) u[j] = update[j];
    u[6] = fix_scale ? 0.0 : update[6];
    return s3o_mul(s3o_exp(u), est);
}
// Entry k of one linearisation (base_binary_edge.hpp:147-196): k = 0 is the estimate, k = 1 + 2d the vertex pushed, updated by
// +1e-9 along axis d and popped again, k = 2 + 2d the same with -1e-9.  inv is what EdgeInverseSim3ProjectXYZ maps with.  Under
// fix_scale both entries of axis 6 are Sim3(0) * estimate, so the seventh Jacobian column is exactly zero.
S3O_HD void s3o_lin_entry(const S3oSim &est, int k, bool fix_scale, S3oSim &e, S3oSim &inv)
{
    if (k == 0) e = est;
    else {
        const int d = (k - 1) >> 1;
        const double delta = ((k - 1) & 1) ? -1e-9 : 1e-9;
        double u[7];
        S3O_UNROLL
        for (int j = 0; j < 7; j++) u[j] = (j == d) ? delta : 0.0;
        e = s3o_oplus(est, u, fix_scale);
    }
    inv = s3o_inverse(e);
}

// obs - cam_map(project(S.map(x))): with the estimate and x2c it is EdgeSim3ProjectXYZ::computeError, with its inverse and x1c
// EdgeInverseSim3ProjectXYZ::computeError
S3O_HD void s3o_error(const S3oSim &S, const S3oCam &cam, const float *x, const float *obs, double &e0, double &e1)
{
    double p0, p1, p2;
    s3o_map(S, (double)x[0], (double)x[1], (double)x[2], p0, p1, p2);
    e0 = (double)obs[0] - (p0 / p2 * cam.fx + cam.cx);
    e1 = (double)obs[1] - (p1 / p2 * cam.fy + cam.cy);
}
S3O_HD double s3o_chi2(double e0, double e1, double info) { return (e0 * e0 + e1 * e1) * info; }

// One edge: its robust chi2 into acc[S3O_CHI] and, with SYSTEM, the numeric Jacobian over lin[1..14] (scaled by 1 / (2 delta)) and
// constructQuadraticForm: b += J^T (rho' * -(Omega e)), H += J^T (rho' Omega) J, upper triangle.  lin is the e or the inv array of a
// linearisation.  J holds the 2 x 7 Jacobian between its two loops: entry (r, d) at J[(7 r + d) * js].  The loop that fills it is
// kept rolled in the kernel, which gives every thread a column of LDS for it (js = the workgroup's size): unrolled, the compiler
// keeps all 30 estimates of the linearisation in registers across the pairs and spills.
template <bool SYSTEM>
S3O_HD void s3o_edge(const S3oSim *lin, const S3oCam &cam, const float *x, const float *obs, double info, double huber_delta, double *acc,
                     double *J, int js)
{
    double e0, e1, rho0, rho1;
    s3o_error(lin[0], cam, x, obs, e0, e1);
    huber(s3o_chi2(e0, e1, info), huber_delta, rho0, rho1);
    acc[SYSTEM ? S3O_CHI : 0] += rho0;
    if (!SYSTEM) return;
    const double scalar = 1.0 / (2 * 1e-9);
    S3O_NO_UNROLL
    for (int d = 0; d < 7; d++) {
        double p0, p1, m0, m1;
        s3o_error(lin[1 + 2 * d], cam, x, obs, p0, p1);
        s3o_error(lin[2 + 2 * d], cam, x, obs, m0, m1);
        J[d * js] = scalar * (p0 - m0);
        J[(7 + d) * js] = scalar * (p1 - m1);
    }
    double J0[7], J1[7];
    S3O_UNROLL
    for (int d = 0; d < 7; d++) { J0[d] = J[d * js]; J1[d] = J[(7 + d) * js]; }
    const double w = rho1 * info;
    const double r0 = -(info * e0) * rho1, r1 = -(info * e1) * rho1;
    int u = 0;
    S3O_UNROLL
    for (int r = 0; r < 7; r++) {
        acc[S3O_B0 + r] += J0[r] * r0 + J1[r] * r1;
        const double w0 = J0[r] * w, w1 = J1[r] * w;
        S3O_UNROLL
        for (int c = r; c < 7; c++, u++) acc[u] += w0 * J0[c] + w1 * J1[c];
    }
}
// One correspondence, in g2o's edge order: e12 (x1 = S12 * X2, camera 1), then e21 (x2 = S21 * X1, camera 2)
template <bool SYSTEM>
S3O_HD void s3o_pair(const S3oSim *lin_e, const S3oSim *lin_inv, const S3oCam &cam1, const S3oCam &cam2, const float *x1c, const float *x2c,
                     const float *obs1, const float *obs2, float inv_sigma2_1, float inv_sigma2_2, double huber_delta, double *acc,
                     double *J, int js)
{
    s3o_edge<SYSTEM>(lin_e, cam1, x2c, obs1, (double)inv_sigma2_1, huber_delta, acc, J, js);
    s3o_edge<SYSTEM>(lin_inv, cam2, x1c, obs2, (double)inv_sigma2_2, huber_delta, acc, J, js);
}
// e12->chi2() > th2 || e21->chi2() > th2 (src/Optimizer.cc:1193, 1227) with the errors at S: the double chi2 against the float th2
S3O_HD bool s3o_pair_bad(const S3oSim &S, const S3oSim &Sinv, const S3oCam &cam1, const S3oCam &cam2, const float *x1c, const float *x2c,
                         const float *obs1, const float *obs2, float inv_sigma2_1, float inv_sigma2_2, float th2)
{
    double a0, a1, b0, b1;
    s3o_error(S, cam1, x2c, obs1, a0, a1);
    s3o_error(Sinv, cam2, x1c, obs2, b0, b1);
    return s3o_chi2(a0, a1, (double)inv_sigma2_1) > (double)th2 || s3o_chi2(b0, b1, (double)inv_sigma2_2) > (double)th2;
}

// OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:66-170, with this fork's _nBad stop :157-164)
// driven by SparseOptimizer::optimize(iterations) (core/sparse_optimizer.cpp:354-420), as pose_optimize (orbp_pose_body.h) restates
// it for six unknowns, for the one 7-dof vertex.  ctx.system(T, sys) is computeActiveErrors + linearizeOplus + constructQuadraticForm at T with the
// robust chi2 of the active edges in sys[S3O_CHI]; ctx.chi2(T) is computeActiveErrors + activeRobustChi2.  err_est follows the
// estimate the errors on the active edges were last computed at: a rejected trial restores the vertex, not the edges
// ("Edge state without per-edge storage").  The bounds are fixed: at most 10 iterations of at most 10 trials.
template <class Ctx>
S3O_HD void s3o_optimize(Ctx &ctx, S3oSim &est, S3oSim &err_est, bool fix_scale, int iterations)
{
    double lambda = 0, ni = 2;
    int lm_bad = 0;
    for (int it = 0; it < 10; it++) {
        if (it >= iterations) break;
        double sys[S3O_NSYS], x[7];
        // right after an accepted step the chi2 summed here is the one the trial summed: same edges, same estimate, same order
        ctx.system(est, sys);
        err_est = est;
        double current = sys[S3O_CHI], temp = current;
        const double ini = current;
        if (it == 0) {
            const double d0 = fabs(sys[0]), d1 = fabs(sys[7]), d2 = fabs(sys[13]), d3 = fabs(sys[18]), d4 = fabs(sys[22]),
                         d5 = fabs(sys[25]), d6 = fabs(sys[27]);
            const double mx = fmax(d6, fmax(d5, fmax(d4, fmax(d3, fmax(d2, fmax(d1, fmax(d0, 0.0)))))));
            lambda = 1e-5 * mx; ni = 2; lm_bad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const S3oSim backup = est;
            const bool ok2 = lm_ldlt_solve<7>(sys, lambda, sys + S3O_B0, x);
            est = s3o_oplus(est, x, fix_scale);
            temp = ctx.chi2(est);
            err_est = est;
            if (!ok2) temp = 1.7976931348623157e308;
            rho = current - temp;
            double scale = 0;
            S3O_UNROLL
            for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + sys[S3O_B0 + j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(temp)) {
                const double t = 2 * rho - 1;
#if defined(__HIP_DEVICE_COMPILE__)
                double alpha = 1. - t * t * t;          // the host's pow(2 rho - 1, 3) as two multiplications
#else
                double alpha = 1. - pow(t, 3);
#endif
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
