// orbp_eg_body.h -- the per-edge arithmetic of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044 of WChen09/My-SLAM, on
// g2o), one text for the host solver (orbp_eg.cc, plain C++) and for the kernels (orbm_eg.hip).  g2o::Sim3 and its arithmetic, the
// oplus of VertexSim3Expmap and the entries of a numeric linearisation are orbp_sim3opt_body.h.  Restated here from Thirdparty/g2o/g2o:
//   Sim3::log                       types/sim3.h:148-230, with deltaR and skew of types/se3_ops.hpp:27-47
//   EdgeSim3::computeError          types/types_seven_dof_expmap.h:106-114
//   linearizeOplus (numeric)        core/base_binary_edge.hpp:130-205, delta = 1e-9, both vertices or the free one
//   constructQuadraticForm          core/base_binary_edge.hpp:55-90, information = identity, no robust kernel
//   the write-back                  src/Optimizer.cc:992-1043
//
// Everything is fp64 and uses + - * / sqrt alone (the build's -ffp-contract=off keeps them unfused), except s3o_exp (sin, cos, exp)
// and eg_log (log, acos, sin, cos), which call the library of the side they are compiled for.  Unlike OptimizeSim3's, a numeric
// perturbation here does reach them: the perturbed estimate goes through log(), so one ulp of difference between two libraries
// becomes about 1e-7 in the Jacobian (1e-16 / 2e-9) and moves the Gauss-Newton fixed point by as much.
#pragma once
#include "orbp_sim3opt_body.h"

#define EG_NLIN 29              // the estimates, then +delta and -delta along the 7 axes of vertex 0, then of vertex 1

S3O_HD S3oSim eg_load(const double *p) { return {{p[0], p[1], p[2], p[3]}, p[4], p[5], p[6], p[7]}; }     // Sim3::operator[] order
S3O_HD void eg_store(double *p, const S3oSim &S)
{
    p[0] = S.qx; p[1] = S.qy; p[2] = S.qz; p[3] = S.qw; p[4] = S.t0; p[5] = S.t1; p[6] = S.t2; p[7] = S.s;
}
// W.lu().solve(t) (sim3.h:217): Eigen's PartialPivLU of a 3 x 3 matrix, unblocked -- per column the first row of largest
// magnitude comes up, a zero pivot skips its division -- then the permuted t through the unit lower and the upper triangle
S3O_HD void eg_lu_solve3(const double *W, const double *t, double *x)
{
    double a[3][3] = {{W[0], W[1], W[2]}, {W[3], W[4], W[5]}, {W[6], W[7], W[8]}};
    double b[3] = {t[0], t[1], t[2]};
    S3O_UNROLL
    for (int k = 0; k < 3; k++) {
        int piv = k;
        double big = fabs(a[k][k]);
        S3O_UNROLL
        for (int i = k + 1; i < 3; i++)
            if (fabs(a[i][k]) > big) { big = fabs(a[i][k]); piv = i; }
        S3O_UNROLL
        for (int i = k + 1; i < 3; i++)
            if (i == piv) {
                S3O_UNROLL
                for (int c = 0; c < 3; c++) { const double w = a[k][c]; a[k][c] = a[i][c]; a[i][c] = w; }
                const double w = b[k]; b[k] = b[i]; b[i] = w;
            }
        S3O_UNROLL
        for (int i = k + 1; i < 3; i++) {
            if (big != 0) a[i][k] /= a[k][k];
            S3O_UNROLL
            for (int c = k + 1; c < 3; c++) a[i][c] -= a[i][k] * a[k][c];
        }
    }
    b[1] -= a[1][0] * b[0];
    b[2] -= a[2][0] * b[0];
    b[2] -= a[2][1] * b[1];
    x[2] = b[2] / a[2][2];
    x[1] = (b[1] - a[1][2] * x[2]) / a[1][1];
    x[0] = ((b[0] - a[0][1] * x[1]) - a[0][2] * x[2]) / a[0][0];
}
// Sim3::log (sim3.h:148-230): omega, upsilon, sigma
S3O_HD void eg_log(const S3oSim &S, double *res)
{
    const double sigma = log(S.s);
    double R[9];
    quat_to_R(S, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};       // deltaR
    const double eps = 0.00001;
    double A, B, C, f;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            f = 0.5; A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            f = theta / (2 * sqrt(1 - d * d));
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            f = 0.5;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            f = theta / (2 * sqrt(1 - d * d));
            const double theta2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double om0 = f * dR[0], om1 = f * dR[1], om2 = f * dR[2];
    const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};     // skew
    double W[9];
    // A * Omega + (B * Omega) * Omega + C * I
    S3O_UNROLL
    for (int i = 0; i < 3; i++)
        S3O_UNROLL
        for (int j = 0; j < 3; j++) {
            const double p = ((B * O[3 * i]) * O[j] + (B * O[3 * i + 1]) * O[3 + j]) + (B * O[3 * i + 2]) * O[6 + j];
            W[3 * i + j] = (A * O[3 * i + j] + p) + C * (i == j);
        }
    const double t[3] = {S.t0, S.t1, S.t2};
    res[0] = om0; res[1] = om1; res[2] = om2;
    eg_lu_solve3(W, t, res + 3);
    res[6] = sigma;
}
// EdgeSim3::computeError: (C * v0->estimate() * v1->estimate().inverse()).log(), the product from the left
S3O_HD void eg_error(const S3oSim &C, const S3oSim &Si, const S3oSim &Sj_inv, double *err)
{
    eg_log(s3o_mul(s3o_mul(C, Si), Sj_inv), err);
}
// chi2(): _error.dot(information() * _error) under the identity
S3O_HD double eg_chi2(const double *e)
{
    double c = 0;
    S3O_UNROLL
    for (int r = 0; r < 7; r++) c += e[r] * e[r];
    return c;
}
// The error of entry k of one edge's linearisation (base_binary_edge.hpp:147-200): k = 0 at the estimates; k = 1 .. 14 with vertex
// 0 pushed, updated along an axis and popped (s3o_lin_entry's numbering), k = 15 .. 28 the same for vertex 1.  A fixed vertex's
// entries are never asked for.
S3O_HD void eg_lin_error(const S3oSim &C, const S3oSim &Si, const S3oSim &Sj, int k, bool fix_scale, double *err)
{
    const bool second = k >= 15;
    S3oSim P, Pinv;
    s3o_lin_entry(second ? Sj : Si, second ? k - 14 : k, fix_scale, P, Pinv);
    if (!second) Pinv = s3o_inverse(Sj);
    eg_error(C, second ? Si : P, Pinv, err);
}
// One Jacobian entry from the two errors of its axis: scalar * (errorBak - _error) with scalar = 1 / (2 delta)
S3O_HD double eg_jac(double plus, double minus) { return (1.0 / (2 * 1e-9)) * (plus - minus); }

// constructQuadraticForm, one edge's terms; J, K are 7 x 7 row-major Jacobians (row = error component, column = axis):
//   b_v += J^T omega_r with omega_r = -e;  H_vv += J^T J;  H_ij += J_i^T J_j (its transpose where vertex j's rows come first)
S3O_HD double eg_b_term(const double *J, const double *e, int a)
{
    double s = 0;
    S3O_UNROLL
    for (int r = 0; r < 7; r++) s += J[7 * r + a] * -e[r];
    return s;
}
S3O_HD double eg_h_term(const double *J, const double *K, int a, int b)
{
    double s = 0;
    S3O_UNROLL
    for (int r = 0; r < 7; r++) s += J[7 * r + a] * K[7 * r + b];
    return s;
}

// src/Optimizer.cc:999-1009: Tiw = [R | t / s] of the corrected Sim3, as floats (Converter::toCvSE3)
S3O_HD void eg_to_Tcw(const S3oSim &S, float *T)
{
    double R[9];
    quat_to_R(S, R);
    const double f = 1. / S.s;
    S3O_UNROLL
    for (int i = 0; i < 3; i++)
        S3O_UNROLL
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j];
    T[3] = (float)(S.t0 * f); T[7] = (float)(S.t1 * f); T[11] = (float)(S.t2 * f);
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}
// :1032-1040: correctedSwr.map(Srw.map(P)), to float
S3O_HD void eg_correct_point(const S3oSim &Srw, const S3oSim &corrected_Srw, float *x)
{
    double a0, a1, a2, b0, b1, b2;
    s3o_map(Srw, (double)x[0], (double)x[1], (double)x[2], a0, a1, a2);
    s3o_map(s3o_inverse(corrected_Srw), a0, a1, a2, b0, b1, b2);
    x[0] = (float)b0; x[1] = (float)b1; x[2] = (float)b2;
}
