// orbp_lba_body.h -- the arithmetic of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778 of WChen09/My-SLAM, on g2o), one text
// for the host solver (orbp_lba.cc, plain C++) and for the kernels (orbm_lba.hip).  Restated from Thirdparty/g2o/g2o:
//   SE3Quat, RobustKernelHuber      orbp_se3_body.h
//   EdgeSE3ProjectXYZ               computeError types/types_six_dof_expmap.h:109-114, isDepthPositive :116-120,
//                                   linearizeOplus types_six_dof_expmap.cpp:103-139, cam_project :141-147
//   EdgeStereoSE3ProjectXYZ         computeError .h:139-144, isDepthPositive :146-150, linearizeOplus .cpp:188-235,
//                                   cam_project with its float invz :150-157
//   constructQuadraticForm          core/base_binary_edge.hpp:55-120, one or both vertices free
//   VertexSE3Expmap::oplusImpl      types_six_dof_expmap.h:62-65 (exp(update) * estimate); VertexSBAPointXYZ::oplusImpl types_sba.h (+=)
//   BlockSolver_6_3::solve          core/block_solver.hpp:354-486 (Schur complement), setLambda :564-589
//   OptimizationAlgorithmLevenberg  the loop itself, lm_optimize, is orbp_lm_body.h
//
// Semantics kept (include/orbp.h, orbp_local_bundle_adjustment, lists them for the caller):
//   rounds        optimize(5); the flagging pass :672-702 (chi2 > 5.991 / 7.815 on the double chi2(), or depth not positive, sets
//                 level 1; every edge loses its robust kernel); initializeOptimization(0) and optimize(10), which starts again at
//                 iteration 0 (new lambda, _ni = 2, _nBad = 0)
//   stale errors  an edge stores the error computeActiveErrors last wrote while the edge was active, a rejected trial's included;
//                 the final pass :715-743 reads chi2() from it and evaluates isDepthPositive() at the final estimates
//   vertices without active edges leave the second round's active set: their estimates keep the first round's bits
//   fixed key frames contribute to the point's blocks only; a local key frame with mnId == 0 is fixed
//   stop          read at the top of every iteration and in the do ... while of the trial loop (sparse_optimizer.cpp:376,
//                 optimization_algorithm_levenberg.cpp:149)
//
// Everything is fp64 and uses + - * / sqrt alone (the build's -ffp-contract=off keeps them unfused), except se3_exp, which calls
// sin and cos of the side it is compiled for.  Every per-edge quantity (camera point, error, chi2, Huber weight, both Jacobians, the
// 54 numbers of the edge's quadratic form) is therefore the same on host and device; the order of the sums over edges, sin / cos
// and the inside of the dense solve are not.
//
// Chosen here where the flat problem does not carry what g2o orders by: g2o numbers its unknowns by vertex id (key frames by mnId,
// points by mnId); the problem has no ids, so the unknowns stand in problem order (lLocalKeyFrames, lLocalMapPoints).  That moves
// the order of computeScale's sum and of the elimination, nothing else.  A free key frame without active edges keeps an identity
// block in the reduced system instead of leaving it (its update is exactly zero and is not applied).  When the solve fails the
// update is zero (g2o applies whatever its x held before).
#pragma once
#include <math.h>
#include <stdint.h>
#include "orbp_lm_body.h"
#include "orbp_se3_body.h"

#if defined(__HIPCC__)
#define LBA_HD __host__ __device__ __forceinline__
#else
#define LBA_HD static inline
#endif

typedef Se3 LbaSe3;                                     // the group itself is orbp_se3_body.h
struct LbaCam { double fx, fy, cx, cy, bf; };

// an edge's quadratic form: the upper triangles row-major, Hpl = B^T Omega A (6 x 3, row-major; B the pose Jacobian, A the point's)
#define LBA_NBLK 54
#define LBA_HPP 0               // 21
#define LBA_BP 21               // 6
#define LBA_HLL 27              // 6
#define LBA_BL 33               // 3
#define LBA_HPL 36              // 18

// VertexSE3Expmap::oplusImpl: setEstimate(SE3Quat::exp(update) * estimate())
LBA_HD LbaSe3 lba_pose_oplus(const LbaSe3 &est, const double *update) { return se3_mul(se3_exp(update), est); }

// computeError of both edges: pc = the point in the camera frame, err = obs - cam_project(pc) (err[2] = 0 on a monocular edge).
// The stereo cam_project divides in double and keeps the quotient as a float (types_six_dof_expmap.cpp:151).
LBA_HD void lba_edge_error(const LbaSe3 &T, const LbaCam &c, const double *xw, const float *obs, float u_right, double *pc, double *err)
{
    se3_map(T, xw, pc);
    if (u_right < 0) {
        err[0] = (double)obs[0] - (pc[0] / pc[2] * c.fx + c.cx);
        err[1] = (double)obs[1] - (pc[1] / pc[2] * c.fy + c.cy);
        err[2] = 0;
    } else {
        const float invz = (float)(1.0 / pc[2]);
        const double u = pc[0] * invz * c.fx + c.cx;
        err[0] = (double)obs[0] - u;
        err[1] = (double)obs[1] - (pc[1] * invz * c.fy + c.cy);
        err[2] = (double)u_right - (u - c.bf * invz);
    }
}
// chi2(): _error.dot(information() * _error) with information = inv_sigma2 * I
LBA_HD double lba_chi2(const double *err, double info)
{
    return err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2]);
}
// isDepthPositive(): (v1->estimate().map(v2->estimate()))(2) > 0.0
LBA_HD bool lba_depth_positive(const LbaSe3 &T, const double *xw)
{
    double pc[3];
    se3_map(T, xw, pc);
    return pc[2] > 0.0;
}
// An edge's robust kernel: none, RobustKernelHuber with LocalBundleAdjustment's deltas (sqrt(5.991) / sqrt(7.815) held as floats,
// :569-570) or with BundleAdjustment's (sqrt(5.99) / sqrt(7.815), :85-86)
#define LBA_KERNEL_NONE 0
#define LBA_KERNEL_LBA 1
#define LBA_KERNEL_BA 2
LBA_HD double lba_huber_delta(bool stereo, int kernel)
{
    return stereo ? (double)(float)sqrt(7.815) : kernel == LBA_KERNEL_BA ? (double)(float)sqrt(5.99) : (double)(float)sqrt(5.991);
}
LBA_HD double lba_chi2_threshold(bool stereo) { return stereo ? 7.815 : 5.991; }                                           // :680, :696
// an active edge's term of activeRobustChi2 (sparse_optimizer.cpp:100-117)
LBA_HD double lba_edge_robust_chi2(const double *err, double info, bool stereo, int robust)
{
    const double c2 = lba_chi2(err, info);
    if (!robust) return c2;
    double rho0, rho1;
    huber(c2, lba_huber_delta(stereo, robust), rho0, rho1);
    return rho0;
}

// linearizeOplus + constructQuadraticForm of one edge at T and xw, with the stored error err: blk[LBA_NBLK].  The point part is
// always formed (a point is never fixed); the pose part and Hpl only for a free key frame (else they are zero).  A monocular edge
// carries a zero third row, so both kinds add three terms.  robust is an LBA_KERNEL_*.
LBA_HD void lba_edge_blocks(const LbaSe3 &T, const LbaCam &c, const double *xw, const double *err, double info, bool stereo, int robust,
                            bool kf_free, double *blk)
{
    double pc[3], R[9], A[3][3], B[3][6];
    se3_map(T, xw, pc);
    quat_to_R(T, R);
    const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z;
    if (!stereo) {
        // _jacobianOplusXi = -1./z * tmp * R with tmp = [fx 0 -x/z*fx; 0 fy -y/z*fy] (.cpp:115-124)
        const double s = -1. / z;
        const double t00 = s * c.fx, t02 = s * (-x / z * c.fx), t11 = s * c.fy, t12 = s * (-y / z * c.fy);
        for (int k = 0; k < 3; k++) {
            A[0][k] = t00 * R[k] + t02 * R[6 + k];
            A[1][k] = t11 * R[3 + k] + t12 * R[6 + k];
            A[2][k] = 0;
        }
    } else {
        for (int k = 0; k < 3; k++) {                       // .cpp:202-212
            A[0][k] = -c.fx * R[k] / z + c.fx * x * R[6 + k] / z_2;
            A[1][k] = -c.fy * R[3 + k] / z + c.fy * y * R[6 + k] / z_2;
            A[2][k] = A[0][k] - c.bf * R[6 + k] / z_2;
        }
    }
    B[0][0] = x * y / z_2 * c.fx; B[0][1] = -(1 + (x * x / z_2)) * c.fx; B[0][2] = y / z * c.fx;
    B[0][3] = -1. / z * c.fx; B[0][4] = 0; B[0][5] = x / z_2 * c.fx;
    B[1][0] = (1 + y * y / z_2) * c.fy; B[1][1] = -x * y / z_2 * c.fy; B[1][2] = -x / z * c.fy;
    B[1][3] = 0; B[1][4] = -1. / z * c.fy; B[1][5] = y / z_2 * c.fy;
    if (stereo) {
        B[2][0] = B[0][0] - c.bf * y / z_2; B[2][1] = B[0][1] + c.bf * x / z_2; B[2][2] = B[0][2];
        B[2][3] = B[0][3]; B[2][4] = 0; B[2][5] = B[0][5] - c.bf / z_2;
    } else {
        for (int k = 0; k < 6; k++) B[2][k] = 0;
    }
    double w = 1.;
    if (robust) {
        double rho0;
        huber(lba_chi2(err, info), lba_huber_delta(stereo, robust), rho0, w);
    }
    const double wi = w * info;                              // weightedOmega = rho' * Omega
    const double r0 = -(info * err[0]) * w, r1 = -(info * err[1]) * w, r2 = -(info * err[2]) * w;      // omega_r (*= rho')
    int u = LBA_HLL;
    for (int a = 0; a < 3; a++) {
        blk[LBA_BL + a] = A[0][a] * r0 + A[1][a] * r1 + A[2][a] * r2;
        const double w0 = A[0][a] * wi, w1 = A[1][a] * wi, w2 = A[2][a] * wi;
        for (int b = a; b < 3; b++, u++) blk[u] = w0 * A[0][b] + w1 * A[1][b] + w2 * A[2][b];
    }
    u = LBA_HPP;
    for (int a = 0; a < 6; a++) {
        const double w0 = B[0][a] * wi, w1 = B[1][a] * wi, w2 = B[2][a] * wi;
        blk[LBA_BP + a] = kf_free ? B[0][a] * r0 + B[1][a] * r1 + B[2][a] * r2 : 0.;
        for (int b = a; b < 6; b++, u++) blk[u] = kf_free ? w0 * B[0][b] + w1 * B[1][b] + w2 * B[2][b] : 0.;
        for (int b = 0; b < 3; b++) blk[LBA_HPL + 3 * a + b] = kf_free ? w0 * A[0][b] + w1 * A[1][b] + w2 * A[2][b] : 0.;
    }
}

// Dinv = (Hll + lambda I)^-1 (block_solver.hpp:389; Eigen's 3 x 3 inverse: cofactors over the determinant) and Dinv b_l (:391-395).
// Hll is the upper triangle (00 01 02 11 12 22); Dinv comes back as a full row-major matrix
LBA_HD void lba_point_dinv(const double *Hll, const double *bl, double lambda, double *Dinv, double *Db)
{
    const double m00 = Hll[0] + lambda, m01 = Hll[1], m02 = Hll[2], m11 = Hll[3] + lambda, m12 = Hll[4], m22 = Hll[5] + lambda;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double invdet = 1. / (m00 * c00 + m01 * c01 + m02 * c02);
    Dinv[0] = c00 * invdet; Dinv[1] = Dinv[3] = c01 * invdet; Dinv[2] = Dinv[6] = c02 * invdet;
    Dinv[4] = c11 * invdet; Dinv[5] = Dinv[7] = c12 * invdet; Dinv[8] = c22 * invdet;
    for (int i = 0; i < 3; i++) Db[i] = Dinv[3 * i] * bl[0] + Dinv[3 * i + 1] * bl[1] + Dinv[3 * i + 2] * bl[2];
}
// BDinv = Bi * Dinv (:407): W is an edge's Hpl (6 x 3), Y = W Dinv
LBA_HD void lba_mul_WD(const double *W, const double *Dinv, double *Y)
{
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 3; b++) Y[3 * a + b] = W[3 * a] * Dinv[b] + W[3 * a + 1] * Dinv[3 + b] + W[3 * a + 2] * Dinv[6 + b];
}
// M (6 x 6, row-major) = Y W2^T, the term BDinv * Bj->transpose() of :429
LBA_HD void lba_mul_YWt(const double *Y, const double *W2, double *M)
{
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) M[6 * a + b] = Y[3 * a] * W2[3 * b] + Y[3 * a + 1] * W2[3 * b + 1] + Y[3 * a + 2] * W2[3 * b + 2];
}
// v (6) = W d, the term (*Bi) * db of :413
LBA_HD void lba_mul_Wd(const double *W, const double *d, double *v)
{
    for (int a = 0; a < 6; a++) v[a] = W[3 * a] * d[0] + W[3 * a + 1] * d[1] + W[3 * a + 2] * d[2];
}
// cl -= W^T xp, one edge's term of _HplCCS->rightMultiply(cl, -xp) (:468-477)
LBA_HD void lba_sub_Wtx(const double *W, const double *xp, double *cl)
{
    for (int b = 0; b < 3; b++) {
        double s = 0;
        for (int a = 0; a < 6; a++) s += W[3 * a + b] * xp[a];
        cl[b] -= s;
    }
}
