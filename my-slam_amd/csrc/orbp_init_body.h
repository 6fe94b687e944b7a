// orbp_init_body.h -- the arithmetic of the monocular Initializer (src/Initializer.cc of WChen09/My-SLAM), one text for the host
// solver (orbp_init.cc, plain C++) and for the kernels (orbm_init.hip): init_normalize() is Normalize (:749-795), init_fill_h_rows /
// init_fill_f_row + init_null_vector + init_finish_h / init_finish_f are ComputeH21 (:226-266) / ComputeF21 (:268-303) with the
// products around them (:160-161, :212), init_check_h_one / init_check_f_one are one match of CheckHomography (:337-385) /
// CheckFundamental (:413-465), init_motions_f is DecomposeE (:909-929) with ReconstructF's four candidates (:479-497),
// init_motions_h the eight Faugeras motions of ReconstructH (:584-688), init_check_rt_one one match of CheckRT (:830-894) with
// Triangulate (:734-747).
//
// Host and device agree byte for byte because the body uses only + - * / sqrt on float and double (correctly rounded on both
// sides; the build's -ffp-contract=off keeps the compilers from fusing them) and every sum in one written order.  Nothing here
// allocates: everything that is indexed at run time (the Jacobi's matrices, the column norms, their order) lives in an InitWork
// the caller provides: the stack on the host, a wave-private piece of LDS in the kernel.
//
// What OpenCV 3.1.0 does inside cv::SVDecomp, cv::invert, cv::determinant, cv::gemm and the MatExpr scalings on CV_32F matrices is
// not pinned:
//   null vector    vt.row(8): one-sided (Hestenes) Jacobi in double on the float entries, cyclic pairs (0,1)(0,2)..(7,8), a pair
//                  left alone once |p.q| <= 2^-52 |p| |q|, at most INIT_SVD_SWEEPS sweeps; the column of V that belongs to the
//                  first smallest column norm, rounded to float.  Its SIGN is whatever the sweeps leave.  The 8 x 9 matrix of
//                  ComputeF21 is padded with a zero row to 9 x 9: the ninth right singular vector (FULL_UV) is then the column of
//                  V whose norm goes to zero.
//   3 x 3 SVD      the same Jacobi; singular values descending in the stable order; U = the rotated columns over their norms, V
//                  the accumulated rotations, all rounded to float; a column of U whose singular value is exactly zero is the
//                  cross product of the other two (the third one only)
//   A * B          3 x 3 and 3 x 1 products: the small-matrix path of cv::gemm (orbm_internal.h gemm3): three float products
//                  summed in float, left to right; alpha and the C operand applied in double.  K.t() * F and u * W.t() carry a
//                  transposition flag into cv::gemm and leave that path: their three products are summed in double
//   inverse        the 3 x 3 branch of cv::invert: determinant and cofactors in double from the float entries, each cofactor
//                  times 1 / det rounded to float; a zero determinant gives the zero matrix
//   determinant    in double from the float entries
//   M / s, M *= s  convertTo's float kernel: element * (float)scale + 0.0f
//   x3D            (float)(v[i] / v[3]) from the unrounded singular vector, as csrc/orbm_tri_body.h does for LocalMapping.cc:339
// Degenerate minimal sets (collinear or repeated points) are outside the value contract; the flags are still 0 / 1.
#pragma once
#include <stdint.h>
#include "orbm_svd4_body.h"

#if defined(__HIPCC__)
#define INIT_HD __host__ __device__ __forceinline__
#define INIT_UNROLL _Pragma("unroll")
#else
#define INIT_HD static inline
#define INIT_UNROLL
#endif

#define INIT_SVD_SWEEPS 40
#define INIT_DBL_EPSILON 2.2204460492503131e-16
#define INIT_MODEL_H 0
#define INIT_MODEL_F 1

// CheckRT's verdict on one match: the line of Initializer.cc that decided it (orbm_init_rt_status of include/orbm.h)
#define INIT_RT_GOOD 0              // :888-893, cosParallax < 0.99998: counted, vbGood set
#define INIT_RT_GOOD_LOW_PARALLAX 1 // :888-890: counted, vP3D written, vbGood left false
#define INIT_RT_NOT_INLIER 2        // :832
#define INIT_RT_NOT_FINITE 3        // :841
#define INIT_RT_BEHIND1 4           // :857
#define INIT_RT_BEHIND2 5           // :863
#define INIT_RT_REPROJ1 6           // :874
#define INIT_RT_REPROJ2 7           // :885

// scratch of one solve; every array is indexed at run time, so none of it may end up in registers or private memory on the GPU
struct InitWork {
    double B[144];                      // the Jacobi's working matrix: 16 x 9 (H), 9 x 9 (F, last row zero) or 3 x 3
    double V[81];
    double w[9];                        // column norms
    int order[9];
};
struct InitCam { float fx, fy, cx, cy; };

INIT_HD double init_abs(double x) { return x < 0 ? -x : x; }

// One-sided (Hestenes) Jacobi on the m x n matrix in B (row-major): B <- B J, V <- J, the columns of B end up orthogonal
INIT_HD void init_jacobi(double *B, int m, int n, double *V)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j;
    for (int sweep = 0; sweep < INIT_SVD_SWEEPS; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double a = 0, b = 0, g = 0;
                for (int i = 0; i < m; i++) {
                    const double x = B[i * n + p], y = B[i * n + q];
                    a += x * x; b += y * y; g += x * y;
                }
                if (init_abs(g) <= INIT_DBL_EPSILON * __builtin_sqrt(a * b) || g == 0.0) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (init_abs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / __builtin_sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < m; i++) {
                    const double x = B[i * n + p], y = B[i * n + q];
                    B[i * n + p] = c * x - s * y;
                    B[i * n + q] = s * x + c * y;
                }
                for (int i = 0; i < n; i++) {
                    const double x = V[i * n + p], y = V[i * n + q];
                    V[i * n + p] = c * x - s * y;
                    V[i * n + q] = s * x + c * y;
                }
            }
        if (!rotated) break;
    }
}
INIT_HD void init_column_norms(const double *B, int m, int n, double *w)
{
    for (int j = 0; j < n; j++) {
        double s = 0;
        for (int i = 0; i < m; i++) s += B[i * n + j] * B[i * n + j];
        w[j] = __builtin_sqrt(s);
    }
}

// rows 2j and 2j+1 of ComputeH21's A (:239-257), the float entries as written
INIT_HD void init_fill_h_rows(double *B, int j, float u1, float v1, float u2, float v2)
{
    double *r0 = B + 18 * j, *r1 = r0 + 9;
    r0[0] = 0.0; r0[1] = 0.0; r0[2] = 0.0; r0[3] = (double)-u1; r0[4] = (double)-v1; r0[5] = -1.0;
    r0[6] = (double)(v2 * u1); r0[7] = (double)(v2 * v1); r0[8] = (double)v2;
    r1[0] = (double)u1; r1[1] = (double)v1; r1[2] = 1.0; r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0;
    r1[6] = (double)(-u2 * u1); r1[7] = (double)(-u2 * v1); r1[8] = (double)-u2;
}
// row j of ComputeF21's A (:281-289); init_zero_row(B, 8) pads it to 9 x 9
INIT_HD void init_fill_f_row(double *B, int j, float u1, float v1, float u2, float v2)
{
    double *r = B + 9 * j;
    r[0] = (double)(u2 * u1); r[1] = (double)(u2 * v1); r[2] = (double)u2; r[3] = (double)(v2 * u1); r[4] = (double)(v2 * v1);
    r[5] = (double)v2; r[6] = (double)u1; r[7] = (double)v1; r[8] = 1.0;
}
INIT_HD void init_zero_row(double *B, int j)
{
    for (int i = 0; i < 9; i++) B[9 * j + i] = 0.0;
}
// vt.row(8) of the m x 9 matrix in wk.B (m = 16 or 9)
INIT_HD void init_null_vector(InitWork &wk, int m, float (&v)[9])
{
    init_jacobi(wk.B, m, 9, wk.V);
    init_column_norms(wk.B, m, 9, wk.w);
    int j = 0;
    for (int k = 1; k < 9; k++)
        if (wk.w[k] < wk.w[j]) j = k;
    INIT_UNROLL
    for (int i = 0; i < 9; i++) v[i] = (float)wk.V[i * 9 + j];
}

// C = A B on 3 x 3 float matrices: cv::gemm's small-matrix path with alpha = 1, no C operand
INIT_HD void init_mul33(const float (&A)[9], const float (&B)[9], float (&C)[9])
{
    INIT_UNROLL
    for (int i = 0; i < 3; i++) {
        INIT_UNROLL
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    }
}
INIT_HD void init_transpose33(const float (&A)[9], float (&T)[9])
{
    INIT_UNROLL
    for (int i = 0; i < 3; i++) {
        INIT_UNROLL
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
    }
}
INIT_HD double init_det3(const float (&m)[9])
{
    return (double)m[0] * ((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) -
           (double)m[1] * ((double)m[3] * (double)m[8] - (double)m[5] * (double)m[6]) +
           (double)m[2] * ((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]);
}
INIT_HD void init_inv33(const float (&S)[9], float (&D)[9])
{
    double d = init_det3(S);
    if (d == 0.0) {
        INIT_UNROLL
        for (int i = 0; i < 9; i++) D[i] = 0.f;
        return;
    }
    d = 1.0 / d;
    D[0] = (float)(((double)S[4] * (double)S[8] - (double)S[5] * (double)S[7]) * d);
    D[1] = (float)(((double)S[2] * (double)S[7] - (double)S[1] * (double)S[8]) * d);
    D[2] = (float)(((double)S[1] * (double)S[5] - (double)S[2] * (double)S[4]) * d);
    D[3] = (float)(((double)S[5] * (double)S[6] - (double)S[3] * (double)S[8]) * d);
    D[4] = (float)(((double)S[0] * (double)S[8] - (double)S[2] * (double)S[6]) * d);
    D[5] = (float)(((double)S[2] * (double)S[3] - (double)S[0] * (double)S[5]) * d);
    D[6] = (float)(((double)S[3] * (double)S[7] - (double)S[4] * (double)S[6]) * d);
    D[7] = (float)(((double)S[1] * (double)S[6] - (double)S[0] * (double)S[7]) * d);
    D[8] = (float)(((double)S[0] * (double)S[4] - (double)S[1] * (double)S[3]) * d);
}

// M = U diag(w) Vt, w descending
INIT_HD void init_svd3(const float (&M)[9], InitWork &wk, float (&U)[9], float (&w)[3], float (&Vt)[9])
{
    INIT_UNROLL
    for (int i = 0; i < 9; i++) wk.B[i] = (double)M[i];
    init_jacobi(wk.B, 3, 3, wk.V);
    init_column_norms(wk.B, 3, 3, wk.w);
    // stable descending order: an insertion sort that moves an index only past strictly smaller values
    for (int j = 0; j < 3; j++) {
        int k = j;
        while (k > 0 && wk.w[j] > wk.w[wk.order[k - 1]]) { wk.order[k] = wk.order[k - 1]; k--; }
        wk.order[k] = j;
    }
    INIT_UNROLL
    for (int k = 0; k < 3; k++) {
        const int j = wk.order[k];
        const double wj = wk.w[j];
        w[k] = (float)wj;
        INIT_UNROLL
        for (int i = 0; i < 3; i++) {
            U[3 * i + k] = (float)(wj > 0 ? wk.B[3 * i + j] / wj : 0.0);
            Vt[3 * k + i] = (float)wk.V[3 * i + j];
        }
    }
    if (!(wk.w[wk.order[2]] > 0)) {
        U[2] = (float)((double)U[3] * (double)U[7] - (double)U[6] * (double)U[4]);
        U[5] = (float)((double)U[6] * (double)U[1] - (double)U[0] * (double)U[7]);
        U[8] = (float)((double)U[0] * (double)U[4] - (double)U[3] * (double)U[1]);
    }
}

// H21i = T2inv * Hn * T1 (:160) and H12i = H21i.inv() (:161) from Hn = vt.row(8).reshape(0, 3)
INIT_HD void init_finish_h(const float (&Hn)[9], const float (&T1)[9], const float (&T2inv)[9], float (&H21)[9], float (&H12)[9])
{
    float tmp[9];
    init_mul33(T2inv, Hn, tmp);
    init_mul33(tmp, T1, H21);
    init_inv33(H21, H12);
}
// F21i = T2t * Fn * T1 (:212), Fn = u * diag(w) * vt with w[2] = 0 (:296-302) from Fpre = vt.row(8).reshape(0, 3)
INIT_HD void init_finish_f(const float (&Fpre)[9], const float (&T1)[9], const float (&T2t)[9], InitWork &wk, float (&F21)[9])
{
    float U[9], w[3], Vt[9], tmp[9], Fn[9];
    init_svd3(Fpre, wk, U, w, Vt);
    const float D[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, 0.f};
    init_mul33(U, D, tmp);
    init_mul33(tmp, Vt, Fn);
    init_mul33(T2t, Fn, tmp);
    init_mul33(tmp, T1, F21);
}

// One match of CheckHomography (:339-384): the inlier flag; s1 / s2 = what :363 / :379 add to the score (0 where they add nothing)
INIT_HD bool init_check_h_one(const float (&H21)[9], const float (&H12)[9], float u1, float v1, float u2, float v2, float invSigmaSquare,
                              float &s1, float &s2)
{
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; s1 = 0.0f; }
    else s1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; s2 = 0.0f; }
    else s2 = th - chiSquare2;
    return bIn;
}
// One match of CheckFundamental (:415-464)
INIT_HD bool init_check_f_one(const float (&F)[9], float u1, float v1, float u2, float v2, float invSigmaSquare, float &s1, float &s2)
{
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; s1 = 0.0f; }
    else s1 = thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; s2 = 0.0f; }
    else s2 = thScore - chiSquare2;
    return bIn;
}
// invSigmaSquare = 1.0/(sigma*sigma) (:335, :411).  A chi-square that is NaN (a degenerate hypothesis) is not `> th`: the match
// stays an inlier and its term makes the score NaN, which never wins `currentScore>score`; the reference does the same
INIT_HD float init_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// Normalize (:749-795) over n keys (x, y pairs): pn[2n] and T (3 x 3).  Float sums in key order.  Host only (n is unbounded).
INIT_HD void init_normalize(const float *keys, int n, float *pn, float (&T)[9])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += keys[2 * i]; meanY += keys[2 * i + 1]; }
    meanX = meanX / (float)n; meanY = meanY / (float)n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) {
        pn[2 * i] = keys[2 * i] - meanX; pn[2 * i + 1] = keys[2 * i + 1] - meanY;
        meanDevX += __builtin_fabsf(pn[2 * i]); meanDevY += __builtin_fabsf(pn[2 * i + 1]);
    }
    meanDevX = meanDevX / (float)n; meanDevY = meanDevY / (float)n;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
    T[0] = sX; T[1] = 0.f; T[2] = -meanX * sX; T[3] = 0.f; T[4] = sY; T[5] = -meanY * sY; T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

INIT_HD void init_K(const InitCam &c, float (&K)[9])
{
    K[0] = c.fx; K[1] = 0.f; K[2] = c.cx; K[3] = 0.f; K[4] = c.fy; K[5] = c.cy; K[6] = 0.f; K[7] = 0.f; K[8] = 1.f;
}
// t / cv::norm(t)
INIT_HD void init_unit3(const float (&t)[3], float (&o)[3])
{
    const double nrm = __builtin_sqrt(tri_dot3(t[0], t[1], t[2], t[0], t[1], t[2]));
    const float sc = (float)(1.0 / nrm);
    INIT_UNROLL
    for (int i = 0; i < 3; i++) o[i] = t[i] * sc + 0.0f;
}
INIT_HD void init_store_motion(float *Rt, const float (&R)[9], const float (&t)[3], bool negate_t)
{
    INIT_UNROLL
    for (int i = 0; i < 9; i++) Rt[i] = R[i];
    INIT_UNROLL
    for (int i = 0; i < 3; i++) Rt[9 + i] = negate_t ? -t[i] : t[i];
}

// ReconstructF's four candidates (:479-497): E21 = K.t() * F21 * K, DecomposeE, then (R1, t) (R2, t) (R1, -t) (R2, -t) into Rt
// (12 floats each: R row-major, then t)
INIT_HD void init_motions_f(const float (&F21)[9], const InitCam &cam, InitWork &wk, float *Rt)
{
    float K[9], KtF[9], E[9], U[9], w[3], Vt[9];
    init_K(cam, K);
    INIT_UNROLL
    for (int i = 0; i < 3; i++) {
        INIT_UNROLL
        for (int j = 0; j < 3; j++)
            KtF[3 * i + j] = (float)(((double)K[i] * (double)F21[j] + (double)K[3 + i] * (double)F21[3 + j]) + (double)K[6 + i] * (double)F21[6 + j]);
    }
    init_mul33(KtF, K, E);
    init_svd3(E, wk, U, w, Vt);
    const float tc[3] = {U[2], U[5], U[8]};
    float t[3];
    init_unit3(tc, t);
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float uW[9], R1[9], R2[9];
    init_mul33(U, W, uW);
    init_mul33(uW, Vt, R1);
    if (init_det3(R1) < 0) {
        INIT_UNROLL
        for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    }
    INIT_UNROLL
    for (int i = 0; i < 3; i++) {
        INIT_UNROLL
        for (int j = 0; j < 3; j++)
            uW[3 * i + j] = (float)(((double)U[3 * i] * (double)W[3 * j] + (double)U[3 * i + 1] * (double)W[3 * j + 1]) + (double)U[3 * i + 2] * (double)W[3 * j + 2]);
    }
    init_mul33(uW, Vt, R2);
    if (init_det3(R2) < 0) {
        INIT_UNROLL
        for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    }
    init_store_motion(Rt, R1, t, false);
    init_store_motion(Rt + 12, R2, t, false);
    init_store_motion(Rt + 24, R1, t, true);
    init_store_motion(Rt + 36, R2, t, true);
}

// one of ReconstructH's motions: R = s * U * Rp * Vt, t = U * tp / norm
INIT_HD void init_h_motion(const float (&U)[9], const float (&Vt)[9], float s, const float (&Rp)[9], const float (&tp)[3], float *Rt)
{
    float sURp[9], R[9];
    INIT_UNROLL
    for (int i = 0; i < 3; i++) {
        INIT_UNROLL
        for (int j = 0; j < 3; j++) {
            const float t0 = U[3 * i] * Rp[j] + U[3 * i + 1] * Rp[3 + j] + U[3 * i + 2] * Rp[6 + j];
            sURp[3 * i + j] = (float)((double)t0 * (double)s);
        }
    }
    init_mul33(sURp, Vt, R);
    float t[3], tn[3];
    INIT_UNROLL
    for (int i = 0; i < 3; i++) t[i] = U[3 * i] * tp[0] + U[3 * i + 1] * tp[1] + U[3 * i + 2] * tp[2];
    init_unit3(t, tn);
    init_store_motion(Rt, R, tn, false);
}
// The eight motions of ReconstructH (:584-686) into Rt (12 floats each); false at the `d1/d2<1.00001 || d2/d3<1.00001` exit (:597)
INIT_HD bool init_motions_h(const float (&H21)[9], const InitCam &cam, InitWork &wk, float *Rt)
{
    float K[9], invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    init_K(cam, K);
    init_inv33(K, invK);
    init_mul33(invK, H21, tmp);
    init_mul33(tmp, K, A);
    init_svd3(A, wk, U, w, Vt);
    const float s = (float)(init_det3(U) * init_det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = (float)__builtin_sqrt((double)((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)));
    const float aux3 = (float)__builtin_sqrt((double)((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3)));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    // case d' = d2
    const float aux_stheta = (float)__builtin_sqrt((double)((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    INIT_UNROLL
    for (int i = 0; i < 4; i++) {
        const float Rp[9] = {ctheta, 0.f, -stheta[i], 0.f, 1.f, 0.f, stheta[i], 0.f, ctheta};
        const float sc = d1 - d3;
        const float tp[3] = {x1[i] * sc + 0.0f, 0.f * sc + 0.0f, -x3[i] * sc + 0.0f};
        init_h_motion(U, Vt, s, Rp, tp, Rt + 12 * i);
    }
    // case d' = -d2
    const float aux_sphi = (float)__builtin_sqrt((double)((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    INIT_UNROLL
    for (int i = 0; i < 4; i++) {
        const float Rp[9] = {cphi, 0.f, sphi[i], 0.f, -1.f, 0.f, sphi[i], 0.f, -cphi};
        const float sc = d1 + d3;
        const float tp[3] = {x1[i] * sc + 0.0f, 0.f * sc + 0.0f, x3[i] * sc + 0.0f};
        init_h_motion(U, Vt, s, Rp, tp, Rt + 12 * (4 + i));
    }
    return true;
}

// what CheckRT prepares once per motion (:814-826): P2 = K * [R | t] (3 x 4) and O2 = -R.t() * t
struct InitMotion { float R[9], t[3], P2[12], O2[3]; };
INIT_HD void init_motion_prepare(const InitCam &cam, const float *Rt, InitMotion &m)
{
    float K[9];
    init_K(cam, K);
    INIT_UNROLL
    for (int i = 0; i < 9; i++) m.R[i] = Rt[i];
    INIT_UNROLL
    for (int i = 0; i < 3; i++) m.t[i] = Rt[9 + i];
    INIT_UNROLL
    for (int i = 0; i < 3; i++) {
        INIT_UNROLL
        for (int j = 0; j < 3; j++) m.P2[4 * i + j] = K[3 * i] * m.R[j] + K[3 * i + 1] * m.R[3 + j] + K[3 * i + 2] * m.R[6 + j];
        m.P2[4 * i + 3] = K[3 * i] * m.t[0] + K[3 * i + 1] * m.t[1] + K[3 * i + 2] * m.t[2];
    }
    INIT_UNROLL
    for (int k = 0; k < 3; k++) {
        const float t0 = m.R[k] * m.t[0] + m.R[3 + k] * m.t[1] + m.R[6 + k] * m.t[2];
        m.O2[k] = (float)((double)t0 * -1.0 + 0.0);
    }
}
// One inlier match of CheckRT (:835-893): its verdict, cosParallax and p3dC1 (X; zero unless the verdict is one of the two GOOD)
INIT_HD int init_check_rt_one(const InitCam &cam, const InitMotion &m, float u1, float v1, float u2, float v2, float th2, float (&X)[3],
                              float &cosParallax)
{
    cosParallax = 0.f;
    X[0] = X[1] = X[2] = 0.f;
    // Triangulate (:736-746); P1 = K [I | 0]; column j of A = element j of the four rows
    const float *P2 = m.P2;
    const D4 c0 = {(double)tri_arow(u1, 0.f, cam.fx), (double)tri_arow(v1, 0.f, 0.f), (double)tri_arow(u2, P2[8], P2[0]), (double)tri_arow(v2, P2[8], P2[4])};
    const D4 c1 = {(double)tri_arow(u1, 0.f, 0.f), (double)tri_arow(v1, 0.f, cam.fy), (double)tri_arow(u2, P2[9], P2[1]), (double)tri_arow(v2, P2[9], P2[5])};
    const D4 c2 = {(double)tri_arow(u1, 1.f, cam.cx), (double)tri_arow(v1, 1.f, cam.cy), (double)tri_arow(u2, P2[10], P2[2]), (double)tri_arow(v2, P2[10], P2[6])};
    const D4 c3 = {(double)tri_arow(u1, 0.f, 0.f), (double)tri_arow(v1, 0.f, 0.f), (double)tri_arow(u2, P2[11], P2[3]), (double)tri_arow(v2, P2[11], P2[7])};
    const D4 v = smallest_right_singular_vector(c0, c1, c2, c3);
    const float x = (float)(v.a / v.d), y = (float)(v.b / v.d), z = (float)(v.c / v.d);
    if (!__builtin_isfinite(x) || !__builtin_isfinite(y) || !__builtin_isfinite(z)) return INIT_RT_NOT_FINITE;      // :841
    // Check parallax :848-854 (O1 = 0)
    const float n1x = x - 0.f, n1y = y - 0.f, n1z = z - 0.f;
    const float dist1 = (float)__builtin_sqrt(tri_dot3(n1x, n1y, n1z, n1x, n1y, n1z));
    const float n2x = x - m.O2[0], n2y = y - m.O2[1], n2z = z - m.O2[2];
    const float dist2 = (float)__builtin_sqrt(tri_dot3(n2x, n2y, n2z, n2x, n2y, n2z));
    const float cosp = (float)(tri_dot3(n1x, n1y, n1z, n2x, n2y, n2z) / (double)(dist1 * dist2));
    cosParallax = cosp;
    if (z <= 0 && (double)cosp < 0.99998) return INIT_RT_BEHIND1;                                                   // :857
    // p3dC2 = R * p3dC1 + t :861
    const float x2 = (float)((double)(m.R[0] * x + m.R[1] * y + m.R[2] * z) + (double)m.t[0]);
    const float y2 = (float)((double)(m.R[3] * x + m.R[4] * y + m.R[5] * z) + (double)m.t[1]);
    const float z2 = (float)((double)(m.R[6] * x + m.R[7] * y + m.R[8] * z) + (double)m.t[2]);
    if (z2 <= 0 && (double)cosp < 0.99998) return INIT_RT_BEHIND2;                                                  // :863
    const float invZ1 = (float)(1.0 / (double)z);
    const float im1x = cam.fx * x * invZ1 + cam.cx, im1y = cam.fy * y * invZ1 + cam.cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return INIT_RT_REPROJ1;                                                                 // :874
    const float invZ2 = (float)(1.0 / (double)z2);
    const float im2x = cam.fx * x2 * invZ2 + cam.cx, im2y = cam.fy * y2 * invZ2 + cam.cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return INIT_RT_REPROJ2;                                                                 // :885
    X[0] = x; X[1] = y; X[2] = z;
    return (double)cosp < 0.99998 ? INIT_RT_GOOD : INIT_RT_GOOD_LOW_PARALLAX;                                       // :892
}
