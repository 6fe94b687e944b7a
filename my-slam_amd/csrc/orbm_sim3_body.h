// orbm_sim3_body.h -- the arithmetic of one Sim3Solver hypothesis (src/Sim3Solver.cc:226-403 of WChen09/My-SLAM), one text for the
// host solver (orbp_sim3.cc, plain C++) and for the kernel (orbm_sim3.hip): sim3_from_triple() is Sim3Solver::ComputeSim3 on the
// three sampled point pairs, sim3_check_one() is one correspondence of CheckInliers / Project, sim3_max_error() is the threshold
// as the reference's std::vector<size_t> holds it.
//
// Host and device agree byte for byte because the body uses only + - * / sqrt on float and double (correctly rounded on both
// sides; the build's -ffp-contract=off keeps the compilers from fusing them) and brings its own atan2 / sin / cos
// (sim3_atan2_pos, sim3_sincos: fdlibm's reductions and minimax polynomials evaluated with those operations alone, < 2 ulp).
//
// What OpenCV 3.1.0 does inside cv::eigen, cv::Rodrigues, cv::reduce and the MatExpr scalings is not pinned:
//   centroid       float sum of the three columns, divided by 3.0f
//   M, P3, R*x+t   the small-matrix gemm of orbm_internal.h's gemm3: three float products summed in float, left to right;
//                  alpha and the C operand applied in double
//   eigenvector    cyclic Jacobi in double on the float N, pairs (0,1)(0,2)(0,3)(1,2)(1,3)(2,3), a pair left alone once
//                  |a_pq| <= 1e-17 ||N||_F, at most 16 sweeps; the first largest diagonal entry wins; rounded to float
//   norm(vec)      the three squares and their sum in double
//   2*ang*vec/norm one double factor (2 ang) / norm per component, rounded to float
//   Rodrigues      in double from the float vector: R = c I + (1 - c) r r^T + s [r]x with r = vec / theta, rounded to float;
//                  the identity below theta = 2^-52
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SIM3_HD __host__ __device__ __forceinline__
#else
#define SIM3_HD static inline
#endif

#define SIM3_JACOBI_SWEEPS 16
#define SIM3_JACOBI_TOL 1e-17

struct Sim3Cam { float fx, fy, cx, cy; };
// one hypothesis: what ComputeSim3 leaves in ms12i, mR12i, mt12i, mT12i and mT21i (the 3x4 tops, row-major)
struct Sim3Hyp { float s, R[9], t[3], T12[12], T21[12]; };

SIM3_HD double sim3_abs(double x) { return x < 0 ? -x : x; }

// atan(x) for x >= 0: fdlibm's s_atan.c (four breakpoints, odd / even split of the degree-11 polynomial in x^2)
SIM3_HD double sim3_atan_pos(double x)
{
    double hi = 0, lo = 0;
    bool red = true;
    if (x < 0.4375) red = false;
    else if (x < 0.6875) { hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; x = (2.0 * x - 1.0) / (2.0 + x); }
    else if (x < 1.1875) { hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; x = (x - 1.0) / (x + 1.0); }
    else if (x < 2.4375) { hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17; x = (x - 1.5) / (1.0 + 1.5 * x); }
    else { hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17; x = -1.0 / x; }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (!red) return x - x * (s1 + s2);
    return hi - ((x * (s1 + s2) - lo) - x);
}
// atan2(y, x) for y >= 0 (y is a norm): e_atan2.c without the cases y < 0
SIM3_HD double sim3_atan2_pos(double y, double x)
{
    if (x == 0) return y == 0 ? 0.0 : 1.57079632679489655800e+00;
    const double z = sim3_atan_pos(sim3_abs(y / x));
    if (x > 0) return z;
    return 3.1415926535897931160e+00 - (z - 1.2246467991473531772e-16);
}
// sin and cos of x in [0, 8]: k = nearest multiple of pi/2, two-term Cody-Waite reduction (k <= 5: k * pio2_1 is exact), then
// k_sin.c / k_cos.c on |r| <= pi/4
SIM3_HD void sim3_sincos(double x, double &sn, double &cs)
{
    const int k = (int)(x * 6.36619772367581382433e-01 + 0.5);
    const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    const double z = r * r;
    const double ps = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 +
                      z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    const double sr = r + (z * r) * (-1.66666666666666324348e-01 + z * ps);
    const double pc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double cr = 1.0 - (0.5 * z - z * pc);
    const int q = k & 3;
    sn = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
    cs = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

// one rotation of the cyclic Jacobi method on the symmetric A (full storage), accumulated in the columns of V
template <int P, int Q>
SIM3_HD bool sim3_jacobi_pair(double (&A)[4][4], double (&V)[4][4], double tol)
{
    const double apq = A[P][Q];
    if (!(sim3_abs(apq) > tol)) return false;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0 ? -1.0 : 1.0) / (sim3_abs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    // written out index by index: every element stays a scalar the compiler keeps in a register
#define SIM3_ROT(x, y) { const double x_ = (x), y_ = (y); (x) = c * x_ - s * y_; (y) = s * x_ + c * y_; }
    SIM3_ROT(A[0][P], A[0][Q]) SIM3_ROT(A[1][P], A[1][Q]) SIM3_ROT(A[2][P], A[2][Q]) SIM3_ROT(A[3][P], A[3][Q])     // A <- A J
    SIM3_ROT(A[P][0], A[Q][0]) SIM3_ROT(A[P][1], A[Q][1]) SIM3_ROT(A[P][2], A[Q][2]) SIM3_ROT(A[P][3], A[Q][3])     // A <- J^T A
    SIM3_ROT(V[0][P], V[0][Q]) SIM3_ROT(V[1][P], V[1][Q]) SIM3_ROT(V[2][P], V[2][Q]) SIM3_ROT(V[3][P], V[3][Q])     // V <- V J
#undef SIM3_ROT
    return true;
}
// the eigenvector of the largest eigenvalue of the symmetric float matrix with upper triangle n[10] (N11 N12 N13 N14 N22 N23 N24
// N33 N34 N44), as cv::eigen's evec.row(0), rounded to float; its sign is whatever the sweeps leave
SIM3_HD void sim3_top_eigenvector(const float (&n)[10], float (&q)[4])
{
    double A[4][4] = {{n[0], n[1], n[2], n[3]}, {n[1], n[4], n[5], n[6]}, {n[2], n[5], n[7], n[8]}, {n[3], n[6], n[8], n[9]}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    double fro = 0;
    for (int i = 0; i < 10; i++) fro += (double)n[i] * (double)n[i] * ((i == 0 || i == 4 || i == 7 || i == 9) ? 1.0 : 2.0);
    const double tol = SIM3_JACOBI_TOL * __builtin_sqrt(fro);
    for (int sweep = 0; sweep < SIM3_JACOBI_SWEEPS; sweep++) {
        bool any = sim3_jacobi_pair<0, 1>(A, V, tol);
        any |= sim3_jacobi_pair<0, 2>(A, V, tol);
        any |= sim3_jacobi_pair<0, 3>(A, V, tol);
        any |= sim3_jacobi_pair<1, 2>(A, V, tol);
        any |= sim3_jacobi_pair<1, 3>(A, V, tol);
        any |= sim3_jacobi_pair<2, 3>(A, V, tol);
        if (!any) break;
    }
    // the column of the first largest diagonal entry, picked value by value (never by address)
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2], d3 = A[3][3];
    const bool b1 = d1 > d0;
    const double m1 = b1 ? d1 : d0;
    const bool b2 = d2 > m1;
    const double m2 = b2 ? d2 : m1;
    const bool b3 = d3 > m2;
    double e[4];
#define SIM3_PICK(k) { const double c0 = V[k][0], c1 = V[k][1], c2 = V[k][2], c3 = V[k][3]; const double t1 = b1 ? c1 : c0, t2 = b2 ? c2 : t1; e[k] = b3 ? c3 : t2; }
    SIM3_PICK(0) SIM3_PICK(1) SIM3_PICK(2) SIM3_PICK(3)
#undef SIM3_PICK
    const double e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
    q[0] = (float)e0; q[1] = (float)e1; q[2] = (float)e2; q[3] = (float)e3;
}

// cv::gemm's small-matrix path on three terms (orbm_internal.h gemm3)
SIM3_HD float sim3_dot3f(float a0, float a1, float a2, float b0, float b1, float b2) { return a0 * b0 + a1 * b1 + a2 * b2; }

// mT12i = [s R | t] and mT21i = [(1/s) R^T | -(1/s) R^T t] (:320-336) from s, R, t
SIM3_HD void sim3_transforms(Sim3Hyp &h)
{
    const double inv_s = 1.0 / (double)h.s;
    float sRinv[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            h.T12[4 * i + j] = h.s * h.R[3 * i + j];
            sRinv[3 * i + j] = (float)(inv_s * (double)h.R[3 * j + i]);
            h.T21[4 * i + j] = sRinv[3 * i + j];
        }
    for (int i = 0; i < 3; i++) {
        h.T12[4 * i + 3] = h.t[i];
        h.T21[4 * i + 3] = -sim3_dot3f(sRinv[3 * i], sRinv[3 * i + 1], sRinv[3 * i + 2], h.t[0], h.t[1], h.t[2]);
    }
}

// Sim3Solver::ComputeSim3 (:226-337).  P1[k] / P2[k]: the k-th sampled point in camera 1 / camera 2 (the columns of P3Dc1i / P3Dc2i)
SIM3_HD void sim3_from_triple(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, Sim3Hyp &h)
{
    // Step 1: centroids and relative coordinates.  Pr[i][k]: coordinate i of point k
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
    for (int i = 0; i < 3; i++) {
        O1[i] = (P1[0][i] + P1[1][i] + P1[2][i]) / 3.0f;
        O2[i] = (P2[0][i] + P2[1][i] + P2[2][i]) / 3.0f;
        for (int k = 0; k < 3; k++) { Pr1[i][k] = P1[k][i] - O1[i]; Pr2[i][k] = P2[k][i] - O2[i]; }
    }
    // Step 2: M = Pr2 Pr1^T
    float M[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = sim3_dot3f(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
    // Step 3: N (double variables assigned from float expressions, stored into a float matrix: the float values)
    const float n[10] = {M[0][0] + M[1][1] + M[2][2], M[1][2] - M[2][1], M[2][0] - M[0][2], M[0][1] - M[1][0],
                         M[0][0] - M[1][1] - M[2][2], M[0][1] + M[1][0], M[2][0] + M[0][2],
                         -M[0][0] + M[1][1] - M[2][2], M[1][2] + M[2][1],
                         -M[0][0] - M[1][1] + M[2][2]};
    // Step 4: eigenvector of the highest eigenvalue, angle-axis
    float q[4];
    sim3_top_eigenvector(n, q);
    const double nrm = __builtin_sqrt((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2] + (double)q[3] * (double)q[3]);
    const double ang = sim3_atan2_pos(nrm, (double)q[0]);
    const double f = (2.0 * ang) / nrm;
    const float vec[3] = {(float)((double)q[1] * f), (float)((double)q[2] * f), (float)((double)q[3] * f)};
    // cv::Rodrigues
    {
        double rx = vec[0], ry = vec[1], rz = vec[2];
        const double theta = __builtin_sqrt(rx * rx + ry * ry + rz * rz);
        if (theta < 2.220446049250313e-16) {
            for (int i = 0; i < 9; i++) h.R[i] = (i % 4 == 0) ? 1.f : 0.f;
        } else {
            double sn, cs;
            sim3_sincos(theta, sn, cs);
            const double c1 = 1.0 - cs, it = 1.0 / theta;
            rx *= it; ry *= it; rz *= it;
            h.R[0] = (float)(cs + c1 * rx * rx); h.R[1] = (float)(c1 * rx * ry - sn * rz); h.R[2] = (float)(c1 * rx * rz + sn * ry);
            h.R[3] = (float)(c1 * rx * ry + sn * rz); h.R[4] = (float)(cs + c1 * ry * ry); h.R[5] = (float)(c1 * ry * rz - sn * rx);
            h.R[6] = (float)(c1 * rx * rz - sn * ry); h.R[7] = (float)(c1 * ry * rz + sn * rx); h.R[8] = (float)(cs + c1 * rz * rz);
        }
    }
    // Step 5: P3 = R Pr2;  Step 6: scale
    if (!fix_scale) {
        double nom = 0, den = 0;
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) {
                const float p3 = sim3_dot3f(h.R[3 * i], h.R[3 * i + 1], h.R[3 * i + 2], Pr2[0][k], Pr2[1][k], Pr2[2][k]);
                nom += (double)Pr1[i][k] * (double)p3;
                den += (double)(p3 * p3);
            }
        h.s = (float)(nom / den);
    } else
        h.s = 1.0f;
    // Step 7: t = O1 - s R O2, one gemm(R, O2, -s, O1, 1)
    for (int i = 0; i < 3; i++) {
        const float t0 = sim3_dot3f(h.R[3 * i], h.R[3 * i + 1], h.R[3 * i + 2], O2[0], O2[1], O2[2]);
        h.t[i] = (float)((double)t0 * (-(double)h.s) + (double)O1[i]);
    }
    sim3_transforms(h);
}

// mvnMaxError1/2 are std::vector<size_t> (include/Sim3Solver.h:78-79): 9.210 * sigma2 is truncated to an integer, and the
// comparison in CheckInliers converts it to float
SIM3_HD float sim3_max_error(float sigma2)
{
    const double v = 9.210 * (double)sigma2;
    return v >= 0 && v < 1.8e19 ? (float)(unsigned long long)v : 0.0f;
}

// Project (:382-403) of one point: (fx x / z + cx, fy y / z + cy) of T x, T a row-major 3x4, or of x itself (FromCameraToImage)
SIM3_HD void sim3_project(const float *T, const float *x, const Sim3Cam &K, float &u, float &v)
{
    float X = x[0], Y = x[1], Z = x[2];
    if (T) {
        X = (float)((double)sim3_dot3f(T[0], T[1], T[2], x[0], x[1], x[2]) + (double)T[3]);
        Y = (float)((double)sim3_dot3f(T[4], T[5], T[6], x[0], x[1], x[2]) + (double)T[7]);
        Z = (float)((double)sim3_dot3f(T[8], T[9], T[10], x[0], x[1], x[2]) + (double)T[11]);
    }
    const float invz = 1 / Z;
    const float px = X * invz, py = Y * invz;
    u = K.fx * px + K.cx; v = K.fy * py + K.cy;
}
// one correspondence of CheckInliers (:340-364): x1 / x2 = the point in camera 1 / 2
SIM3_HD bool sim3_check_one(const Sim3Hyp &h, const float *x1, const float *x2, const Sim3Cam &K1, const Sim3Cam &K2,
                            float max_err1, float max_err2, float *err1_out = nullptr, float *err2_out = nullptr)
{
    float u11, v11, u22, v22, u21, v21, u12, v12;
    sim3_project(nullptr, x1, K1, u11, v11);     // mvP1im1
    sim3_project(nullptr, x2, K2, u22, v22);     // mvP2im2
    sim3_project(h.T12, x2, K1, u21, v21);       // vP2im1
    sim3_project(h.T21, x1, K2, u12, v12);       // vP1im2
    const float d1x = u11 - u21, d1y = v11 - v21, d2x = u12 - u22, d2y = v12 - v22;
    const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
    const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
    if (err1_out) *err1_out = err1;
    if (err2_out) *err2_out = err2;
    return err1 < max_err1 && err2 < max_err2;
}
