// orbp_se3_body.h -- the quaternion / SE3 group of g2o::SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h, on Eigen's Quaterniond) and
// RobustKernelHuber, one text for the host solvers and for the kernels.  orbp_lba_body.h (LBA, BA) and orbp_pose_body.h
// (PoseOptimization) build on Se3; orbp_sim3opt_body.h (OptimizeSim3, and through it orbp_eg_body.h) builds its Sim3 on Quat.
//
// Everything is fp64 and uses + - * / sqrt alone (the build's -ffp-contract=off keeps them unfused), except se3_exp, which calls
// sin and cos of the side it is compiled for.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SE3_HD __host__ __device__ __forceinline__
#else
#define SE3_HD static inline
#endif

struct Quat { double qx, qy, qz, qw; };             // Eigen's coefficient order
struct Se3 : Quat { double t0, t1, t2; };           // g2o::SE3Quat: a unit quaternion (w >= 0) and a translation

// Eigen's Quaterniond(Matrix3d) of a row-major R, the branch on the largest diagonal entry written out per case
SE3_HD void quat_from_R(const double *R, Quat &q)
{
    double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        tr = sqrt(tr + 1.0);
        q.qw = 0.5 * tr;
        tr = 0.5 / tr;
        q.qx = (R[7] - R[5]) * tr; q.qy = (R[2] - R[6]) * tr; q.qz = (R[3] - R[1]) * tr;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i ? R[4] : R[0])) i = 2;
        if (i == 0) {               // j = 1, k = 2
            tr = sqrt(R[0] - R[4] - R[8] + 1.0);
            q.qx = 0.5 * tr; tr = 0.5 / tr;
            q.qw = (R[7] - R[5]) * tr; q.qy = (R[3] + R[1]) * tr; q.qz = (R[6] + R[2]) * tr;
        } else if (i == 1) {        // j = 2, k = 0
            tr = sqrt(R[4] - R[8] - R[0] + 1.0);
            q.qy = 0.5 * tr; tr = 0.5 / tr;
            q.qw = (R[2] - R[6]) * tr; q.qz = (R[7] + R[5]) * tr; q.qx = (R[1] + R[3]) * tr;
        } else {                    // j = 0, k = 1
            tr = sqrt(R[8] - R[0] - R[4] + 1.0);
            q.qz = 0.5 * tr; tr = 0.5 / tr;
            q.qw = (R[3] - R[1]) * tr; q.qx = (R[2] + R[6]) * tr; q.qy = (R[5] + R[7]) * tr;
        }
    }
}
SE3_HD void quat_normalize(Quat &q)                 // SE3Quat::normalizeRotation (se3quat.h:280-285)
{
    if (q.qw < 0) { q.qw = -q.qw; q.qx = -q.qx; q.qy = -q.qy; q.qz = -q.qz; }
    const double n = sqrt(q.qw * q.qw + q.qx * q.qx + q.qy * q.qy + q.qz * q.qz);
    q.qw /= n; q.qx /= n; q.qy /= n; q.qz /= n;
}
SE3_HD void quat_mul(const Quat &a, const Quat &b, Quat &r)       // Eigen's Quaterniond * Quaterniond; r is neither a nor b
{
    r.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
    r.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
    r.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
    r.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
}
// Eigen's Quaterniond * Vector3d: v + w uv + q.vec x uv with uv = 2 q.vec x v (exact only for a unit quaternion)
SE3_HD void quat_rotate(const Quat &q, double v0, double v1, double v2, double &o0, double &o1, double &o2)
{
    double u0 = q.qy * v2 - q.qz * v1, u1 = q.qz * v0 - q.qx * v2, u2 = q.qx * v1 - q.qy * v0;
    u0 += u0; u1 += u1; u2 += u2;
    o0 = v0 + q.qw * u0 + (q.qy * u2 - q.qz * u1);
    o1 = v1 + q.qw * u1 + (q.qz * u0 - q.qx * u2);
    o2 = v2 + q.qw * u2 + (q.qx * u1 - q.qy * u0);
}
SE3_HD void quat_to_R(const Quat &q, double *R)     // Eigen's toRotationMatrix: nothing is normalised
{
    const double tx = 2 * q.qx, ty = 2 * q.qy, tz = 2 * q.qz;
    const double twx = tx * q.qw, twy = ty * q.qw, twz = tz * q.qw, txx = tx * q.qx, txy = ty * q.qx, txz = tz * q.qx;
    const double tyy = ty * q.qy, tyz = tz * q.qy, tzz = tz * q.qz;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
SE3_HD void se3_map(const Se3 &T, const double *x, double *o)     // se3quat.h:119-121; o is not x
{
    quat_rotate(T, x[0], x[1], x[2], o[0], o[1], o[2]);
    o[0] += T.t0; o[1] += T.t1; o[2] += T.t2;
}
// Converter::toSE3Quat (src/Converter.cc:37-46) of a row-major 4 x 4 float pose: SE3Quat(R, t) normalises
SE3_HD Se3 se3_from_Tcw(const float *T)
{
    double R[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
    Se3 S;
    quat_from_R(R, S);
    quat_normalize(S);
    S.t0 = (double)T[3]; S.t1 = (double)T[7]; S.t2 = (double)T[11];
    return S;
}
// Converter::toCvMat(SE3Quat) (src/Converter.cc:48-52): to_homogeneous_matrix cast to float
SE3_HD void se3_to_Tcw(const Se3 &S, float *T)
{
    double R[9];
    quat_to_R(S, R);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j];
    T[3] = (float)S.t0; T[7] = (float)S.t1; T[11] = (float)S.t2;
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}
// SE3Quat::exp (se3quat.h:223-257), omega first, then upsilon; pow(theta, 3) as two multiplications on both sides
SE3_HD Se3 se3_exp(const double *u)
{
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double O[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0) + O[i] + O2[i]; V[i] = R[i]; }
    } else {
        const double sn = sin(theta), cs = cos(theta);
        const double a = sn / theta, b = (1 - cs) / (theta * theta), c = (theta - sn) / (theta * theta * theta);
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0) + a * O[i] + b * O2[i]; V[i] = (i % 4 == 0) + b * O[i] + c * O2[i]; }
    }
    Se3 T;
    quat_from_R(R, T);
    quat_normalize(T);
    T.t0 = V[0] * u[3] + V[1] * u[4] + V[2] * u[5];
    T.t1 = V[3] * u[3] + V[4] * u[4] + V[5] * u[5];
    T.t2 = V[6] * u[3] + V[7] * u[4] + V[8] * u[5];
    return T;
}
SE3_HD Se3 se3_mul(const Se3 &a, const Se3 &b)      // se3quat.h:104-110
{
    Se3 r;
    double r0, r1, r2;
    quat_rotate(a, b.t0, b.t1, b.t2, r0, r1, r2);
    r.t0 = a.t0 + r0; r.t1 = a.t1 + r1; r.t2 = a.t2 + r2;
    quat_mul(a, b, r);
    quat_normalize(r);
    return r;
}

// RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91): rho and rho'
SE3_HD void huber(double c2, double delta, double &rho0, double &rho1)
{
    const double dsqr = delta * delta;
    if (c2 <= dsqr) { rho0 = c2; rho1 = 1.; }
    else { const double s = sqrt(c2); rho0 = 2 * s * delta - dsqr; rho1 = delta / s; }
}
