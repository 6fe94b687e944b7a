// orbm_pose.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:239-451 of WChen09/My-SLAM, on g2o) for a batch of independent
// problems in one launch: the frames of a step, or the candidate key frames of Tracking::Relocalization (src/Tracking.cc:1447-1478).
// orbm_pose_optimization_batch / orbm_pose_optimization_batch_device (include/orbm.h).  The kernel restates the host path
// orbp_pose_optimization (orbp.cc) operation by operation in fp64; the build's -ffp-contract=off keeps every per-edge quantity
// bit-identical to the host's, and only the order of the sums over the edges differs.
//
// One workgroup of 256 threads per problem; thread t owns the edges t, t + 256, ... of its problem in every pass, so no edge's flag
// is read by a thread that did not write it.  The pose, the Levenberg state and the 6x6 solve are held redundantly by every thread:
// all of them read the same reduced sums from one LDS block after a barrier, hence take the same branches, and every barrier is
// reached by the whole workgroup.  The loops are bounded at compile time (4 rounds x 10 iterations x 10 trials); there is no wait
// on another workgroup and no atomic.
//
// Sums over edges (the 21 + 6 entries of the normal equations and the robust chi2): every thread adds its own edges in ascending
// order from 0, then a fixed tree: 8 threads per sum add 32 of the 256 partials each (partial k*8 + c for k = 0..31), one thread
// adds those 8 as ((0+1)+(2+3))+((4+5)+(6+7)).  The result depends on the problem alone, not on the batch around it.
//
// Edge state: g2o leaves the errors of a rejected trial on the edges, and the flagging pass reads them (orbp.cc, "the edges keep
// the trial's errors").  The errors of all active edges are always those at the estimate compute_active_errors() last saw, and an
// inactive edge is recomputed at the final estimate before it is read, so one extra estimate per problem (err_est) stands for the
// per-edge store: an edge's error is recomputed from it where the host reads the stored one, with the same operations.
#include "orbm_hyp.h"

#define POSE_THREADS 256
#define POSE_NSYS 28                            // 21 upper-triangle sums, 6 of b, the robust chi2
#define POSE_PSTRIDE (POSE_THREADS + 8)         // partial row stride (doubles): the 8 threads of a sum read different banks

struct PQuat { double w, x, y, z; };
struct PSe3 { PQuat r; double t0, t1, t2; };
struct PCam { double fx, fy, cx, cy, bf; };

// Eigen's Quaterniond(Matrix3d) (orbp.cc quat_from_R); the branch on the largest diagonal entry written out per case
__device__ __forceinline__ PQuat pose_quat_from_R(const double (&R)[9])
{
    PQuat q;
    double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        tr = sqrt(tr + 1.0);
        q.w = 0.5 * tr;
        tr = 0.5 / tr;
        q.x = (R[7] - R[5]) * tr; q.y = (R[2] - R[6]) * tr; q.z = (R[3] - R[1]) * tr;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i ? R[4] : R[0])) i = 2;
        if (i == 0) {               // j = 1, k = 2
            tr = sqrt(R[0] - R[4] - R[8] + 1.0);
            q.x = 0.5 * tr; tr = 0.5 / tr;
            q.w = (R[7] - R[5]) * tr; q.y = (R[3] + R[1]) * tr; q.z = (R[6] + R[2]) * tr;
        } else if (i == 1) {        // j = 2, k = 0
            tr = sqrt(R[4] - R[8] - R[0] + 1.0);
            q.y = 0.5 * tr; tr = 0.5 / tr;
            q.w = (R[2] - R[6]) * tr; q.z = (R[7] + R[5]) * tr; q.x = (R[1] + R[3]) * tr;
        } else {                    // j = 0, k = 1
            tr = sqrt(R[8] - R[0] - R[4] + 1.0);
            q.z = 0.5 * tr; tr = 0.5 / tr;
            q.w = (R[3] - R[1]) * tr; q.x = (R[2] + R[6]) * tr; q.y = (R[5] + R[7]) * tr;
        }
    }
    return q;
}
__device__ __forceinline__ void pose_quat_normalize(PQuat &q)
{
    if (q.w < 0) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
    const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    q.w /= n; q.x /= n; q.y /= n; q.z /= n;
}
__device__ __forceinline__ PQuat pose_quat_mul(const PQuat &a, const PQuat &b)
{
    PQuat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
__device__ __forceinline__ void pose_quat_rotate(const PQuat &q, double v0, double v1, double v2, double &o0, double &o1, double &o2)
{
    double u0 = q.y * v2 - q.z * v1, u1 = q.z * v0 - q.x * v2, u2 = q.x * v1 - q.y * v0;
    u0 += u0; u1 += u1; u2 += u2;
    o0 = v0 + q.w * u0 + (q.y * u2 - q.z * u1);
    o1 = v1 + q.w * u1 + (q.z * u0 - q.x * u2);
    o2 = v2 + q.w * u2 + (q.x * u1 - q.y * u0);
}
// se3quat.h:223-257 (orbp.cc se3_exp).  sin / cos are the device library's (within an ulp of the host's libm); theta^3 is
// theta * theta * theta where the host calls pow(theta, 3)
__device__ __forceinline__ PSe3 pose_se3_exp(const double (&u)[6])
{
    const double om0 = u[0], om1 = u[1], om2 = u[2];
    const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
    double O2[9], R[9], V[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0) + O[i] + O2[i]; V[i] = R[i]; }
    } else {
        const double sn = sin(theta), cs = cos(theta);
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        const double c = (theta - sn) / (theta * theta * theta);
#pragma unroll
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0) + a * O[i] + b * O2[i]; V[i] = (i % 4 == 0) + b * O[i] + c * O2[i]; }
    }
    PSe3 T;
    T.r = pose_quat_from_R(R);
    pose_quat_normalize(T.r);
    T.t0 = V[0] * u[3] + V[1] * u[4] + V[2] * u[5];
    T.t1 = V[3] * u[3] + V[4] * u[4] + V[5] * u[5];
    T.t2 = V[6] * u[3] + V[7] * u[4] + V[8] * u[5];
    return T;
}
__device__ __forceinline__ PSe3 pose_se3_mul(const PSe3 &a, const PSe3 &b)     // se3quat.h:104-110
{
    PSe3 r = a;
    double r0, r1, r2;
    pose_quat_rotate(a.r, b.t0, b.t1, b.t2, r0, r1, r2);
    r.t0 += r0; r.t1 += r1; r.t2 += r2;
    r.r = pose_quat_mul(a.r, b.r);
    pose_quat_normalize(r.r);
    return r;
}

// orbp.cc ldlt_solve6 on the upper triangle Hu (row-major, 21 entries) with lambda on the diagonal; false (and x = 0) where the
// host returns before it writes x
__device__ __forceinline__ bool pose_ldlt_solve6(const double (&Hu)[21], double lambda, const double (&b)[6], double (&x)[6])
{
    double H[36];
    {
        int u = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++, u++) H[6 * r + c] = H[6 * c + r] = Hu[u];
    }
#pragma unroll
    for (int j = 0; j < 6; j++) H[7 * j] += lambda;
    double L[36], D[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = H[6 * j + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[6 * j + k] * L[6 * j + k] * D[k];
        if (!(fabs(d) > 0) || !isfinite(d)) ok = false;
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = H[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = s / d;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[6 * i + k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] /= D[i];
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[6 * k + i] * x[k];
        x[i] = s;
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = 0;
    }
    return ok;
}

struct PEdge { bool stereo; double o0, o1, o2, info, pc0, pc1, pc2, e0, e1, e2; };

// the edge as orbp_pose_optimization builds it, and compute_error at T (types_six_dof_expmap.h:153-157,184-188; .cpp:290-306)
__device__ __forceinline__ void pose_edge_error(PEdge &e, const PSe3 &T, const PCam &cam, long long i, const float *__restrict__ obs,
                                                const float *__restrict__ u_right, const float *__restrict__ inv_sigma2,
                                                const float *__restrict__ xw)
{
    const float ur = u_right ? u_right[i] : -1.0f;
    e.stereo = u_right && ur >= 0;
    e.o0 = obs[2 * i]; e.o1 = obs[2 * i + 1]; e.o2 = e.stereo ? (double)ur : 0.0;
    e.info = inv_sigma2[i];
    pose_quat_rotate(T.r, (double)xw[3 * i], (double)xw[3 * i + 1], (double)xw[3 * i + 2], e.pc0, e.pc1, e.pc2);
    e.pc0 += T.t0; e.pc1 += T.t1; e.pc2 += T.t2;
    if (!e.stereo) {
        e.e0 = e.o0 - (e.pc0 / e.pc2 * cam.fx + cam.cx);
        e.e1 = e.o1 - (e.pc1 / e.pc2 * cam.fy + cam.cy);
        e.e2 = 0;
    } else {
        const float invz = __fdiv_rn(1.0f, (float)e.pc2);
        const double u = e.pc0 * invz * cam.fx + cam.cx;
        e.e0 = e.o0 - u;
        e.e1 = e.o1 - (e.pc1 * invz * cam.fy + cam.cy);
        e.e2 = e.o2 - (u - cam.bf * invz);
    }
}
__device__ __forceinline__ double pose_chi2(const PEdge &e) { return (e.e0 * e.e0 + e.e1 * e.e1 + e.e2 * e.e2) * e.info; }
// RobustKernelHuber (robust_kernel_impl.cpp:78-91): rho and rho'
__device__ __forceinline__ void pose_huber(bool stereo, double c2, double &rho0, double &rho1)
{
    const double delta = stereo ? (double)(float)2.7955321496988725 : (double)(float)2.4476519360399264;   // (float)sqrt(7.815), (float)sqrt(5.991)
    const double dsqr = delta * delta;
    if (c2 <= dsqr) { rho0 = c2; rho1 = 1.; }
    else { const double s = sqrt(c2); rho0 = 2 * s * delta - dsqr; rho1 = delta / s; }
}

// The fixed tree of the file comment: acc[v] of every thread -> the same total in acc[v] of every thread.  Three barriers, each
// reached by the whole workgroup.
template <int NV>
__device__ __forceinline__ void pose_reduce(double (&acc)[NV], double *part, double *mid, double *out)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int v = 0; v < NV; v++) part[v * POSE_PSTRIDE + tid] = acc[v];
    __syncthreads();
    if (tid < NV * 8) {
        const int v = tid >> 3, c = tid & 7;
        double s = 0;
#pragma unroll 8
        for (int k = 0; k < POSE_THREADS / 8; k++) s += part[v * POSE_PSTRIDE + k * 8 + c];
        mid[tid] = s;
    }
    __syncthreads();
    if (tid < NV) {
        const double *q = mid + 8 * tid;
        out[tid] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = out[v];
}

// compute_active_errors + active_robust_chi2 at T, and with SYSTEM build_system (linearizeOplus .cpp:266-288,335-364 +
// constructQuadraticForm) from the same errors.  acc: [0..20] Hu, [21..26] b, [27] chi2 (SYSTEM) or [0] chi2.
template <bool SYSTEM>
__device__ __forceinline__ void pose_pass(const PSe3 &T, const PCam &cam, bool robust, int n, const float *__restrict__ obs,
                                          const float *__restrict__ u_right, const float *__restrict__ inv_sigma2,
                                          const float *__restrict__ xw, const uint8_t *outl, double (&acc)[SYSTEM ? POSE_NSYS : 1],
                                          double *part, double *mid, double *out)
{
    constexpr int NV = SYSTEM ? POSE_NSYS : 1, CHI = SYSTEM ? POSE_NSYS - 1 : 0;
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = 0;
    for (int i = threadIdx.x; i < n; i += POSE_THREADS) {
        if (outl[i]) continue;                  // level 1: not in the active set
        PEdge e;
        pose_edge_error(e, T, cam, i, obs, u_right, inv_sigma2, xw);
        const double c2 = pose_chi2(e);
        double rho0 = c2, w = 1.0;
        if (robust) pose_huber(e.stereo, c2, rho0, w);
        acc[CHI] += rho0;
        if (SYSTEM) {
            const double x = e.pc0, y = e.pc1, invz = 1.0 / e.pc2, invz_2 = invz * invz;
            const double fx = cam.fx, fy = cam.fy, bf = cam.bf;
            double J[3][6];
            J[0][0] = x * y * invz_2 * fx; J[0][1] = -(1 + (x * x * invz_2)) * fx; J[0][2] = y * invz * fx;
            J[0][3] = -invz * fx; J[0][4] = 0; J[0][5] = x * invz_2 * fx;
            J[1][0] = (1 + y * y * invz_2) * fy; J[1][1] = -x * y * invz_2 * fy; J[1][2] = -x * invz * fy;
            J[1][3] = 0; J[1][4] = -invz * fy; J[1][5] = y * invz_2 * fy;
            const double wi = w * e.info;
            double wJ[3][6];
#pragma unroll
            for (int r = 0; r < 6; r++) { wJ[0][r] = J[0][r] * wi; wJ[1][r] = J[1][r] * wi; }
            if (!e.stereo) {
                int u = 0;
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    const double g = J[0][r] * e.info * e.e0 + J[1][r] * e.info * e.e1;
                    acc[21 + r] -= w * g;
#pragma unroll
                    for (int c = r; c < 6; c++, u++) acc[u] += wJ[0][r] * J[0][c] + wJ[1][r] * J[1][c];
                }
            } else {
                J[2][0] = J[0][0] - bf * y * invz_2; J[2][1] = J[0][1] + bf * x * invz_2; J[2][2] = J[0][2];
                J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - bf * invz_2;
#pragma unroll
                for (int r = 0; r < 6; r++) wJ[2][r] = J[2][r] * wi;
                int u = 0;
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    const double g = J[0][r] * e.info * e.e0 + J[1][r] * e.info * e.e1 + J[2][r] * e.info * e.e2;
                    acc[21 + r] -= w * g;
#pragma unroll
                    for (int c = r; c < 6; c++, u++) acc[u] += wJ[0][r] * J[0][c] + wJ[1][r] * J[1][c] + wJ[2][r] * J[2][c];
                }
            }
        }
    }
    pose_reduce<NV>(acc, part, mid, out);
}

__global__ __launch_bounds__(POSE_THREADS) void k_pose_optimization(
    const int32_t *__restrict__ off, const float *__restrict__ obs_all, const float *__restrict__ u_right_all,
    const float *__restrict__ inv_sigma2_all, const float *__restrict__ xw_all, const orbm_pose_camera *__restrict__ cams,
    const float *Tcw_in, float *Tcw_out, uint8_t *outlier_all, int32_t *__restrict__ n_good)
{
    __shared__ double part[POSE_NSYS * POSE_PSTRIDE];
    __shared__ double mid[POSE_NSYS * 8];
    __shared__ double out[POSE_NSYS];
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long e0 = off[p];
    const int n = off[p + 1] - off[p];
    const float *obs = obs_all + 2 * e0, *u_right = u_right_all ? u_right_all + e0 : nullptr;
    const float *inv_sigma2 = inv_sigma2_all + e0, *xw = xw_all + 3 * e0;
    uint8_t *outl = outlier_all + e0;
    const float *Tin = Tcw_in + 16 * (long long)p;
    float *Tout = Tcw_out + 16 * (long long)p;

    for (int i = tid; i < n; i += POSE_THREADS) outl[i] = 0;
    if (n < 3) {                                // src/Optimizer.cc:363-364: the pose stays as it came
        if (Tin != Tout && tid < 16) Tout[tid] = Tin[tid];
        if (tid == 0) n_good[p] = 0;
        return;
    }
    PCam cam;
    cam.fx = cams[p].fx; cam.fy = cams[p].fy; cam.cx = cams[p].cx; cam.cy = cams[p].cy; cam.bf = cams[p].bf;
    PSe3 init;
    {
        double R0[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R0[3 * i + j] = Tin[4 * i + j];
        init.r = pose_quat_from_R(R0);
        pose_quat_normalize(init.r);
        init.t0 = Tin[3]; init.t1 = Tin[7]; init.t2 = Tin[11];
    }
    PSe3 est = init, err_est = init;            // err_est: the estimate the errors on the active edges were computed at
    int n_bad = 0;
    for (int round = 0; round < 4; round++) {
        est = init;                             // every round restarts from pFrame->mTcw (:375)
        const bool robust = round < 3;          // setRobustKernel(0) after the third round (:435-436)
        if (n - n_bad > 0) {
            // OptimizationAlgorithmLevenberg::solve driven by SparseOptimizer::optimize(10) (orbp.cc PoseProblem::optimize)
            double lambda = 0, ni = 2, carried = 0;
            int lm_bad = 0;
            bool fresh = false;
            for (int it = 0; it < 10; it++) {
                double sys[POSE_NSYS];
                pose_pass<true>(est, cam, robust, n, obs, u_right, inv_sigma2, xw, outl, sys, part, mid, out);
                err_est = est;
                // right after an accepted step the chi2 the trial summed is the one this pass sums again: same edges, same
                // estimate, same tree
                if (!fresh) carried = sys[POSE_NSYS - 1];
                double current = carried, temp = current;
                const double ini = current;
                double Hu[21], b[6], x[6];
#pragma unroll
                for (int v = 0; v < 21; v++) Hu[v] = sys[v];
#pragma unroll
                for (int v = 0; v < 6; v++) b[v] = sys[21 + v];
                if (it == 0) {
                    const double mx = fmax(fabs(Hu[20]), fmax(fabs(Hu[18]), fmax(fabs(Hu[15]), fmax(fabs(Hu[11]), fmax(fabs(Hu[6]), fmax(fabs(Hu[0]), 0.0))))));
                    lambda = 1e-5 * mx; ni = 2; lm_bad = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    const PSe3 backup = est;
                    const bool ok2 = pose_ldlt_solve6(Hu, lambda, b, x);
                    est = pose_se3_mul(pose_se3_exp(x), est);
                    double t1[1];
                    pose_pass<false>(est, cam, robust, n, obs, u_right, inv_sigma2, xw, outl, t1, part, mid, out);
                    err_est = est;
                    temp = ok2 ? t1[0] : 1.7976931348623157e308;
                    rho = current - temp;
                    double scale = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && isfinite(temp)) {
                        const double t = 2 * rho - 1;
                        double alpha = 1. - t * t * t;          // the host's pow(2 rho - 1, 3) as two multiplications
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha);
                        ni = 2;
                        current = temp;
                        fresh = true; carried = temp;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        est = backup;                           // err_est stays at the trial, as the edges do in g2o
                        fresh = false;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                if (qmax == 10 || rho == 0) break;
                if ((ini - current) * 1e3 < ini) lm_bad++; else lm_bad = 0;
                if (lm_bad >= 3) break;
            }
        }
        // the flagging pass (:384-440): an outlier of the last round is recomputed at the final estimate, every other edge
        // keeps the error of the estimate the optimiser last evaluated
        double bad[1] = {0};
        for (int i = tid; i < n; i += POSE_THREADS) {
            PEdge e;
            pose_edge_error(e, outl[i] ? est : err_est, cam, i, obs, u_right, inv_sigma2, xw);
            const float c2 = (float)pose_chi2(e);
            const bool o = c2 > (e.stereo ? 7.815f : 5.991f);
            outl[i] = o ? 1 : 0;
            bad[0] += o ? 1.0 : 0.0;
        }
        pose_reduce<1>(bad, part, mid, out);    // a count: exact in double
        n_bad = (int)bad[0];
        if (n < 10) break;                      // optimizer.edges().size() < 10 (:443-444)
    }
    if (tid == 0) {
        const PQuat &q = est.r;
        const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
        const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
        const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
        Tout[0] = (float)(1 - (tyy + tzz)); Tout[1] = (float)(txy - twz); Tout[2] = (float)(txz + twy); Tout[3] = (float)est.t0;
        Tout[4] = (float)(txy + twz); Tout[5] = (float)(1 - (txx + tzz)); Tout[6] = (float)(tyz - twx); Tout[7] = (float)est.t1;
        Tout[8] = (float)(txz - twy); Tout[9] = (float)(tyz + twx); Tout[10] = (float)(1 - (txx + tyy)); Tout[11] = (float)est.t2;
        Tout[12] = 0.f; Tout[13] = 0.f; Tout[14] = 0.f; Tout[15] = 1.f;
        n_good[p] = n - n_bad;
    }
}

extern "C" int orbm_pose_optimization_batch(orbm_matcher *m, int n_problems, const int32_t *off, const float *obs, const float *u_right,
                                            const float *inv_sigma2, const float *xw, const orbm_pose_camera *cams, float *Tcw,
                                            uint8_t *outlier, int32_t *n_good)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(off, cams, Tcw, n_good)) return mfail(ORBX_E_INVALID, "NULL buffer");
    int total;
    MTRY(check_off_csr(n_problems, off, "observations", total));
    if (total > 0 && any_null(obs, inv_sigma2, xw, outlier)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (u_right)
        for (int p = 0; p < n_problems; p++) {
            if (cams[p].bf != 0.0f) continue;
            for (int i = off[p]; i < off[p + 1]; i++)
                if (u_right[i] >= 0) return mfail(ORBX_E_INVALID, "problem %d has a stereo edge (u_right[%d] >= 0) but its camera's bf is 0", p, i);
        }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out (3 * max_q ints) holds the poses, the counts, then the flags
    const size_t B = (size_t)n_problems, N = (size_t)total;
    const OutBlock out({{Tcw, B * 64}, {n_good, B * 4}, {outlier, N}});
    MTRY(orbm_grow(m, (long long)((out.words() + 2) / 3), 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int po = in.add(off, (B + 1) * 4), pb = in.add(obs, N * 8), pu = in.add(u_right, u_right ? N * 4 : 0), pi = in.add(inv_sigma2, N * 4),
              px = in.add(xw, N * 12), pc = in.add(cams, B * sizeof(orbm_pose_camera)), pt = in.add(Tcw, B * 64);
    MTRY(in.upload(s));
    hipLaunchKernelGGL(k_pose_optimization, dim3(n_problems), dim3(POSE_THREADS), 0, s, in.dev_at<int32_t>(po), in.at<float>(pb), in.at<float>(pu),
                       in.at<float>(pi), in.at<float>(px), in.dev_at<orbm_pose_camera>(pc), in.dev_at<float>(pt), out.dev_at<float>(m, 0),
                       out.dev_at<uint8_t>(m, 2), out.dev_at<int32_t>(m, 1));
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_pose_optimization_batch_device(orbm_matcher *m, int n_problems, const int32_t *d_off, const float *d_obs,
                                                   const float *d_u_right, const float *d_inv_sigma2, const float *d_xw,
                                                   const orbm_pose_camera *d_cams, float *d_Tcw, uint8_t *d_outlier, int32_t *d_n_good,
                                                   void *hip_stream)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(d_off, d_obs, d_inv_sigma2, d_xw, d_cams, d_Tcw, d_outlier, d_n_good)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_off, d_obs, d_u_right, d_inv_sigma2, d_xw, d_cams, d_Tcw, d_n_good))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    hipLaunchKernelGGL(k_pose_optimization, dim3(n_problems), dim3(POSE_THREADS), 0, s, d_off, d_obs, d_u_right, d_inv_sigma2, d_xw, d_cams,
                       d_Tcw, d_Tcw, d_outlier, d_n_good);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
