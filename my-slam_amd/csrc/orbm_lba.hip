// orbm_lba.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778 of WChen09/My-SLAM, on g2o) on the GPU:
// orbm_local_bundle_adjustment (include/orbm.h).  The kernels run the text of the host path orbp_local_bundle_adjustment
// (orbp_lba.cc): csrc/orbp_lba_body.h holds the SE3 algebra, both edges' computeError and linearizeOplus, Huber, an edge's quadratic
// form, a point's 3x3 inverse and the Schur terms for both, csrc/orbp_lm_body.h the Levenberg loop; only the order of the sums over
// edges, the device's sin / cos and the inside of the dense solve differ.
//
// Launch structure: one upload, then lm_optimize (the Levenberg loop, on the host) over plain kernel launches in stream
// order, then one download.  A trial is six launches and one 64-byte read-back (robust chi2, computeScale's sum, the solve's ok
// flag), where the host takes g2o's decisions and reads `stop`.  There is no cooperative launch, no grid-wide barrier, no spin-wait,
// no communication between workgroups other than kernel boundaries and no floating-point atomic; every kernel loop is bounded by
// the problem's counts and the host loop by the iterations asked for x 10 trials.
//
// Sums (all in fixed orders, so the result is a function of the problem alone):
//   a point's Hll, b_l and its back-substitution     one thread per point, its edges in ascending order (the host's order)
//   a key frame's Hpp, b_p                           one wave per key frame over its edges in ascending order: lane l adds the
//                                                    edges l, l + 64, ... of the list, then opt_wave_sum (orbm_opt.h)
//   a block (i1 <= i2) of B Dinv B^T and of bschur   one wave per block over key frame i1's edges, the same lanes and butterfly.
//                                                    Key frame i2's edge on the same point comes from a dense n_local x n_points
//                                                    table of edge indices (4 bytes an entry, 1.3 MB at 40 x 8000): one load
//                                                    instead of a search of the point's observers, and the table is rebuilt by one
//                                                    launch a call
//   robust chi2, computeScale, counts                one workgroup of 1024 threads: thread t adds the entries t, t + 1024, ...,
//                                                    then opt_block_sum (orbm_opt.h has the tree)
// The dense solve: one workgroup of 256 threads factors S = L L^T in place in the workspace, right-looking over 6-wide block
// columns, then substitutes forwards and backwards; a pivot that is not positive or not finite clears the ok flag and the update.
//
// orbm_bundle_adjustment (Optimizer::BundleAdjustment, src/Optimizer.cc:49-237) is a second short driver over the same set-up and
// the same launches: one optimize(n_iterations) with the call's robust kernel, no flagging pass, and the reduced system handed to the
// many-workgroup solve of orbm_spd.hip instead of k_lba_solve.
#include "orbm_hyp.h"
#include "orbm_opt.h"
#include "ws_layout.h"
#include "orbp_internal.h"
#include "orbp_lba_body.h"
#include "../../include/orbp.h"
#include "../../include/orbm.h"

#define LBA_T 256
#define LBA_RT 1024

namespace {
struct LbaDev {
    int K, NK, P, E, n;                     // local key frames, all key frames, points, edges, 6 K
    // the problem
    const float *Tcw, *cam, *xw_in, *obs, *u_right, *inv_sigma2;
    const uint8_t *local_fixed;
    const int32_t *edge_off, *edge_kf, *kf_off, *kf_edge;    // kf_off / kf_edge: CSR by local key frame, edges ascending
    // state
    double *est[2], *X[2];                  // 7 doubles a key frame, 3 a point; [cur] the estimates, [1 - cur] a trial's
    double *err, *chi_e, *blk;              // 3, 1, LBA_NBLK an edge
    int32_t *edge_pt, *table;               // the edge's point; table[k * P + pt] = key frame k's edge on pt or -1
    uint8_t *level, *kf_active, *pt_active, *erase;
    double *Hll, *bl, *Dinv, *Db, *pmax, *pterm;             // 6, 3, 9, 3, 1, 1 a point
    double *Hpp, *bp, *kmax, *kterm;        // 21, 6, 1, 1 a local key frame
    double *S, *bs, *xp;                    // n x n, n, n
    double *out;                            // 8: chi2, scale, ok, maxdiag, active edges, level-1 edges
    float *out_Tcw, *out_xw;
};
enum { OUT_CHI = 0, OUT_SCALE = 1, OUT_OK = 2, OUT_MAXDIAG = 3, OUT_ACTIVE = 4, OUT_LEVEL1 = 5 };

__device__ __forceinline__ LbaSe3 load_se3(const double *p) { return {{p[0], p[1], p[2], p[3]}, p[4], p[5], p[6]}; }
__device__ __forceinline__ void store_se3(double *p, const LbaSe3 &T)
{
    p[0] = T.qx; p[1] = T.qy; p[2] = T.qz; p[3] = T.qw; p[4] = T.t0; p[5] = T.t1; p[6] = T.t2;
}
__device__ __forceinline__ LbaCam load_cam(const float *c) { return {c[0], c[1], c[2], c[3], c[4]}; }
__device__ __forceinline__ bool kf_is_free(const LbaDev &d, int k) { return k < d.K && !d.local_fixed[k]; }

// thread i: key frame i (the estimate of its pose), point i, edge i (level 0, no stored error, its place in the table)
__global__ __launch_bounds__(LBA_T) void k_lba_init(LbaDev d)
{
    const long long i = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (i < d.NK) store_se3(d.est[0] + 7 * i, se3_from_Tcw(d.Tcw + 16 * i));
    if (i < d.P) {
        for (int j = 0; j < 3; j++) d.X[0][3 * i + j] = (double)d.xw_in[3 * i + j];
        for (int e = d.edge_off[i]; e < d.edge_off[i + 1]; e++) {
            d.edge_pt[e] = (int)i;
            const int k = d.edge_kf[e];
            if (k < d.K) d.table[(long long)k * d.P + i] = e;
        }
    }
    if (i < d.E) {
        d.level[i] = 0;
        d.err[3 * i] = d.err[3 * i + 1] = d.err[3 * i + 2] = 0;
    }
}
// initializeOptimization(0): thread i decides point i and local key frame i
__global__ __launch_bounds__(LBA_T) void k_lba_activate(LbaDev d)
{
    const long long i = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (i < d.P) {
        uint8_t a = 0;
        for (int e = d.edge_off[i]; e < d.edge_off[i + 1]; e++) a |= !d.level[e];
        d.pt_active[i] = a;
    }
    if (i < d.K) {
        uint8_t a = 0;
        if (!d.local_fixed[i])
            for (int q = d.kf_off[i]; q < d.kf_off[i + 1]; q++) a |= !d.level[d.kf_edge[q]];
        d.kf_active[i] = a;
    }
}
// computeActiveErrors and every active edge's term of activeRobustChi2 at the estimates [b]
__global__ __launch_bounds__(LBA_T) void k_lba_errors(LbaDev d, int b, int robust)
{
    const long long e = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E) return;
    if (d.level[e]) { d.chi_e[e] = 0; return; }
    const int k = d.edge_kf[e];
    double pc[3], err[3];
    lba_edge_error(load_se3(d.est[b] + 7 * (long long)k), load_cam(d.cam + 5 * (long long)k), d.X[b] + 3 * (long long)d.edge_pt[e],
                   d.obs + 2 * e, d.u_right[e], pc, err);
    d.err[3 * e] = err[0]; d.err[3 * e + 1] = err[1]; d.err[3 * e + 2] = err[2];
    d.chi_e[e] = lba_edge_robust_chi2(err, (double)d.inv_sigma2[e], !(d.u_right[e] < 0), robust);
}
// linearizeOplus + constructQuadraticForm of every active edge
__global__ __launch_bounds__(LBA_T) void k_lba_linearize(LbaDev d, int b, int robust)
{
    const long long e = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E || d.level[e]) return;
    const int k = d.edge_kf[e];
    const double err[3] = {d.err[3 * e], d.err[3 * e + 1], d.err[3 * e + 2]};
    double blk[LBA_NBLK];
    lba_edge_blocks(load_se3(d.est[b] + 7 * (long long)k), load_cam(d.cam + 5 * (long long)k), d.X[b] + 3 * (long long)d.edge_pt[e], err,
                    (double)d.inv_sigma2[e], !(d.u_right[e] < 0), robust, kf_is_free(d, k), blk);
    double *o = d.blk + LBA_NBLK * e;
#pragma unroll
    for (int i = 0; i < LBA_NBLK; i++) o[i] = blk[i];
}
// Hll and b_l of point i over its active edges in ascending order, and its part of computeLambdaInit's maximum
__global__ __launch_bounds__(LBA_T) void k_lba_reduce_points(LbaDev d)
{
    const long long i = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (i >= d.P) return;
    double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int e = d.edge_off[i]; e < d.edge_off[i + 1]; e++) {
        if (d.level[e]) continue;
        const double *s = d.blk + LBA_NBLK * (long long)e;
#pragma unroll
        for (int j = 0; j < 6; j++) H[j] += s[LBA_HLL + j];
#pragma unroll
        for (int j = 0; j < 3; j++) b[j] += s[LBA_BL + j];
    }
#pragma unroll
    for (int j = 0; j < 6; j++) d.Hll[6 * i + j] = H[j];
#pragma unroll
    for (int j = 0; j < 3; j++) d.bl[3 * i + j] = b[j];
    d.pmax[i] = d.pt_active[i] ? fmax(fabs(H[5]), fmax(fabs(H[3]), fmax(fabs(H[0]), 0.0))) : 0.0;
}
// Hpp and b_p of local key frame k: one wave, lanes stride its edge list, then the butterfly
__global__ __launch_bounds__(64) void k_lba_reduce_kfs(LbaDev d)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    double acc[27];
#pragma unroll
    for (int j = 0; j < 27; j++) acc[j] = 0;
    if (d.kf_active[k])
        for (int q = d.kf_off[k] + lane; q < d.kf_off[k + 1]; q += 64) {
            const int e = d.kf_edge[q];
            if (d.level[e]) continue;
            const double *s = d.blk + LBA_NBLK * (long long)e;
#pragma unroll
            for (int j = 0; j < 27; j++) acc[j] += s[LBA_HPP + j];
        }
#pragma unroll
    for (int j = 0; j < 27; j++) acc[j] = opt_wave_sum(acc[j]);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 21; j++) d.Hpp[21 * (long long)k + j] = acc[j];
#pragma unroll
        for (int j = 0; j < 6; j++) d.bp[6 * (long long)k + j] = acc[21 + j];
        d.kmax[k] = fmax(fabs(acc[20]), fmax(fabs(acc[18]), fmax(fabs(acc[15]), fmax(fabs(acc[11]), fmax(fabs(acc[6]), fmax(fabs(acc[0]), 0.0))))));
    }
}
// setLambda on a point's block, Dinv and Dinv b_l
__global__ __launch_bounds__(LBA_T) void k_lba_dinv(LbaDev d, double lambda)
{
    const long long i = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (i >= d.P || !d.pt_active[i]) return;
    double Dinv[9], Db[3];
    lba_point_dinv(d.Hll + 6 * i, d.bl + 3 * i, lambda, Dinv, Db);
#pragma unroll
    for (int j = 0; j < 9; j++) d.Dinv[9 * i + j] = Dinv[j];
#pragma unroll
    for (int j = 0; j < 3; j++) d.Db[3 * i + j] = Db[j];
}
// Block (i1, i2), i1 <= i2, of S = (Hpp + lambda I) - sum B Dinv B^T, mirrored below the diagonal, and on the diagonal blocks
// bschur = b_p - sum B Dinv b_l.  A local key frame without active edges keeps an identity block and a zero right-hand side.
__global__ __launch_bounds__(64) void k_lba_schur(LbaDev d, double lambda)
{
    const int i2 = blockIdx.x, i1 = blockIdx.y, lane = threadIdx.x, n = d.n;
    if (i1 > i2) return;
    const bool on = d.kf_active[i1] && d.kf_active[i2];
    double acc[36], coef[6];
#pragma unroll
    for (int j = 0; j < 36; j++) acc[j] = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) coef[j] = 0;
    if (on)
        for (int q = d.kf_off[i1] + lane; q < d.kf_off[i1 + 1]; q += 64) {
            const int e = d.kf_edge[q];
            if (d.level[e]) continue;
            const int pt = d.edge_pt[e];
            const int e2 = i1 == i2 ? e : d.table[(long long)i2 * d.P + pt];
            if (e2 < 0 || d.level[e2]) continue;
            const double *W = d.blk + LBA_NBLK * (long long)e + LBA_HPL, *W2 = d.blk + LBA_NBLK * (long long)e2 + LBA_HPL;
            double Y[18], M[36];
            lba_mul_WD(W, d.Dinv + 9 * (long long)pt, Y);
            lba_mul_YWt(Y, W2, M);
#pragma unroll
            for (int j = 0; j < 36; j++) acc[j] += M[j];
            if (i1 == i2) {
                double v[6];
                lba_mul_Wd(W, d.Db + 3 * (long long)pt, v);
#pragma unroll
                for (int j = 0; j < 6; j++) coef[j] += v[j];
            }
        }
#pragma unroll
    for (int j = 0; j < 36; j++) acc[j] = opt_wave_sum(acc[j]);
    if (i1 == i2) {
#pragma unroll
        for (int j = 0; j < 6; j++) coef[j] = opt_wave_sum(coef[j]);
    }
    if (lane != 0) return;
    if (i1 == i2) {
        int u = 0;
        for (int r = 0; r < 6; r++)
            for (int c = r; c < 6; c++, u++) {
                const double v = on ? (d.Hpp[21 * (long long)i1 + u] + (r == c ? lambda : 0.)) - acc[6 * r + c] : (r == c ? 1. : 0.);
                d.S[(long long)(6 * i1 + r) * n + 6 * i1 + c] = v;
                d.S[(long long)(6 * i1 + c) * n + 6 * i1 + r] = v;
            }
        for (int r = 0; r < 6; r++) d.bs[6 * i1 + r] = on ? d.bp[6 * (long long)i1 + r] - coef[r] : 0.;
    } else {
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 6; c++) {
                const double v = 0. - acc[6 * r + c];
                d.S[(long long)(6 * i1 + r) * n + 6 * i2 + c] = v;
                d.S[(long long)(6 * i2 + c) * n + 6 * i1 + r] = v;
            }
    }
}
// S = L L^T in place (the lower triangle), right-looking over 6-wide block columns, then L y = bschur and L^T x = y in bs; x into
// xp and the ok flag into out.  One workgroup; every barrier is reached by all of it (the failure flag is read after a barrier).
__global__ __launch_bounds__(LBA_T) void k_lba_solve(LbaDev d)
{
    __shared__ int fail;
    __shared__ double piv[6];
    const int n = d.n, nb = d.K, tid = threadIdx.x;
    double *A = d.S, *b = d.bs;
    if (tid == 0) fail = 0;
    __syncthreads();
    for (int J = 0; J < nb; J++) {
        const int j0 = 6 * J;
        if (tid == 0) {                     // the diagonal block, unblocked
            for (int j = 0; j < 6; j++) {
                double v = A[(long long)(j0 + j) * n + j0 + j];
                for (int k = 0; k < j; k++) v -= A[(long long)(j0 + j) * n + j0 + k] * A[(long long)(j0 + j) * n + j0 + k];
                if (!(v > 0) || !isfinite(v)) { fail = 1; break; }
                v = sqrt(v);
                A[(long long)(j0 + j) * n + j0 + j] = v;
                for (int i = j + 1; i < 6; i++) {
                    double s = A[(long long)(j0 + i) * n + j0 + j];
                    for (int k = 0; k < j; k++) s -= A[(long long)(j0 + i) * n + j0 + k] * A[(long long)(j0 + j) * n + j0 + k];
                    A[(long long)(j0 + i) * n + j0 + j] = s / v;
                }
            }
        }
        __syncthreads();
        if (fail) break;
        for (int i = j0 + 6 + tid; i < n; i += LBA_T) {          // the panel below it: row i of L_IJ = A_IJ L_JJ^-T
            double *row = A + (long long)i * n + j0;
            for (int j = 0; j < 6; j++) {
                double s = row[j];
                for (int k = 0; k < j; k++) s -= row[k] * A[(long long)(j0 + j) * n + j0 + k];
                row[j] = s / A[(long long)(j0 + j) * n + j0 + j];
            }
        }
        __syncthreads();
        // the trailing matrix: its lower triangle alone, row r holding the r + 1 entries c <= r.  The thread walks the entries
        // tid, tid + 256, ... of the triangle in row order by stepping (r, c), with no division; both loops end at r == m
        const int m = n - j0 - 6;
        int r = 0, c = tid;
        while (r < m && c > r) { c -= r + 1; r++; }
        while (r < m) {
            const int i = j0 + 6 + r, k = j0 + 6 + c;
            const double *ri = A + (long long)i * n + j0, *rk = A + (long long)k * n + j0;
            double s = A[(long long)i * n + k];
#pragma unroll
            for (int u = 0; u < 6; u++) s -= ri[u] * rk[u];
            A[(long long)i * n + k] = s;
            c += LBA_T;
            while (r < m && c > r) { c -= r + 1; r++; }
        }
        __syncthreads();
    }
    const bool ok = !fail;
    if (ok) {
        for (int J = 0; J < nb; J++) {      // L y = b
            const int j0 = 6 * J;
            if (tid == 0)
                for (int j = 0; j < 6; j++) {
                    double s = b[j0 + j];
                    for (int k = 0; k < j; k++) s -= A[(long long)(j0 + j) * n + j0 + k] * piv[k];
                    piv[j] = s / A[(long long)(j0 + j) * n + j0 + j];
                    b[j0 + j] = piv[j];
                }
            __syncthreads();
            for (int i = j0 + 6 + tid; i < n; i += LBA_T) {
                double s = b[i];
#pragma unroll
                for (int c = 0; c < 6; c++) s -= A[(long long)i * n + j0 + c] * piv[c];
                b[i] = s;
            }
            __syncthreads();
        }
        for (int J = nb - 1; J >= 0; J--) { // L^T x = y
            const int j0 = 6 * J;
            if (tid == 0)
                for (int j = 5; j >= 0; j--) {
                    double s = b[j0 + j];
                    for (int k = j + 1; k < 6; k++) s -= A[(long long)(j0 + k) * n + j0 + j] * piv[k];
                    piv[j] = s / A[(long long)(j0 + j) * n + j0 + j];
                    b[j0 + j] = piv[j];
                }
            __syncthreads();
            for (int i = tid; i < j0; i += LBA_T) {
                double s = b[i];
#pragma unroll
                for (int c = 0; c < 6; c++) s -= A[(long long)(j0 + c) * n + i] * piv[c];
                b[i] = s;
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += LBA_T) d.xp[i] = ok ? b[i] : 0.;
    if (tid == 0) d.out[OUT_OK] = ok ? 1. : 0.;
}
// x_l = Dinv (b_l - B^T x_p), update() into the trial estimates [1 - cur] and every vertex's terms of computeScale.  Thread i:
// point i and key frame i.  A vertex outside the active set, and every vertex when the solve failed, is copied.
__global__ __launch_bounds__(LBA_T) void k_lba_update(LbaDev d, int cur, double lambda)
{
    const long long i = (long long)blockIdx.x * LBA_T + threadIdx.x;
    const bool ok = d.out[OUT_OK] != 0.;
    if (i < d.P) {
        const double *x0 = d.X[cur] + 3 * i;
        double *x1 = d.X[1 - cur] + 3 * i;
        double term = 0;
        if (ok && d.pt_active[i]) {
            double cl[3] = {d.bl[3 * i], d.bl[3 * i + 1], d.bl[3 * i + 2]};
            for (int e = d.edge_off[i]; e < d.edge_off[i + 1]; e++) {
                const int k = d.edge_kf[e];
                if (d.level[e] || !kf_is_free(d, k)) continue;
                lba_sub_Wtx(d.blk + LBA_NBLK * (long long)e + LBA_HPL, d.xp + 6 * (long long)k, cl);
            }
            const double *D = d.Dinv + 9 * i;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double xl = D[3 * j] * cl[0] + D[3 * j + 1] * cl[1] + D[3 * j + 2] * cl[2];
                term += lm_scale_term(xl, d.bl[3 * i + j], lambda);
                x1[j] = x0[j] + xl;
            }
        } else {
            x1[0] = x0[0]; x1[1] = x0[1]; x1[2] = x0[2];
        }
        d.pterm[i] = term;
    }
    if (i < d.NK) {
        const LbaSe3 T = load_se3(d.est[cur] + 7 * i);
        if (i < d.K && ok && d.kf_active[i]) {
            double term = 0;
#pragma unroll
            for (int j = 0; j < 6; j++) term += lm_scale_term(d.xp[6 * i + j], d.bp[6 * i + j], lambda);
            d.kterm[i] = term;
            store_se3(d.est[1 - cur] + 7 * i, lba_pose_oplus(T, d.xp + 6 * i));
        } else {
            if (i < d.K) d.kterm[i] = 0;
            store_se3(d.est[1 - cur] + 7 * i, T);
        }
    }
}
// One workgroup: the sums and counts the host reads after a trial (orbm_opt.h has the trees)
__global__ __launch_bounds__(LBA_RT) void k_lba_reduce_out(LbaDev d)
{
    __shared__ double sh[LBA_RT / 64];
    const int tid = threadIdx.x;
    double chi = 0, scale = 0, scale_p = 0, active = 0, level1 = 0, mx = 0;
    for (long long e = tid; e < d.E; e += LBA_RT) {
        chi += d.chi_e[e];
        if (d.level[e]) level1 += 1.; else active += 1.;
    }
    for (long long k = tid; k < d.K; k += LBA_RT) { scale += d.kterm[k]; mx = fmax(mx, d.kmax[k]); }
    for (long long p = tid; p < d.P; p += LBA_RT) { scale_p += d.pterm[p]; mx = fmax(mx, d.pmax[p]); }
    chi = opt_block_sum<LBA_RT>(chi, sh);
    scale = opt_block_sum<LBA_RT>(scale, sh);
    scale_p = opt_block_sum<LBA_RT>(scale_p, sh);
    active = opt_block_sum<LBA_RT>(active, sh); // counts: exact in double
    level1 = opt_block_sum<LBA_RT>(level1, sh);
    mx = opt_block_max<LBA_RT>(mx, sh);
    if (tid == 0) {
        d.out[OUT_CHI] = chi; d.out[OUT_SCALE] = scale + scale_p; d.out[OUT_MAXDIAG] = mx; d.out[OUT_ACTIVE] = active;
        d.out[OUT_LEVEL1] = level1;
    }
}
// e->chi2() > 5.991 / 7.815 || !e->isDepthPositive() on the stored error and the estimates [cur]: the level (:672-702) or the
// erase flag (:715-743)
__global__ __launch_bounds__(LBA_T) void k_lba_flag(LbaDev d, int cur, int final_pass)
{
    const long long e = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E) return;
    const double err[3] = {d.err[3 * e], d.err[3 * e + 1], d.err[3 * e + 2]};
    const bool bad = lba_chi2(err, (double)d.inv_sigma2[e]) > lba_chi2_threshold(!(d.u_right[e] < 0)) ||
                     !lba_depth_positive(load_se3(d.est[cur] + 7 * (long long)d.edge_kf[e]), d.X[cur] + 3 * (long long)d.edge_pt[e]);
    if (final_pass) d.erase[e] = bad ? 1 : 0;
    else d.level[e] = bad ? 1 : 0;
}
// Converter::toCvMat of the local key frames' estimates and of the points (:762-777)
__global__ __launch_bounds__(LBA_T) void k_lba_output(LbaDev d, int cur)
{
    const long long i = (long long)blockIdx.x * LBA_T + threadIdx.x;
    if (i < d.K) se3_to_Tcw(load_se3(d.est[cur] + 7 * i), d.out_Tcw + 16 * i);
    if (i < d.P)
        for (int j = 0; j < 3; j++) d.out_xw[3 * i + j] = (float)d.X[cur][3 * i + j];
}

// "the passes of a problem" for lm_optimize (orbp_lm_body.h), as kernel launches on the handle's stream (OptGpu, orbm_opt.h)
struct LbaGpu : OptGpu {
    LbaDev d = {};
    const volatile uint8_t *stop_flag = nullptr;
    int robust = LBA_KERNEL_LBA;
    double *spd_y = nullptr;                // orbm_bundle_adjustment: the reduced system goes to orbm_spd_solve_device (orbm_spd.hip),
    int *spd_flag = nullptr;                // whose ok flag lands where k_lba_solve writes its own
    bool stop() const { return status != ORBX_OK || orbp_lba_read_stop(stop_flag); }
    int read_out()                          // the one small block: reduce, copy, synchronise
    {
        prof.pre(s);
        hipLaunchKernelGGL(k_lba_reduce_out, dim3(1), dim3(LBA_RT), 0, s, d);
        return read_back(ORBM_LBA_SPLIT_READ_BACK);
    }
    int activate(int &n_active, int &n_level1)
    {
        prof.pre(s);
        hipLaunchKernelGGL(k_lba_activate, dim3(opt_blocks(std::max(d.P, d.K), LBA_T)), dim3(LBA_T), 0, s, d);
        if (d.E) MHIPCHK(hipMemsetAsync(d.chi_e, 0, sizeof(double) * (size_t)d.E, s));
        if (d.K + d.P) {
            MHIPCHK(hipMemsetAsync(d.kterm, 0, sizeof(double) * (size_t)(d.K + d.P), s));  // kterm, then pterm
            MHIPCHK(hipMemsetAsync(d.kmax, 0, sizeof(double) * (size_t)(d.K + d.P), s));   // kmax, then pmax
        }
        prof.post(ORBM_LBA_SPLIT_SETUP, s);
        MTRY(read_out());
        n_active = (int)pin[OUT_ACTIVE]; n_level1 = (int)pin[OUT_LEVEL1];
        return ORBX_OK;
    }
    int do_linearize(bool first, bool with_errors, double &chi, double &maxdiag)
    {
        if (with_errors) SPLIT_GROUP(prof, ORBM_LBA_SPLIT_ERRORS, s, hipLaunchKernelGGL(k_lba_errors, dim3(opt_blocks(d.E, LBA_T)), dim3(LBA_T), 0, s, d, cur, robust));
        SPLIT_GROUP(prof, ORBM_LBA_SPLIT_LINEARIZE, s, hipLaunchKernelGGL(k_lba_linearize, dim3(opt_blocks(d.E, LBA_T)), dim3(LBA_T), 0, s, d, cur, robust));
        SPLIT_GROUP(prof, ORBM_LBA_SPLIT_REDUCE_POINTS, s, hipLaunchKernelGGL(k_lba_reduce_points, dim3(opt_blocks(d.P, LBA_T)), dim3(LBA_T), 0, s, d));
        if (d.K) SPLIT_GROUP(prof, ORBM_LBA_SPLIT_REDUCE_KFS, s, hipLaunchKernelGGL(k_lba_reduce_kfs, dim3(d.K), dim3(64), 0, s, d));
        MHIPCHK(hipGetLastError());
        if (first || with_errors) {
            MTRY(read_out());
            chi = pin[OUT_CHI]; maxdiag = pin[OUT_MAXDIAG];
        }
        return ORBX_OK;
    }
    int do_trial(double lambda, double &chi, double &scale, bool &ok)
    {
        SPLIT_GROUP(prof, ORBM_LBA_SPLIT_DINV, s, hipLaunchKernelGGL(k_lba_dinv, dim3(opt_blocks(d.P, LBA_T)), dim3(LBA_T), 0, s, d, lambda));
        if (d.K) SPLIT_GROUP(prof, ORBM_LBA_SPLIT_SCHUR, s, hipLaunchKernelGGL(k_lba_schur, dim3(d.K, d.K), dim3(64), 0, s, d, lambda));
        if (spd_y && d.n > 0)
            SPLIT_GROUP(prof, ORBM_LBA_SPLIT_SOLVE, s, MTRY(orbm_spd_solve_device(d.S, d.bs, spd_y, d.xp, spd_flag, d.out + OUT_OK, d.n, s)));
        else                                // without unknowns k_lba_solve only sets the ok flag
            SPLIT_GROUP(prof, ORBM_LBA_SPLIT_SOLVE, s, hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(LBA_T), 0, s, d));
        SPLIT_GROUP(prof, ORBM_LBA_SPLIT_UPDATE, s, hipLaunchKernelGGL(k_lba_update, dim3(opt_blocks(std::max(d.P, d.NK), LBA_T)), dim3(LBA_T), 0, s, d, cur, lambda));
        SPLIT_GROUP(prof, ORBM_LBA_SPLIT_ERRORS, s, hipLaunchKernelGGL(k_lba_errors, dim3(opt_blocks(d.E, LBA_T)), dim3(LBA_T), 0, s, d, 1 - cur, robust));
        MTRY(read_out());                   // checks the launches above as well
        chi = pin[OUT_CHI]; scale = pin[OUT_SCALE]; ok = pin[OUT_OK] != 0.;
        return ORBX_OK;
    }
    void linearize(bool first, bool with_errors, double &chi, double &maxdiag) { if (status == ORBX_OK) status = do_linearize(first, with_errors, chi, maxdiag); }
    void trial(double lambda, double &chi, double &scale, bool &ok) { if (status == ORBX_OK) status = do_trial(lambda, chi, scale, ok); }
};

// What both drivers do between their checks and their first activate(): the CSR by local key frame, the workspace, the upload and
// k_lba_init.  with_spd: also the two parts orbm_spd_solve_device asks for (BundleAdjustment).  `in` outlives the call's orbm_sync().
int lba_setup(orbm_matcher *m, LbaGpu &g, InBlock &in, const orbp_lba_problem *p, const float *xw, const volatile uint8_t *stop,
              bool with_spd, double *split_ms, int32_t *split_count)
{
    LbaDev &d = g.d;
    const int K = p->n_local, NK = p->n_local + p->n_fixed, P = p->n_points, E = p->edge_off[P];
    // CSR by local key frame, edges ascending
    std::vector<int32_t> kf_off((size_t)K + 1, 0), kf_edge;
    for (int e = 0; e < E; e++)
        if (p->edge_kf[e] < K) kf_off[p->edge_kf[e] + 1]++;
    for (int k = 0; k < K; k++) kf_off[k + 1] += kf_off[k];
    kf_edge.resize((size_t)kf_off[K]);
    {
        std::vector<int32_t> at(kf_off.begin(), kf_off.end() - 1);
        for (int e = 0; e < E; e++)
            if (p->edge_kf[e] < K) kf_edge[at[p->edge_kf[e]]++] = e;
    }
    // the workspace: 8-byte parts first
    d.K = K; d.NK = NK; d.P = P; d.E = E; d.n = 6 * K;
    const size_t n = (size_t)d.n, sK = (size_t)K, sNK = (size_t)NK, sP = (size_t)P, sE = (size_t)E;
    WsLayout ws;
    ws.take(d.est[0], 7 * sNK); ws.take(d.est[1], 7 * sNK); ws.take(d.X[0], 3 * sP); ws.take(d.X[1], 3 * sP);
    ws.take(d.err, 3 * sE); ws.take(d.chi_e, sE); ws.take(d.blk, LBA_NBLK * sE); ws.take(d.Hll, 6 * sP);
    ws.take(d.bl, 3 * sP); ws.take(d.Dinv, 9 * sP); ws.take(d.Db, 3 * sP);
    ws.take(d.kmax, sK + sP); ws.take(d.kterm, sK + sP);            // the key frames', then the points': pmax and pterm below
    ws.take(d.Hpp, 21 * sK); ws.take(d.bp, 6 * sK); ws.take(d.S, n * n); ws.take(d.bs, n); ws.take(d.xp, n); ws.take(d.out, 8);
    uint8_t *res = nullptr;
    ws.take(res, 64 * sK + 12 * sP + sE);   // the results back to back: one copy home
    ws.take(d.edge_pt, sE); ws.take(d.table, sK * sP); ws.take(d.level, sE); ws.take(d.kf_active, sK); ws.take(d.pt_active, sP);
    if (with_spd) { ws.take(g.spd_y, n); ws.take(g.spd_flag, 16); }
    MTRY(orbm_ensure_opt(m, ws.bytes()));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    ws.bind(m->d_opt.get());
    d.pmax = d.kmax + K; d.pterm = d.kterm + K;
    d.out_Tcw = (float *)res; d.out_xw = d.out_Tcw + 16 * sK; d.erase = (uint8_t *)(d.out_xw + 3 * sP);
    const int pT = in.add(p->Tcw, 64 * sNK), pc = in.add(p->cam, 20 * sNK), pf = in.add(p->local_fixed, sK), px = in.add(xw, 12 * sP),
              po = in.add(p->edge_off, 4 * (sP + 1)), pk = in.add(p->edge_kf, 4 * sE), pb = in.add(p->obs, 8 * sE),
              pu = in.add(p->u_right, 4 * sE), pi = in.add(p->inv_sigma2, 4 * sE), pko = in.add(kf_off.data(), 4 * (sK + 1)),
              pke = in.add(kf_edge.data(), 4 * kf_edge.size());
    if (split_ms && split_count) g.prof.start(split_ms, split_count, ORBM_LBA_SPLIT_N);
    g.prof.pre(s);
    MTRY(in.upload(s));
    g.prof.post(ORBM_LBA_SPLIT_UPLOAD, s);
    d.Tcw = in.at<float>(pT); d.cam = in.at<float>(pc); d.local_fixed = in.at<uint8_t>(pf); d.xw_in = in.at<float>(px);
    d.edge_off = in.dev_at<int32_t>(po); d.edge_kf = in.at<int32_t>(pk); d.obs = in.at<float>(pb); d.u_right = in.at<float>(pu);
    d.inv_sigma2 = in.at<float>(pi); d.kf_off = in.dev_at<int32_t>(pko); d.kf_edge = in.at<int32_t>(pke);
    g.m = m; g.s = s; g.stop_flag = stop; g.pin = (double *)m->opt_pin.get(); g.out = d.out;
    g.prof.pre(s);
    if (sK * sP) MHIPCHK(hipMemsetAsync(d.table, 0xFF, 4 * sK * sP, s));
    MHIPCHK(hipMemsetAsync(d.out, 0, 64, s));
    hipLaunchKernelGGL(k_lba_init, dim3(opt_blocks(std::max(std::max(NK, P), E), LBA_T)), dim3(LBA_T), 0, s, d);
    MHIPCHK(hipGetLastError());
    g.prof.post(ORBM_LBA_SPLIT_SETUP, s);
    return ORBX_OK;
}

// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778): two rounds, the flagging passes, three result parts
int lba_run(orbm_matcher *m, const orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase, const volatile uint8_t *stop,
            orbp_lba_stats *stats, double *split_ms, int32_t *split_count)
{
    char text[200];
    if (orbp_lba_check(p, Tcw_local, xw, erase, text, (int)sizeof text) != ORBX_OK) return mfail(ORBX_E_INVALID, "%s", text);
    if (orbp_lba_read_stop(stop)) return ORBP_LBA_STOPPED;          // :655-657: nothing is launched
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // k_lba_solve is one workgroup: its time grows with the cube of 6 K and a call runs it up to 150 times (DESIGN.md section 22
    // has the time at the cap)
    if ((long long)p->n_local * p->n_points > (1ll << 28) || p->n_local > ORBM_LBA_MAX_LOCAL)
        return mfail(ORBX_E_CAPACITY, "request beyond %d local key frames / 2^28 table entries", ORBM_LBA_MAX_LOCAL);
    InBlock in(m); LbaGpu g;
    MTRY(lba_setup(m, g, in, p, xw, stop, false, split_ms, split_count));
    const LbaDev &d = g.d; hipStream_t s = g.s;
    orbp_lba_stats st;
    memset(&st, 0, sizeof st);
    LmRun run = {0, 0, 0, 0};
    int n_active = 0, n_level1 = 0;
    MTRY(g.activate(n_active, n_level1));                       // :659
    if (n_active > 0) {
        lm_optimize(g, 5, run);                                 // :660
        MTRY(g.status);
        st.iterations[0] = run.iterations; st.trials[0] = run.trials; st.lambda = run.lambda; st.chi2 = run.chi2;
    }
    if (!orbp_lba_read_stop(stop)) {                            // :662-709
        st.second_round = 1;
        SPLIT_GROUP(g.prof, ORBM_LBA_SPLIT_FLAG_OUTPUT, s, hipLaunchKernelGGL(k_lba_flag, dim3(opt_blocks(d.E, LBA_T)), dim3(LBA_T), 0, s, d, g.cur, 0));
        g.robust = LBA_KERNEL_NONE;
        MTRY(g.activate(n_active, n_level1));                   // :706
        st.n_level1 = n_level1;
        if (n_active > 0) {
            lm_optimize(g, 10, run);                            // :707
            MTRY(g.status);
            st.iterations[1] = run.iterations; st.trials[1] = run.trials; st.lambda = run.lambda; st.chi2 = run.chi2;
        }
    }
    g.prof.pre(s);
    hipLaunchKernelGGL(k_lba_flag, dim3(opt_blocks(d.E, LBA_T)), dim3(LBA_T), 0, s, d, g.cur, 1);          // :715-743
    hipLaunchKernelGGL(k_lba_output, dim3(opt_blocks(std::max(d.K, d.P), LBA_T)), dim3(LBA_T), 0, s, d, g.cur);     // :762-777
    MHIPCHK(hipGetLastError());
    g.prof.post(ORBM_LBA_SPLIT_FLAG_OUTPUT, s);
    MTRY(g.download({Tcw_local, xw, erase}, {64 * (size_t)d.K, 12 * (size_t)d.P, (size_t)d.E}, d.out_Tcw, ORBM_LBA_SPLIT_DOWNLOAD));
    if (stats) *stats = st;
    return ORBP_LBA_DONE;
}

// Optimizer::BundleAdjustment (src/Optimizer.cc:49-237): one round with the call's robust kind, the many-workgroup solve of
// orbm_spd.hip in place of k_lba_solve, two result parts
int ba_run(orbm_matcher *m, const orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local, float *xw,
           const volatile uint8_t *stop, orbp_ba_stats *stats, double *split_ms, int32_t *split_count)
{
    char text[200];                                             // no entry check of `stop` (src/Optimizer.cc:49-188 has none)
    if (orbp_ba_check(p, n_iterations, Tcw_local, xw, text, (int)sizeof text) != ORBX_OK) return mfail(ORBX_E_INVALID, "%s", text);
    // decided from the counts, before the handle is touched
    if (p->n_local > ORBM_BA_MAX_KFS || (long long)p->n_local * p->n_points > ORBM_BA_MAX_TABLE)
        return mfail(ORBX_E_CAPACITY, "bundle_adjustment: beyond %d key frames / %d entries of the key frame x point table", ORBM_BA_MAX_KFS,
                     ORBM_BA_MAX_TABLE);
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    InBlock in(m); LbaGpu g;
    MTRY(lba_setup(m, g, in, p, xw, stop, true, split_ms, split_count));
    const LbaDev &d = g.d; hipStream_t s = g.s;
    LmRun run = {0, 0, 0, 0};                                   // src/Optimizer.cc:187-235
    int n_active = 0, n_level1 = 0;
    g.robust = robust ? LBA_KERNEL_BA : LBA_KERNEL_NONE;
    MTRY(g.activate(n_active, n_level1));                       // :187
    if (n_active > 0) {
        lm_optimize(g, n_iterations, run);                      // :188
        MTRY(g.status);
    }
    SPLIT_GROUP(g.prof, ORBM_LBA_SPLIT_FLAG_OUTPUT, s,            // a point without edges keeps its bits: float -> double -> float
              hipLaunchKernelGGL(k_lba_output, dim3(opt_blocks(std::max(d.K, d.P), LBA_T)), dim3(LBA_T), 0, s, d, g.cur));
    MHIPCHK(hipGetLastError());
    MTRY(g.download({Tcw_local, xw}, {64 * (size_t)d.K, 12 * (size_t)d.P}, d.out_Tcw, ORBM_LBA_SPLIT_DOWNLOAD));
    if (stats) *stats = {run.iterations, run.trials, run.lambda, run.chi2};
    return ORBX_OK;
}
}   // namespace

extern "C" int orbm_local_bundle_adjustment(orbm_matcher *m, const orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase,
                                            const volatile uint8_t *stop, orbp_lba_stats *stats)
{
    return lba_run(m, p, Tcw_local, xw, erase, stop, stats, nullptr, nullptr);
}
extern "C" int orbm_local_bundle_adjustment_split(orbm_matcher *m, const orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase,
                                                  const volatile uint8_t *stop, orbp_lba_stats *stats, double *split_ms,
                                                  int32_t *split_count)
{
    if (!split_ms || !split_count) return mfail(ORBX_E_INVALID, "local_bundle_adjustment_split: NULL split_ms or split_count");
    return lba_run(m, p, Tcw_local, xw, erase, stop, stats, split_ms, split_count);
}
extern "C" int orbm_bundle_adjustment(orbm_matcher *m, const orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local, float *xw,
                                      const volatile uint8_t *stop, orbp_ba_stats *stats)
{
    return ba_run(m, p, n_iterations, robust, Tcw_local, xw, stop, stats, nullptr, nullptr);
}
extern "C" int orbm_bundle_adjustment_split(orbm_matcher *m, const orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local,
                                            float *xw, const volatile uint8_t *stop, orbp_ba_stats *stats, double *split_ms,
                                            int32_t *split_count)
{
    if (!split_ms || !split_count) return mfail(ORBX_E_INVALID, "bundle_adjustment_split: NULL split_ms or split_count");
    return ba_run(m, p, n_iterations, robust, Tcw_local, xw, stop, stats, split_ms, split_count);
}
