// orbp_epnp_body.h -- the arithmetic of one PnPsolver hypothesis (src/PnPsolver.cc:312-957 of WChen09/My-SLAM), one text for the
// host solver (orbp.cc, plain C++) and for the kernel (orbm_pnp.hip): epnp_compute_pose() is PnPsolver::compute_pose on n
// correspondences, epnp_check_one() is one correspondence of CheckInliers.
//
// Host and device agree byte for byte because the body uses only + - * / sqrt on float and double (correctly rounded on both
// sides; the build's -ffp-contract=off keeps the compilers from fusing them), its own abs and max, and every sum in one written
// order.  Nothing here allocates: the 12 x 12 eigen-problem, the small SVDs and the Gauss-Newton systems live in an EpnpWork the
// caller provides (the stack on the host, a wave-private piece of LDS in the kernel), the per-point arrays (pws, us, alphas, pcs)
// are the caller's too: fixed arrays of ORBM_PNP_MAX_SET points for a RANSAC sample, heap vectors for Refine's n-point solve.
//
// What OpenCV does inside cv::SVD / cvInvert / cvSolve is not pinned: a one-sided Jacobi stands in for it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EPNP_HD __host__ __device__ __forceinline__
#define EPNP_UNROLL _Pragma("unroll")
#else
#define EPNP_HD static inline
#define EPNP_UNROLL
#endif

#ifndef ORBM_PNP_MAX_SET
#define ORBM_PNP_MAX_SET 8          // include/orbm.h: the largest sample the kernel takes
#endif
#define EPNP_DBL_EPSILON 2.2204460492503131e-16
#define EPNP_SVD_SWEEPS 60

// scratch of one solve; every array is indexed at run time, so none of it may end up in registers or private memory on the GPU
struct EpnpWork {
    double B[144], V[144], vt[144];     // the Jacobi's working copy of M^T M, its V, and the sorted eigenvectors as rows
    double w[12];                        // column norms before sorting
    int order[12];
    double L[60];                        // L_6x10
    double sA[30], sB[30], sU[30], sV[25], sW[5];      // the small SVDs (3 x 3 and 6 x {3, 4, 5}) and their solves
    double dv[72];                       // compute_L_6x10's differences [4][6][3]
    double gA[24];                       // the 6 x 4 Gauss-Newton system
    double W12[12], cc[9], ci[9], eye[9], sx[5], rho[6];      // what the solves above read and write through run-time indices
};

EPNP_HD double epnp_abs(double x) { return x < 0 ? -x : x; }
EPNP_HD double epnp_max(double a, double b) { return a < b ? b : a; }       // std::max(a, b)
EPNP_HD double epnp_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
EPNP_HD double epnp_dist2_3(const double *a, const double *b)
{
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// One-sided (Hestenes) Jacobi SVD of the m x n matrix in B (row-major, m >= n, destroyed): A = U diag(W) V^T, W descending in the
// stable order (equal values keep their column order), U m x n (skipped when NULL), Vout n x n: column k is the k-th right vector
// when !transposed, row k when transposed.  Columns of U that belong to a zero singular value are left zero.  V (n x n), w and
// order are scratch.
EPNP_HD void epnp_jacobi_svd(double *B, int m, int n, double *U, double *W, double *V, double *Vout, bool transposed, double *w, int *order)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j;
    for (int sweep = 0; sweep < EPNP_SVD_SWEEPS; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double a = 0, b = 0, g = 0;
                for (int i = 0; i < m; i++) {
                    const double x = B[i * n + p], y = B[i * n + q];
                    a += x * x; b += y * y; g += x * y;
                }
                if (epnp_abs(g) <= EPNP_DBL_EPSILON * __builtin_sqrt(a * b) || g == 0.0) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (epnp_abs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
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
    for (int j = 0; j < n; j++) {
        double s = 0;
        for (int i = 0; i < m; i++) s += B[i * n + j] * B[i * n + j];
        w[j] = __builtin_sqrt(s);
    }
    // stable descending order: an insertion sort that moves an index only past strictly smaller values
    for (int j = 0; j < n; j++) {
        int k = j;
        while (k > 0 && w[j] > w[order[k - 1]]) { order[k] = order[k - 1]; k--; }
        order[k] = j;
    }
    for (int k = 0; k < n; k++) {
        const int j = order[k];
        W[k] = w[j];
        if (U)
            for (int i = 0; i < m; i++) U[i * n + k] = w[j] > 0 ? B[i * n + j] / w[j] : 0.0;
        if (transposed)
            for (int i = 0; i < n; i++) Vout[k * n + i] = V[i * n + j];
        else
            for (int i = 0; i < n; i++) Vout[i * n + k] = V[i * n + j];
    }
}

// x = pinv(A) b through the SVD, singular values below 2 eps sum(w) dropped (cvSolve / cvInvert with CV_SVD).  A: m x n, m <= 6,
// n <= 5, copied into wk.sB; b: m x nrhs; x: n x nrhs.
EPNP_HD void epnp_svd_solve(const double *A, int m, int n, const double *b, int nrhs, double *x, EpnpWork &wk)
{
    double *U = wk.sU, *W = wk.sW, *V = wk.sV;
    for (int i = 0; i < m * n; i++) wk.sB[i] = A[i];
    epnp_jacobi_svd(wk.sB, m, n, U, W, wk.V, V, false, wk.w, wk.order);
    double thr = 0;
    for (int i = 0; i < n; i++) thr += W[i];
    thr *= 2 * EPNP_DBL_EPSILON;
    for (int r = 0; r < nrhs; r++) {
        for (int i = 0; i < n; i++) x[i * nrhs + r] = 0;
        for (int k = 0; k < n; k++) {
            if (!(W[k] > thr)) continue;
            double s = 0;
            for (int i = 0; i < m; i++) s += U[i * n + k] * b[i * nrhs + r];
            s /= W[k];
            for (int i = 0; i < n; i++) x[i * nrhs + r] += V[i * n + k] * s;
        }
    }
}

// Householder QR least squares for the 6 x 4 Gauss-Newton system (PnPsolver.cc:878-957: scaled columns, R's diagonal kept
// aside).  Returns false on a zero column, which leaves x untouched like the reference's early return.
EPNP_HD bool epnp_qr_solve_6x4(double *A, double *b, double *x)
{
    const int nr = 6, nc = 4;
    double a1[4], a2[4];
    EPNP_UNROLL
    for (int k = 0; k < nc; k++) {
        double eta = 0;
        for (int i = k; i < nr; i++) eta = epnp_max(eta, epnp_abs(A[i * nc + k]));
        if (eta == 0) return false;
        double sum = 0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) { A[i * nc + k] *= inv_eta; sum += A[i * nc + k] * A[i * nc + k]; }
        double sigma = __builtin_sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        a1[k] = sigma * A[k * nc + k];
        a2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s = 0;
            for (int i = k; i < nr; i++) s += A[i * nc + k] * A[i * nc + j];
            const double tau = s / a1[k];
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    EPNP_UNROLL
    for (int j = 0; j < nc; j++) {          // b <- Q^T b
        double tau = 0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= a1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    x[nc - 1] = b[nc - 1] / a2[nc - 1];     // back substitution
    EPNP_UNROLL
    for (int i = nc - 2; i >= 0; i--) {
        double s = 0;
        for (int j = i + 1; j < nc; j++) s += A[i * nc + j] * x[j];
        x[i] = (b[i] - s) / a2[i];
    }
    return true;
}

// the problem of one solve: n correspondences in the caller's arrays (pws 3n, us 2n in; alphas 4n, pcs 3n scratch)
struct EpnpProblem {
    double fu, fv, uc, vc;
    int n;
    const double *pws, *us;
    double *alphas, *pcs;
    double cws[4][3], ccs[4][3];
};

EPNP_HD void epnp_choose_control_points(EpnpProblem &e, EpnpWork &wk)             // :346-384
{
    const int n = e.n;
    for (int j = 0; j < 3; j++) e.cws[0][j] = 0;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) e.cws[0][j] += e.pws[3 * i + j];
    for (int j = 0; j < 3; j++) e.cws[0][j] /= n;
    double *c = wk.sB;
    for (int j = 0; j < 9; j++) c[j] = 0;
    for (int i = 0; i < n; i++) {
        double d[3];
        for (int j = 0; j < 3; j++) d[j] = e.pws[3 * i + j] - e.cws[0][j];
        for (int r = 0; r < 3; r++)
            for (int s = 0; s < 3; s++) c[3 * r + s] += d[r] * d[s];
    }
    double *W = wk.sW, *V = wk.sV;
    epnp_jacobi_svd(c, 3, 3, wk.sU, W, wk.V, V, false, wk.w, wk.order);        // symmetric PSD: V holds the principal axes
    for (int i = 1; i < 4; i++) {
        // The sign of a principal axis is the SVD routine's choice (OpenCV's in the reference) and, with noisy
        // points, changes which local minimum the betas reach.  Fixed here: largest component positive.
        int big = 0;
        for (int j = 1; j < 3; j++)
            if (epnp_abs(V[3 * j + (i - 1)]) > epnp_abs(V[3 * big + (i - 1)])) big = j;
        const double sgn = V[3 * big + (i - 1)] < 0 ? -1.0 : 1.0;
        const double k = sgn * __builtin_sqrt(W[i - 1] / n);
        for (int j = 0; j < 3; j++) e.cws[i][j] = e.cws[0][j] + k * V[3 * j + (i - 1)];
    }
}

EPNP_HD void epnp_compute_barycentric_coordinates(EpnpProblem &e, EpnpWork &wk)   // :386-412
{
    double *cc = wk.cc, *ci = wk.ci, *eye = wk.eye;
    for (int i = 0; i < 9; i++) eye[i] = (i & 3) == 0;
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = e.cws[j][i] - e.cws[0][i];
    epnp_svd_solve(cc, 3, 3, eye, 3, ci, wk);     // pseudo-inverse (cvInvert CV_SVD)
    for (int i = 0; i < e.n; i++) {
        const double *pi = &e.pws[3 * i];
        double *a = &e.alphas[4 * i];
        for (int j = 0; j < 3; j++)
            a[1 + j] = ci[3 * j] * (pi[0] - e.cws[0][0]) + ci[3 * j + 1] * (pi[1] - e.cws[0][1]) + ci[3 * j + 2] * (pi[2] - e.cws[0][2]);
        a[0] = 1.0f - a[1] - a[2] - a[3];
    }
}

EPNP_HD void epnp_compute_ccs(EpnpProblem &e, const double *betas, const double *vt)    // :431-444; vt row r = r-th singular vector
{
    for (int i = 0; i < 4; i++) e.ccs[i][0] = e.ccs[i][1] = e.ccs[i][2] = 0.0;
    for (int i = 0; i < 4; i++) {
        const double *v = vt + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) e.ccs[j][k] += betas[i] * v[3 * j + k];
    }
}

EPNP_HD void epnp_compute_pcs(EpnpProblem &e)                        // :446-456
{
    for (int i = 0; i < e.n; i++) {
        const double *a = &e.alphas[4 * i];
        for (int j = 0; j < 3; j++)
            e.pcs[3 * i + j] = a[0] * e.ccs[0][j] + a[1] * e.ccs[1][j] + a[2] * e.ccs[2][j] + a[3] * e.ccs[3][j];
    }
}

EPNP_HD void epnp_solve_for_sign(EpnpProblem &e)                     // :610-624
{
    if (e.pcs[2] < 0.0) {
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 3; j++) e.ccs[i][j] = -e.ccs[i][j];
        for (int i = 0; i < 3 * e.n; i++) e.pcs[i] = -e.pcs[i];
    }
}

EPNP_HD double epnp_reprojection_error(const EpnpProblem &e, const double *R, const double *t)     // :528-546; R row-major
{
    double sum = 0.0;
    for (int i = 0; i < e.n; i++) {
        const double *pw = &e.pws[3 * i];
        const double Xc = epnp_dot3(R, pw) + t[0], Yc = epnp_dot3(R + 3, pw) + t[1];
        const double inv_Zc = 1.0 / (epnp_dot3(R + 6, pw) + t[2]);
        const double ue = e.uc + e.fu * Xc * inv_Zc, ve = e.vc + e.fv * Yc * inv_Zc;
        const double u = e.us[2 * i], v = e.us[2 * i + 1];
        sum += __builtin_sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum / e.n;
}

EPNP_HD void epnp_estimate_R_and_t(const EpnpProblem &e, EpnpWork &wk, double *R, double *t)     // :548-601 (absolute orientation, Arun et al.)
{
    const int n = e.n;
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) { pc0[j] += e.pcs[3 * i + j]; pw0[j] += e.pws[3 * i + j]; }
    for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
    double *abt = wk.sB;
    for (int j = 0; j < 9; j++) abt[j] = 0;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) abt[3 * j + k] += (e.pcs[3 * i + j] - pc0[j]) * (e.pws[3 * i + k] - pw0[k]);
    double *U = wk.sU, *W = wk.sW, *V = wk.sV;
    epnp_jacobi_svd(abt, 3, 3, U, W, wk.V, V, false, wk.w, wk.order);
    if (!(W[2] > 2 * EPNP_DBL_EPSILON * (W[0] + W[1] + W[2]))) {
        // rank-deficient (coplanar points): complete U to an orthonormal basis.  In OpenCV's Jacobi SVD the third
        // left vector is what rounding noise leaves after orthogonalisation against the other two, i.e. +-(u1 x u2)
        // with a sign nobody chose; the reference is implementation-defined here.
        const double a[3] = {U[0], U[3], U[6]}, b[3] = {U[1], U[4], U[7]};
        U[2] = a[1] * b[2] - a[2] * b[1]; U[5] = a[2] * b[0] - a[0] * b[2]; U[8] = a[0] * b[1] - a[1] * b[0];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] -
                       R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int j = 0; j < 3; j++) t[j] = pc0[j] - epnp_dot3(R + 3 * j, pw0);
}

EPNP_HD double epnp_compute_R_and_t(EpnpProblem &e, EpnpWork &wk, const double *betas, double *R, double *t)     // :626-637
{
    epnp_compute_ccs(e, betas, wk.vt);
    epnp_compute_pcs(e);
    epnp_solve_for_sign(e);
    epnp_estimate_R_and_t(e, wk, R, t);
    return epnp_reprojection_error(e, R, t);
}

// betas10 = [B11 B12 B22 B13 B23 B33 B14 B24 B34 B44]; the three linearisations :639-757.  cols: the first nc entries of
// {0, 1, 3, 6} (which == 1), {0, 1, 2} (2) or {0, 1, 2, 3, 4} (3).
EPNP_HD void epnp_sub_solve(EpnpWork &wk, const double *rho, int which, int nc, double *out)
{
    double *A = wk.sA;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < nc; j++) {
            const int col = which == 1 ? (j == 2 ? 3 : j == 3 ? 6 : j) : j;
            A[i * nc + j] = wk.L[10 * i + col];
        }
    epnp_svd_solve(A, 6, nc, rho, 1, out, wk);
}
EPNP_HD void epnp_find_betas_approx_1(EpnpWork &wk, const double *rho, double *betas)
{
    double *b4 = wk.sx;
    epnp_sub_solve(wk, rho, 1, 4, b4);
    if (b4[0] < 0) {
        betas[0] = __builtin_sqrt(-b4[0]);
        betas[1] = -b4[1] / betas[0]; betas[2] = -b4[2] / betas[0]; betas[3] = -b4[3] / betas[0];
    } else {
        betas[0] = __builtin_sqrt(b4[0]);
        betas[1] = b4[1] / betas[0]; betas[2] = b4[2] / betas[0]; betas[3] = b4[3] / betas[0];
    }
}
EPNP_HD void epnp_find_betas_approx_2(EpnpWork &wk, const double *rho, double *betas)
{
    double *b3 = wk.sx;
    epnp_sub_solve(wk, rho, 2, 3, b3);
    if (b3[0] < 0) {
        betas[0] = __builtin_sqrt(-b3[0]);
        betas[1] = (b3[2] < 0) ? __builtin_sqrt(-b3[2]) : 0.0;
    } else {
        betas[0] = __builtin_sqrt(b3[0]);
        betas[1] = (b3[2] > 0) ? __builtin_sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) betas[0] = -betas[0];
    betas[2] = 0.0; betas[3] = 0.0;
}
EPNP_HD void epnp_find_betas_approx_3(EpnpWork &wk, const double *rho, double *betas)
{
    double *b5 = wk.sx;
    epnp_sub_solve(wk, rho, 3, 5, b5);
    if (b5[0] < 0) {
        betas[0] = __builtin_sqrt(-b5[0]);
        betas[1] = (b5[2] < 0) ? __builtin_sqrt(-b5[2]) : 0.0;
    } else {
        betas[0] = __builtin_sqrt(b5[0]);
        betas[1] = (b5[2] > 0) ? __builtin_sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) betas[0] = -betas[0];
    betas[2] = b5[3] / betas[0];
    betas[3] = 0.0;
}

EPNP_HD void epnp_compute_L_6x10(EpnpWork &wk)      // :760-801; dv[i][j][k] at wk.dv[18 i + 3 j + k]
{
    for (int i = 0; i < 4; i++) {
        const double *v = wk.vt + 12 * (11 - i);
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            for (int k = 0; k < 3; k++) wk.dv[18 * i + 3 * j + k] = v[3 * a + k] - v[3 * b + k];
            if (++b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; i++) {
        double *row = wk.L + 10 * i;
        const double *d0 = wk.dv + 3 * i, *d1 = wk.dv + 18 + 3 * i, *d2 = wk.dv + 36 + 3 * i, *d3 = wk.dv + 54 + 3 * i;
        row[0] = epnp_dot3(d0, d0);
        row[1] = 2.0f * epnp_dot3(d0, d1);
        row[2] = epnp_dot3(d1, d1);
        row[3] = 2.0f * epnp_dot3(d0, d2);
        row[4] = 2.0f * epnp_dot3(d1, d2);
        row[5] = epnp_dot3(d2, d2);
        row[6] = 2.0f * epnp_dot3(d0, d3);
        row[7] = 2.0f * epnp_dot3(d1, d3);
        row[8] = 2.0f * epnp_dot3(d2, d3);
        row[9] = epnp_dot3(d3, d3);
    }
}

EPNP_HD void epnp_gauss_newton(EpnpWork &wk, const double *rho, double *be)      // :813-876
{
    for (int k = 0; k < 5; k++) {
        double *A = wk.gA, b[6], x[4] = {0, 0, 0, 0};
    EPNP_UNROLL
        for (int i = 0; i < 6; i++) {
            const double *r = wk.L + 10 * i;
            double *a = A + 4 * i;
            a[0] = 2 * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3];
            a[1] = r[1] * be[0] + 2 * r[2] * be[1] + r[4] * be[2] + r[7] * be[3];
            a[2] = r[3] * be[0] + r[4] * be[1] + 2 * r[5] * be[2] + r[8] * be[3];
            a[3] = r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + 2 * r[9] * be[3];
            b[i] = rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] + r[3] * be[0] * be[2] +
                             r[4] * be[1] * be[2] + r[5] * be[2] * be[2] + r[6] * be[0] * be[3] + r[7] * be[1] * be[3] +
                             r[8] * be[2] * be[3] + r[9] * be[3] * be[3]);
        }
        if (!epnp_qr_solve_6x4(A, b, x)) continue;    // singular column: the reference leaves X as it was
        for (int i = 0; i < 4; i++) be[i] += x[i];
    }
}

// PnPsolver::compute_pose (:458-508): R (9, row-major) and t of the linearisation with the least mean reprojection error, which
// is returned.  e.fu .. e.vc, e.n and the four array pointers are the input.
EPNP_HD double epnp_compute_pose(EpnpProblem &e, EpnpWork &wk, double *R, double *t)
{
    epnp_choose_control_points(e, wk);
    epnp_compute_barycentric_coordinates(e, wk);
    double *mtm = wk.B;
    for (int i = 0; i < 144; i++) mtm[i] = 0;
    for (int i = 0; i < e.n; i++) {        // rows of M (:414-429) accumulated straight into M^T M
        const double *as = &e.alphas[4 * i];
        const double u = e.us[2 * i], v = e.us[2 * i + 1];
        double *m1 = wk.sA, *m2 = wk.sA + 12;
        for (int j = 0; j < 4; j++) {
            m1[3 * j] = as[j] * e.fu; m1[3 * j + 1] = 0.0; m1[3 * j + 2] = as[j] * (e.uc - u);
            m2[3 * j] = 0.0; m2[3 * j + 1] = as[j] * e.fv; m2[3 * j + 2] = as[j] * (e.vc - v);
        }
        for (int r = 0; r < 12; r++)
            for (int c = 0; c < 12; c++) mtm[12 * r + c] += m1[r] * m1[c] + m2[r] * m2[c];
    }
    // symmetric PSD: eigenvectors = columns of V, eigenvalues descending; vt holds them as rows
    epnp_jacobi_svd(mtm, 12, 12, nullptr, wk.W12, wk.V, wk.vt, true, wk.w, wk.order);
    double *rho = wk.rho;
    epnp_compute_L_6x10(wk);
    rho[0] = epnp_dist2_3(e.cws[0], e.cws[1]); rho[1] = epnp_dist2_3(e.cws[0], e.cws[2]); rho[2] = epnp_dist2_3(e.cws[0], e.cws[3]);
    rho[3] = epnp_dist2_3(e.cws[1], e.cws[2]); rho[4] = epnp_dist2_3(e.cws[1], e.cws[3]); rho[5] = epnp_dist2_3(e.cws[2], e.cws[3]);
    double betas[4], Rk[9], tk[3];
    epnp_find_betas_approx_1(wk, rho, betas); epnp_gauss_newton(wk, rho, betas);
    double best = epnp_compute_R_and_t(e, wk, betas, R, t);
    epnp_find_betas_approx_2(wk, rho, betas); epnp_gauss_newton(wk, rho, betas);
    double err = epnp_compute_R_and_t(e, wk, betas, Rk, tk);
    if (err < best) { best = err; for (int i = 0; i < 9; i++) R[i] = Rk[i]; for (int i = 0; i < 3; i++) t[i] = tk[i]; }
    epnp_find_betas_approx_3(wk, rho, betas); epnp_gauss_newton(wk, rho, betas);
    err = epnp_compute_R_and_t(e, wk, betas, Rk, tk);
    if (err < best) { best = err; for (int i = 0; i < 9; i++) R[i] = Rk[i]; for (int i = 0; i < 3; i++) t[i] = tk[i]; }
    return best;
}

// One correspondence of PnPsolver::CheckInliers (:312-344), with its float / double mix: Ri (9, row-major) and ti are mRi / mti,
// X is the world point, u the undistorted keypoint, max_err = mvMaxError[i].
EPNP_HD bool epnp_check_one(const double *Ri, const double *ti, double fu, double fv, double uc, double vc, const float *Xw, const float *uv,
                            float max_err)
{
    const float X = Xw[0], Y = Xw[1], Z = Xw[2];
    const float Xc = (float)(Ri[0] * X + Ri[1] * Y + Ri[2] * Z + ti[0]);
    const float Yc = (float)(Ri[3] * X + Ri[4] * Y + Ri[5] * Z + ti[1]);
    const float invZc = (float)(1 / (Ri[6] * X + Ri[7] * Y + Ri[8] * Z + ti[2]));
    const double ue = uc + fu * Xc * invZc;
    const double ve = vc + fv * Yc * invZc;
    const float dx = (float)(uv[0] - ue), dy = (float)(uv[1] - ve);
    const float error2 = dx * dx + dy * dy;
    return error2 < max_err;
}
