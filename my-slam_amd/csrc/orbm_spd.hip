// orbm_spd.hip -- a dense symmetric positive definite solve in fp64 over many workgroups: orbm_spd_solve_f64 (include/orbm.h) and
// orbm_spd_solve_device, which orbm_bundle_adjustment (orbm_lba.hip) runs on the reduced system S of its Schur complement where
// orbm_local_bundle_adjustment runs the one-workgroup k_lba_solve.
//
// A = L L^T by panels of SPD_NB columns, right-looking, in place in the lower triangle of the row-major n x n A (the upper triangle
// is neither read nor written), then L y = b and L^T x = y panel by panel.  Plain launches in stream order:
//   per panel J (columns j0 .. j0 + nb, nb = min(SPD_NB, n - j0))
//     k_spd_diag     one workgroup: the diagonal block in LDS, factored column by column; a pivot that is not positive or not
//                    finite sets the solve's flag
//     k_spd_panel    one workgroup per 64 rows below the block: L_IJ = A_IJ L_JJ^-T, L_JJ and the rows in LDS, one thread a row
//     k_spd_update   one workgroup per SPD_NB x SPD_NB tile (I, K), K <= I, of the trailing lower triangle:
//                    A_IK -= L_IJ L_KJ^T, both factors in LDS, a thread owns 3 x 3 entries and adds the panel's columns in
//                    ascending order
//   per panel J ascending    k_spd_forward: every workgroup solves L_JJ y_J = b_J in LDS (the same arithmetic in each), workgroup 0
//                            stores y_J, and workgroup w subtracts L_IJ y_J from its 64 rows of b below the block
//   per panel J descending   k_spd_backward: every workgroup solves L_JJ^T x_J = y_J, workgroup 0 stores x_J, and workgroup w
//                            subtracts L_JI^T x_J from its 256 entries of y above the block
// That is 5 launches a panel: 5 ceil(n / SPD_NB) - 2 for a solve (the last panel has no rows below it), and one 4-byte memset.
//
// Kept because the machines are shared (DESIGN.md sections 22 and 23): no cooperative launch, no grid-wide barrier, no spin-wait,
// nothing between workgroups but kernel boundaries, no atomic.  Every loop is bounded by n.  The flag is a word of device memory:
// every later launch of the solve reads it first and returns at once when it is set (k_spd_backward then writes zeros into its part
// of x, so a failed solve leaves x all zeros, as k_lba_solve does); there is no trap and no host read-back between the panels.
// Every sum runs in an order fixed by (n, SPD_NB) alone, so x is a function of (A, b): not of the handle's history, not of the
// number of workgroups that happen to run together.
//
// SPD_NB = 48: a multiple of 6 (8 key frames a panel), two 48 x 49 fp64 tiles are 37 KB of the 160 KB of LDS (four workgroups a CU
// by LDS), and at n = 3072 the first trailing update is 2016 tiles for 256 CUs.  A wider panel makes k_spd_diag, the one
// single-workgroup step, longer; a narrower one adds launches, which dominate below n of about 1000.
#include "orbm_internal.h"
#include "ws_layout.h"
#include "../../include/orbm.h"

#define SPD_NB 48
#define SPD_LD 49                   // LDS row stride in doubles: odd, so rows 3 apart fall into different banks
#define SPD_PR 64                   // rows a workgroup of k_spd_panel / k_spd_forward
#define SPD_BC 256                  // entries a workgroup of k_spd_backward

namespace {
struct SpdDev {
    double *A, *b, *y, *x;          // n x n row-major (lower triangle), the right-hand side (overwritten), L^-1 b, the solution
    int *flag;                      // != 0: a pivot failed
    double *ok_out;                 // may be NULL: 1.0 / 0.0 once the last launch of the solve has run
    int n;
};

// the nb x nb block at (j0, j0): its lower triangle into LDS (row stride SPD_LD)
__device__ __forceinline__ void spd_load_diag(const SpdDev &d, int j0, int nb, double *L, int nthreads)
{
    for (int i = threadIdx.x; i < nb * nb; i += nthreads) {
        const int r = i / nb, c = i - r * nb;
        L[r * SPD_LD + c] = c <= r ? d.A[(long long)(j0 + r) * d.n + j0 + c] : 0.;
    }
}

__global__ __launch_bounds__(256) void k_spd_diag(SpdDev d, int j0, int nb)
{
    __shared__ double L[SPD_NB * SPD_LD];
    __shared__ int fail;
    if (*d.flag) return;
    const int tid = threadIdx.x;
    if (tid == 0) fail = 0;
    spd_load_diag(d, j0, nb, L, 256);
    __syncthreads();
    for (int j = 0; j < nb; j++) {
        if (tid == 0) {
            const double v = L[j * SPD_LD + j];
            if (!(v > 0) || !isfinite(v)) fail = 1;
            else L[j * SPD_LD + j] = sqrt(v);
        }
        __syncthreads();
        if (fail) break;                                    // read after the barrier: the whole workgroup leaves together
        if (tid > j && tid < nb) L[tid * SPD_LD + j] /= L[j * SPD_LD + j];
        __syncthreads();
        // the block's trailing triangle: entry (r, c), j < c <= r < nb, over the threads
        const int m = nb - j - 1;
        for (int i = tid; i < m * m; i += 256) {
            const int r = j + 1 + i / m, c = j + 1 + i % m;
            if (c <= r) L[r * SPD_LD + c] -= L[r * SPD_LD + j] * L[c * SPD_LD + j];
        }
        __syncthreads();
    }
    if (fail) {
        if (tid == 0) *d.flag = 1;
        return;
    }
    for (int i = tid; i < nb * nb; i += 256) {
        const int r = i / nb, c = i - r * nb;
        if (c <= r) d.A[(long long)(j0 + r) * d.n + j0 + c] = L[r * SPD_LD + c];
    }
}

// rows j0 + nb + 64 w .. of the panel: row = (row - its earlier entries . L_JJ's row) / pivot, entry by entry
__global__ __launch_bounds__(SPD_PR) void k_spd_panel(SpdDev d, int j0, int nb)
{
    __shared__ double L[SPD_NB * SPD_LD];
    __shared__ double R[SPD_PR * SPD_LD];
    if (*d.flag) return;
    const int tid = threadIdx.x, n = d.n;
    const int i0 = j0 + nb + SPD_PR * (int)blockIdx.x, rows = min(SPD_PR, n - i0);
    spd_load_diag(d, j0, nb, L, SPD_PR);
    for (int i = tid; i < rows * nb; i += SPD_PR) {
        const int r = i / nb, c = i - r * nb;
        R[r * SPD_LD + c] = d.A[(long long)(i0 + r) * n + j0 + c];
    }
    __syncthreads();
    if (tid < rows) {
        double *row = R + tid * SPD_LD;
        for (int j = 0; j < nb; j++) {
            double s = row[j];
            for (int k = 0; k < j; k++) s -= row[k] * L[j * SPD_LD + k];
            row[j] = s / L[j * SPD_LD + j];
        }
    }
    __syncthreads();
    for (int i = tid; i < rows * nb; i += SPD_PR) {
        const int r = i / nb, c = i - r * nb;
        d.A[(long long)(i0 + r) * n + j0 + c] = R[r * SPD_LD + c];
    }
}

// tile t of the trailing lower triangle, tiles numbered row by row: (0,0) (1,0) (1,1) (2,0) ...; rows i0 .., columns k0 .. <= rows
__global__ __launch_bounds__(256) void k_spd_update(SpdDev d, int j0, int nb)
{
    __shared__ double P[SPD_NB * SPD_LD];                   // L_IJ
    __shared__ double Q[SPD_NB * SPD_LD];                   // L_KJ
    if (*d.flag) return;
    const int tid = threadIdx.x, n = d.n, base = j0 + nb;
    int ti = 0, t = (int)blockIdx.x;
    while (t > ti) { t -= ti + 1; ti++; }                   // at most ceil(n / SPD_NB) steps
    const int i0 = base + SPD_NB * ti, k0 = base + SPD_NB * t;
    const int ri = min(SPD_NB, n - i0), rk = min(SPD_NB, n - k0);
    for (int i = tid; i < SPD_NB * nb; i += 256) {
        const int r = i / nb, c = i - r * nb;
        P[r * SPD_LD + c] = r < ri ? d.A[(long long)(i0 + r) * n + j0 + c] : 0.;
        Q[r * SPD_LD + c] = r < rk ? d.A[(long long)(k0 + r) * n + j0 + c] : 0.;
    }
    __syncthreads();
    const int r0 = 3 * (tid >> 4), c0 = 3 * (tid & 15);
    double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int k = 0; k < nb; k++) {
        const double a0 = P[r0 * SPD_LD + k], a1 = P[(r0 + 1) * SPD_LD + k], a2 = P[(r0 + 2) * SPD_LD + k];
        const double b0 = Q[c0 * SPD_LD + k], b1 = Q[(c0 + 1) * SPD_LD + k], b2 = Q[(c0 + 2) * SPD_LD + k];
        // explicit fma: the build keeps a * b + c unfused (-ffp-contract=off), and this loop is the solve's arithmetic
        acc[0][0] = fma(a0, b0, acc[0][0]); acc[0][1] = fma(a0, b1, acc[0][1]); acc[0][2] = fma(a0, b2, acc[0][2]);
        acc[1][0] = fma(a1, b0, acc[1][0]); acc[1][1] = fma(a1, b1, acc[1][1]); acc[1][2] = fma(a1, b2, acc[1][2]);
        acc[2][0] = fma(a2, b0, acc[2][0]); acc[2][1] = fma(a2, b1, acc[2][1]); acc[2][2] = fma(a2, b2, acc[2][2]);
    }
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const int i = i0 + r0 + u, k = k0 + c0 + v;
            if (r0 + u < ri && c0 + v < rk && k <= i) d.A[(long long)i * n + k] -= acc[u][v];
        }
}

// L_JJ v = rhs (transposed == 0) or L_JJ^T v = rhs (transposed != 0) in LDS by one wave's worth of threads: v[] holds rhs on
// entry and the solution on return.  Thread t owns v[t] and subtracts the solved unknowns from it in the order they are solved.
__device__ __forceinline__ void spd_tri_solve(const double *L, double *v, int nb, bool transposed)
{
    const int t = threadIdx.x;
    for (int s = 0; s < nb; s++) {
        const int j = transposed ? nb - 1 - s : s;
        if (t == j) v[j] /= L[j * SPD_LD + j];
        __syncthreads();
        if (t < nb && (transposed ? t < j : t > j)) v[t] -= (transposed ? L[j * SPD_LD + t] : L[t * SPD_LD + j]) * v[j];
        __syncthreads();
    }
}

__global__ __launch_bounds__(SPD_PR) void k_spd_forward(SpdDev d, int j0, int nb)
{
    __shared__ double L[SPD_NB * SPD_LD];
    __shared__ double v[SPD_NB];
    if (*d.flag) return;
    const int tid = threadIdx.x, n = d.n;
    spd_load_diag(d, j0, nb, L, SPD_PR);
    if (tid < nb) v[tid] = d.b[j0 + tid];
    __syncthreads();
    spd_tri_solve(L, v, nb, false);
    if (blockIdx.x == 0 && tid < nb) d.y[j0 + tid] = v[tid];
    const int i = j0 + nb + SPD_PR * (int)blockIdx.x + tid;
    if (i < n) {
        const double *row = d.A + (long long)i * n + j0;
        double s = d.b[i];
        for (int c = 0; c < nb; c++) s -= row[c] * v[c];
        d.b[i] = s;
    }
}

__global__ __launch_bounds__(SPD_BC) void k_spd_backward(SpdDev d, int j0, int nb)
{
    __shared__ double L[SPD_NB * SPD_LD];
    __shared__ double v[SPD_NB];
    const int tid = threadIdx.x, n = d.n;
    const bool failed = *d.flag != 0;
    if (blockIdx.x == 0 && j0 == 0 && tid == 0 && d.ok_out) *d.ok_out = failed ? 0. : 1.;
    if (failed) {
        if (blockIdx.x == 0 && tid < nb) d.x[j0 + tid] = 0.;
        return;
    }
    spd_load_diag(d, j0, nb, L, SPD_BC);
    if (tid < nb) v[tid] = d.y[j0 + tid];
    __syncthreads();
    spd_tri_solve(L, v, nb, true);
    if (blockIdx.x == 0 && tid < nb) d.x[j0 + tid] = v[tid];
    const int i = SPD_BC * (int)blockIdx.x + tid;
    if (i < j0) {
        double s = d.y[i];
        for (int r = 0; r < nb; r++) s -= d.A[(long long)(j0 + r) * n + i] * v[r];
        d.y[i] = s;
    }
}
}   // namespace

namespace {
void spd_factor(const SpdDev &d, hipStream_t s)
{
    const int n = d.n;
    for (int j0 = 0; j0 < n; j0 += SPD_NB) {
        const int nb = std::min(SPD_NB, n - j0), m = n - j0 - nb;
        hipLaunchKernelGGL(k_spd_diag, dim3(1), dim3(256), 0, s, d, j0, nb);
        if (m > 0) {
            const int tiles = (m + SPD_NB - 1) / SPD_NB;
            hipLaunchKernelGGL(k_spd_panel, dim3((m + SPD_PR - 1) / SPD_PR), dim3(SPD_PR), 0, s, d, j0, nb);
            hipLaunchKernelGGL(k_spd_update, dim3(tiles * (tiles + 1) / 2), dim3(256), 0, s, d, j0, nb);
        }
    }
}
void spd_substitute(const SpdDev &d, hipStream_t s)
{
    const int n = d.n;
    for (int j0 = 0; j0 < n; j0 += SPD_NB) {
        const int nb = std::min(SPD_NB, n - j0), m = n - j0 - nb;
        hipLaunchKernelGGL(k_spd_forward, dim3(std::max((m + SPD_PR - 1) / SPD_PR, 1)), dim3(SPD_PR), 0, s, d, j0, nb);
    }
    for (int j0 = (n - 1) / SPD_NB * SPD_NB; j0 >= 0; j0 -= SPD_NB) {
        const int nb = std::min(SPD_NB, n - j0);
        hipLaunchKernelGGL(k_spd_backward, dim3(std::max((j0 + SPD_BC - 1) / SPD_BC, 1)), dim3(SPD_BC), 0, s, d, j0, nb);
    }
}
}   // namespace

// The device routine: A (n x n, row-major, its lower triangle), b, y, x, flag and ok_out (may be NULL) are device memory; A, b
// and y are overwritten.  Everything is enqueued on s; nothing is read back.
int orbm_spd_solve_device(double *A, double *b, double *y, double *x, int *flag, double *ok_out, int n, hipStream_t s)
{
    const SpdDev d = {A, b, y, x, flag, ok_out, n};
    MHIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));
    spd_factor(d, s);
    spd_substitute(d, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

// For tools/bench_ba.py alone (not in include/orbm.h): the device routine `reps` times on one uploaded system, each time from a
// fresh device copy of A and b, timed by events on the handle's stream.  ms[0] = the factorisation, ms[1] = both substitutions:
// medians over the repetitions.  Nothing else about the solve differs.
extern "C" int orbm_spd_solve_timed(orbm_matcher *m, const double *A, const double *b, int n, int reps, double *ms)
{
    if (!A || !b || !ms || n < 1 || n > ORBM_SPD_MAX_N || reps < 1 || reps > 1000)
        return mfail(ORBX_E_INVALID, "spd_solve_timed: bad argument");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    const size_t sn = (size_t)n, nn = sn * sn * sizeof(double);
    SpdDev d = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n};
    double *dA0 = nullptr, *db0 = nullptr;  // the uploaded system: every repetition starts from a copy of it
    WsLayout ws;
    ws.take(d.A, sn * sn); ws.take(dA0, sn * sn); ws.take(d.b, sn); ws.take(db0, sn); ws.take(d.y, sn); ws.take(d.x, sn); ws.take(d.flag, 16);
    MTRY(orbm_ensure_opt(m, ws.bytes()));
    hipStream_t s = m->stream;
    ws.bind(m->d_opt.get());
    MHIPCHK(hipMemcpyAsync(dA0, A, nn, hipMemcpyHostToDevice, s));
    MHIPCHK(hipMemcpyAsync(db0, b, sn * sizeof(double), hipMemcpyHostToDevice, s));
    hipEvent_t ev[3];
    for (int i = 0; i < 3; i++) MHIPCHK(hipEventCreate(&ev[i]));
    std::vector<float> tf, ts;
    int rc = ORBX_OK;
    for (int r = 0; r < reps && rc == ORBX_OK; r++) {
        hipError_t e = hipMemcpyAsync(d.A, dA0, nn, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d.b, db0, sn * sizeof(double), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(d.flag, 0, sizeof(int), s);
        if (e == hipSuccess) e = hipEventRecord(ev[0], s);
        spd_factor(d, s);
        if (e == hipSuccess) e = hipEventRecord(ev[1], s);
        spd_substitute(d, s);
        if (e == hipSuccess) e = hipEventRecord(ev[2], s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        float a = 0, c = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&a, ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&c, ev[1], ev[2]);
        if (e != hipSuccess) rc = mfail(ORBX_E_HIP, "spd_solve_timed: %s", hipGetErrorString(e));
        tf.push_back(a); ts.push_back(c);
    }
    for (int i = 0; i < 3; i++) (void)hipEventDestroy(ev[i]);
    MTRY(rc);
    std::sort(tf.begin(), tf.end()); std::sort(ts.begin(), ts.end());
    ms[0] = tf[tf.size() / 2]; ms[1] = ts[ts.size() / 2];
    return ORBX_OK;
}

extern "C" int orbm_spd_solve_f64(orbm_matcher *m, const double *A, const double *b, int n, double *x, int *ok)
{
    if (!A || !b || !x || !ok) return mfail(ORBX_E_INVALID, "spd_solve: NULL argument");
    if (n < 1) return mfail(ORBX_E_INVALID, "spd_solve: n = %d", n);
    if (n > ORBM_SPD_MAX_N) return mfail(ORBX_E_CAPACITY, "spd_solve: n = %d beyond %d", n, ORBM_SPD_MAX_N);
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    const size_t sn = (size_t)n;
    SpdDev d = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n};
    WsLayout ws;
    ws.take(d.A, sn * sn); ws.take(d.b, sn); ws.take(d.y, sn); ws.take(d.x, sn); ws.take(d.flag, 16);
    MTRY(orbm_ensure_opt(m, ws.bytes()));
    hipStream_t s = m->stream;
    ws.bind(m->d_opt.get());
    MHIPCHK(hipMemcpyAsync(d.A, A, sn * sn * sizeof(double), hipMemcpyHostToDevice, s));
    MHIPCHK(hipMemcpyAsync(d.b, b, sn * sizeof(double), hipMemcpyHostToDevice, s));
    MTRY(orbm_spd_solve_device(d.A, d.b, d.y, d.x, d.flag, nullptr, n, s));
    int failed = 0;
    MHIPCHK(hipMemcpyAsync(x, d.x, sn * sizeof(double), hipMemcpyDeviceToHost, s));
    MHIPCHK(hipMemcpyAsync(&failed, d.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    MHIPCHK(hipStreamSynchronize(s));
    *ok = failed ? 0 : 1;
    return ORBX_OK;
}
