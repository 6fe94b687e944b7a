// orbm_eg.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044 of WChen09/My-SLAM, on g2o) on the GPU:
// orbm_optimize_essential_graph (include/orbm.h) over the flat problem of orbp_optimize_essential_graph (include/orbp.h).  Host and
// kernels run one text for the edges (orbp_eg_body.h); the host drives lba_optimize (orbp_lba_body.h) with launches as its passes,
// as orbm_bundle_adjustment does, and the 7N x 7N system goes to the many-workgroup solve of orbm_spd.hip.
//
//   once          k_eg_measure     a thread an edge: Sji = Sjw * Swi from Scw or Snc (:857-867, :889-972)
//   an iteration  k_eg_linearize   32 lanes an edge, 8 edges a workgroup: lane k < 29 evaluates entry k of the numeric
//                                  linearisation (one exp and one log each; a fixed vertex's 14 are skipped), the errors meet in
//                                  LDS, then the lanes write e (7), J_i and J_j (7 x 7 each) and e . e
//                 k_eg_diag        a wave a free vertex: H_vv (lower triangle) and b_v over its edges in edge order
//                 k_eg_offdiag     a wave a pair of free vertices that share edges: their 7 x 7 block, in edge order, into the
//                                  lower triangle of the dense row-major H0
//   a trial       k_eg_stage       the lower triangle of H0 + lambda I into the work matrix, b beside it
//                 orbm_spd_solve_device
//                 k_eg_update      a thread a vertex: the trial's estimate Sim3(x_v) * estimate into the other buffer
//                 k_eg_errors      a thread an edge: e . e at the trial's estimates
//                 k_eg_reduce_out  one workgroup: chi2 and computeScale's x . (lambda x + b), each a fixed tree, into the 64 bytes
//                                  the host reads
//   at the end    k_eg_output, k_eg_points, one copy home
// H0 is zeroed once a call: the graph does not change, so every iteration rewrites the same blocks.  The estimates are double
// buffered ([cur] and the trial's), so accept is a flip and reject nothing.
//
// Kept because the machines are shared (DESIGN.md sections 22 to 24): plain launches in stream order, no cooperative launch, no
// grid-wide barrier, no spin-wait, nothing between workgroups but kernel boundaries, no atomic; every loop is bounded by a count
// known at launch; a failed pivot leaves x = 0 through the solve's flag and nothing traps.
#include "orbm_internal.h"
#include "orbm_prof.h"
#include "orbp_internal.h"
#include "orbp_eg_body.h"
#include "orbp_lba_body.h"
#include "../../include/orbp.h"
#include "../../include/orbm.h"

#define EG_T 256
#define EG_RT 1024
#define EG_EPB 8                    // edges a workgroup of k_eg_linearize: 32 lanes each

static_assert(7 * ORBM_EG_MAX_KFS <= ORBM_SPD_MAX_N, "the unknowns of a call stay inside the solve's tested range");

namespace {
struct EgDev {
    int n, fixed, nf, N, E, P, npairs, fix_scale;   // key frames, the fixed one or -1, free ones, 7 nf, edges, points, pairs
    // the problem and the host's tables
    const double *Scw, *Snc;
    const int32_t *edge_i, *edge_j, *ref;
    const uint8_t *edge_corrected;
    const float *xw_in;
    const int32_t *free_of;                         // key frame -> its place among the free ones, or -1
    const int32_t *vtx_off, *vtx_edge;              // CSR key frame -> incident edges, ascending
    const int32_t *pair_off, *pair_edge, *pair_hi, *pair_lo;   // CSR pair -> its edges, ascending; the free places, hi > lo
    // state
    double *meas, *est[2];                          // 8 doubles an edge / a key frame
    double *err, *Ji, *Jj, *chi_e;                  // 7, 49, 49, 1 an edge
    double *H0, *b0, *W, *bw, *y, *x;               // N x N, N, N x N, N, N, N
    double *out;                                    // 8: chi2, scale, ok
    float *out_Tcw, *out_xw;
    double *out_S;
};
enum { OUT_CHI = 0, OUT_SCALE = 1, OUT_OK = 2 };

__device__ __forceinline__ double eg_wave_sum(double a)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
    return a;
}
__device__ __forceinline__ double eg_block_sum(double a, double *sh)
{
    a = eg_wave_sum(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    for (int s = EG_RT / 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(EG_T) void k_eg_measure(EgDev d)
{
    const int e = blockIdx.x * EG_T + threadIdx.x;
    if (e >= d.E) return;
    const double *S = d.edge_corrected[e] ? d.Scw : d.Snc;
    eg_store(d.meas + 8 * (long long)e, s3o_mul(eg_load(S + 8 * (long long)d.edge_j[e]), s3o_inverse(eg_load(S + 8 * (long long)d.edge_i[e]))));
}

// The axis of a lane is data, not an unrolled index: a thread holds one perturbed estimate, never the 29 of its edge
__global__ __launch_bounds__(EG_T) void k_eg_linearize(EgDev d, int cur)
{
    __shared__ double sh[EG_EPB][EG_NLIN][7];
    const int g = threadIdx.x >> 5, lane = threadIdx.x & 31;
    const long long e = (long long)blockIdx.x * EG_EPB + g;
    const bool edge = e < d.E;
    if (edge && lane < EG_NLIN) {
        const int vi = d.edge_i[e], vj = d.edge_j[e];
        const bool wanted = lane == 0 || (lane < 15 ? d.free_of[vi] >= 0 : d.free_of[vj] >= 0);
        double r[7] = {0, 0, 0, 0, 0, 0, 0};
        if (wanted)
            eg_lin_error(eg_load(d.meas + 8 * e), eg_load(d.est[cur] + 8 * (long long)vi), eg_load(d.est[cur] + 8 * (long long)vj), lane,
                         d.fix_scale != 0, r);
#pragma unroll
        for (int j = 0; j < 7; j++) sh[g][lane][j] = r[j];
    }
    __syncthreads();
    if (!edge) return;
    for (int idx = lane; idx < 7 + 98; idx += 32) {
        if (idx < 7) d.err[7 * e + idx] = sh[g][0][idx];
        else {
            const int q = idx - 7, side = q / 49, rd = q - 49 * side, r = rd / 7, ax = rd - 7 * r;
            (side ? d.Jj : d.Ji)[49 * e + rd] = eg_jac(sh[g][14 * side + 1 + 2 * ax][r], sh[g][14 * side + 2 + 2 * ax][r]);
        }
    }
    if (lane == 0) d.chi_e[e] = eg_chi2(sh[g][0]);
}

// free place f -> its key frame: at most one key frame is fixed
__device__ __forceinline__ int eg_vertex_of(const EgDev &d, int f) { return d.fixed >= 0 && f >= d.fixed ? f + 1 : f; }

__global__ __launch_bounds__(64) void k_eg_diag(EgDev d)
{
    const int f = blockIdx.x, v = eg_vertex_of(d, f), l = threadIdx.x;
    if (l >= 56) return;
    const int a = l < 49 ? l / 7 : l - 49, c = l < 49 ? l - 7 * a : 0;
    if (l < 49 && c > a) return;
    double acc = 0;
    for (int q = d.vtx_off[v]; q < d.vtx_off[v + 1]; q++) {
        const long long e = d.vtx_edge[q];
        const double *J = (d.edge_i[e] == v ? d.Ji : d.Jj) + 49 * e;
        acc += l < 49 ? eg_h_term(J, J, a, c) : eg_b_term(J, d.err + 7 * e, a);
    }
    if (l < 49) d.H0[(long long)(7 * f + a) * d.N + 7 * f + c] = acc;
    else d.b0[7 * f + a] = acc;
}

__global__ __launch_bounds__(64) void k_eg_offdiag(EgDev d)
{
    const int pr = blockIdx.x, l = threadIdx.x;
    if (l >= 49) return;
    const int hi = d.pair_hi[pr], lo = d.pair_lo[pr], a = l / 7, c = l - 7 * a;
    double acc = 0;
    for (int q = d.pair_off[pr]; q < d.pair_off[pr + 1]; q++) {
        const long long e = d.pair_edge[q];
        const bool i_rows = d.free_of[d.edge_i[e]] == hi;
        acc += eg_h_term((i_rows ? d.Ji : d.Jj) + 49 * e, (i_rows ? d.Jj : d.Ji) + 49 * e, a, c);
    }
    d.H0[(long long)(7 * hi + a) * d.N + 7 * lo + c] = acc;
}

// row blockIdx.y, columns 256 blockIdx.x ..: the lower triangle alone (the solve reads nothing else)
__global__ __launch_bounds__(EG_T) void k_eg_stage(EgDev d, double lambda)
{
    const int r = blockIdx.y, c = blockIdx.x * EG_T + threadIdx.x;
    if (c > r) return;
    const long long at = (long long)r * d.N + c;
    d.W[at] = c == r ? d.H0[at] + lambda : d.H0[at];
    if (c == r) d.bw[r] = d.b0[r];
}

// push + oplus (types_seven_dof_expmap.h:60-69) into the other buffer; the fixed key frame is carried over
__global__ __launch_bounds__(EG_T) void k_eg_update(EgDev d, int cur)
{
    const int v = blockIdx.x * EG_T + threadIdx.x;
    if (v >= d.n) return;
    S3oSim S = eg_load(d.est[cur] + 8 * (long long)v);
    const int f = d.free_of[v];
    if (f >= 0) {
        double u[7];
#pragma unroll
        for (int j = 0; j < 7; j++) u[j] = d.x[7 * f + j];
        S = s3o_oplus(S, u, d.fix_scale != 0);
    }
    eg_store(d.est[1 - cur] + 8 * (long long)v, S);
}

__global__ __launch_bounds__(EG_T) void k_eg_errors(EgDev d, int which)
{
    const long long e = (long long)blockIdx.x * EG_T + threadIdx.x;
    if (e >= d.E) return;
    double err[7];
    eg_error(eg_load(d.meas + 8 * e), eg_load(d.est[which] + 8 * (long long)d.edge_i[e]),
             s3o_inverse(eg_load(d.est[which] + 8 * (long long)d.edge_j[e])), err);
    d.chi_e[e] = eg_chi2(err);
}

__global__ __launch_bounds__(EG_RT) void k_eg_reduce_out(EgDev d, double lambda)
{
    __shared__ double sh[EG_RT / 64];
    const int tid = threadIdx.x;
    double chi = 0, scale = 0;
    for (int e = tid; e < d.E; e += EG_RT) chi += d.chi_e[e];
    for (int i = tid; i < d.N; i += EG_RT) scale += lba_scale_term(d.x[i], d.b0[i], lambda);
    chi = eg_block_sum(chi, sh);
    scale = eg_block_sum(scale, sh);
    if (tid == 0) { d.out[OUT_CHI] = chi; d.out[OUT_SCALE] = scale; }
}

__global__ __launch_bounds__(EG_T) void k_eg_output(EgDev d, int cur)
{
    const int v = blockIdx.x * EG_T + threadIdx.x;
    if (v >= d.n) return;
    const S3oSim S = eg_load(d.est[cur] + 8 * (long long)v);
    eg_to_Tcw(S, d.out_Tcw + 16 * (long long)v);
    eg_store(d.out_S + 8 * (long long)v, S);
}
__global__ __launch_bounds__(EG_T) void k_eg_points(EgDev d, int cur)
{
    const long long q = (long long)blockIdx.x * EG_T + threadIdx.x;
    if (q >= d.P) return;
    float x[3] = {d.xw_in[3 * q], d.xw_in[3 * q + 1], d.xw_in[3 * q + 2]};
    const int r = d.ref[q];
    if (r >= 0) eg_correct_point(eg_load(d.Scw + 8 * (long long)r), eg_load(d.est[cur] + 8 * (long long)r), x);
    d.out_xw[3 * q] = x[0]; d.out_xw[3 * q + 1] = x[1]; d.out_xw[3 * q + 2] = x[2];
}

inline unsigned eg_blocks(long long n, int per = EG_T) { return (unsigned)std::max<long long>((n + per - 1) / per, 1); }

// "the passes of a problem" for lba_optimize (orbp_lba_body.h), as kernel launches on the handle's stream
struct EgGpu {
    EgDev d;
    hipStream_t s;
    int cur = 0, status = ORBX_OK;
    double *pin, *spd_y;
    int *spd_flag;
    double chi2_initial = 0;
    SplitProf prof;

    bool stop() const { return status != ORBX_OK; }
    int read_out(double lambda)             // the one small block: reduce, copy, synchronise
    {
        prof.pre(s);
        hipLaunchKernelGGL(k_eg_reduce_out, dim3(1), dim3(EG_RT), 0, s, d, lambda);
        MHIPCHK(hipGetLastError());
        MHIPCHK(hipMemcpyAsync(pin, d.out, 64, hipMemcpyDeviceToHost, s));
        prof.post(ORBM_EG_SPLIT_READ_BACK, s);
        MHIPCHK(hipStreamSynchronize(s));
        prof.drain();
        return ORBX_OK;
    }
    int errors_now(double &chi)             // computeActiveErrors + activeChi2 at the current estimates
    {
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_UPDATE_ERRORS, s, hipLaunchKernelGGL(k_eg_errors, dim3(eg_blocks(d.E)), dim3(EG_T), 0, s, d, cur));
        MTRY(read_out(0.));
        chi = pin[OUT_CHI];
        return ORBX_OK;
    }
    int do_linearize(bool first, bool with_errors, double &chi)
    {
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_LINEARIZE, s, hipLaunchKernelGGL(k_eg_linearize, dim3(eg_blocks(d.E, EG_EPB)), dim3(EG_T), 0, s, d, cur));
        prof.pre(s);
        hipLaunchKernelGGL(k_eg_diag, dim3(d.nf), dim3(64), 0, s, d);
        if (d.npairs) hipLaunchKernelGGL(k_eg_offdiag, dim3(d.npairs), dim3(64), 0, s, d);
        prof.post(ORBM_EG_SPLIT_ASSEMBLE, s);
        MHIPCHK(hipGetLastError());
        if (first || with_errors) {
            MTRY(read_out(0.));
            if (with_errors) chi = pin[OUT_CHI];
            if (first) chi2_initial = pin[OUT_CHI];
        }
        return ORBX_OK;
    }
    int do_trial(double lambda, double &chi, double &scale, bool &ok)
    {
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_STAGE, s, hipLaunchKernelGGL(k_eg_stage, dim3(eg_blocks(d.N), d.N), dim3(EG_T), 0, s, d, lambda));
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_SOLVE, s, MTRY(orbm_spd_solve_device(d.W, d.bw, spd_y, d.x, spd_flag, d.out + OUT_OK, d.N, s)));
        prof.pre(s);
        hipLaunchKernelGGL(k_eg_update, dim3(eg_blocks(d.n)), dim3(EG_T), 0, s, d, cur);
        hipLaunchKernelGGL(k_eg_errors, dim3(eg_blocks(d.E)), dim3(EG_T), 0, s, d, 1 - cur);
        prof.post(ORBM_EG_SPLIT_UPDATE_ERRORS, s);
        MHIPCHK(hipGetLastError());
        MTRY(read_out(lambda));
        chi = pin[OUT_CHI]; scale = pin[OUT_SCALE]; ok = pin[OUT_OK] != 0.;
        return ORBX_OK;
    }
    // a failed launch or copy ends the loop through stop() and comes back as the call's status
    void linearize(bool first, bool with_errors, double &chi, double &maxdiag)
    {
        maxdiag = 0;                        // computeLambdaInit returns the user's value
        if (status == ORBX_OK) status = do_linearize(first, with_errors, chi);
    }
    void trial(double lambda, double &chi, double &scale, bool &ok) { if (status == ORBX_OK) status = do_trial(lambda, chi, scale, ok); }
    void accept() { cur ^= 1; }
    void reject() {}
};

int eg_run(orbm_matcher *m, const orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw, double *Scw_out, orbp_eg_stats *stats,
           double *split_ms, int32_t *split_count)
{
    char text[200];
    if (orbp_eg_check(p, n_iterations, Tcw, xw, text, (int)sizeof text) != ORBX_OK) return mfail(ORBX_E_INVALID, "%s", text);
    // decided from the counts, before the handle is touched
    if (p->n_kfs > ORBM_EG_MAX_KFS)
        return mfail(ORBX_E_CAPACITY, "optimize_essential_graph: %d key frames beyond %d", p->n_kfs, ORBM_EG_MAX_KFS);
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    const int n = p->n_kfs, E = p->n_edges, P = p->n_points;
    // the free key frames renumbered densely; CSR key frame -> edges and pair of free key frames -> edges, both in edge order
    std::vector<int32_t> free_of((size_t)n, -1), vtx_off((size_t)n + 1, 0), vtx_edge(2 * (size_t)E);
    int nf = 0;
    for (int k = 0; k < n; k++)
        if (k != p->fixed) free_of[k] = nf++;
    for (int e = 0; e < E; e++) { vtx_off[p->edge_i[e] + 1]++; vtx_off[p->edge_j[e] + 1]++; }
    for (int k = 0; k < n; k++) vtx_off[k + 1] += vtx_off[k];
    {
        std::vector<int32_t> at(vtx_off.begin(), vtx_off.end() - 1);
        for (int e = 0; e < E; e++) { vtx_edge[at[p->edge_i[e]]++] = e; vtx_edge[at[p->edge_j[e]]++] = e; }
    }
    std::vector<int32_t> pair_off(1, 0), pair_edge, pair_hi, pair_lo;
    {
        std::vector<std::pair<long long, int32_t>> keyed;       // (hi * nf + lo, edge): sorted, a pair's edges stay ascending
        for (int e = 0; e < E; e++) {
            const int a = free_of[p->edge_i[e]], c = free_of[p->edge_j[e]];
            if (a >= 0 && c >= 0) keyed.push_back({(long long)std::max(a, c) * nf + std::min(a, c), e});
        }
        std::sort(keyed.begin(), keyed.end());
        for (size_t i = 0; i < keyed.size(); i++) {
            if (i == 0 || keyed[i].first != keyed[i - 1].first) {
                if (i) pair_off.push_back((int32_t)i);
                pair_hi.push_back((int32_t)(keyed[i].first / nf)); pair_lo.push_back((int32_t)(keyed[i].first % nf));
            }
            pair_edge.push_back(keyed[i].second);
        }
        pair_off.push_back((int32_t)keyed.size());
    }
    const int npairs = (int)pair_hi.size();

    EgDev d = {};
    d.n = n; d.fixed = p->fixed; d.nf = nf; d.N = 7 * nf; d.E = E; d.P = P; d.npairs = npairs; d.fix_scale = p->fix_scale;
    size_t need = 0;
    auto take = [&need](size_t bytes) { const size_t at = need; need += (bytes + 63) & ~(size_t)63; return at; };
    const size_t N = (size_t)d.N, szd = sizeof(double);
    const size_t o_meas = take(8 * szd * E), o_est0 = take(8 * szd * n), o_est1 = take(8 * szd * n), o_err = take(7 * szd * E),
                 o_Ji = take(49 * szd * E), o_Jj = take(49 * szd * E), o_chi = take(szd * E), o_H0 = take(szd * N * N),
                 o_b0 = take(szd * N), o_W = take(szd * N * N), o_bw = take(szd * N), o_y = take(szd * N), o_x = take(szd * N),
                 o_out = take(64), o_flag = take(64),
                 o_res = take(64 * (size_t)n + 64 * (size_t)n + 12 * (size_t)P);     // the results back to back: one copy home
    MTRY(orbm_ensure_lba(m, need));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    uint8_t *w = m->d_lba;
    d.meas = (double *)(w + o_meas); d.est[0] = (double *)(w + o_est0); d.est[1] = (double *)(w + o_est1); d.err = (double *)(w + o_err);
    d.Ji = (double *)(w + o_Ji); d.Jj = (double *)(w + o_Jj); d.chi_e = (double *)(w + o_chi); d.H0 = (double *)(w + o_H0);
    d.b0 = (double *)(w + o_b0); d.W = (double *)(w + o_W); d.bw = (double *)(w + o_bw); d.y = (double *)(w + o_y);
    d.x = (double *)(w + o_x); d.out = (double *)(w + o_out);
    d.out_S = (double *)(w + o_res); d.out_Tcw = (float *)(d.out_S + 8 * (size_t)n); d.out_xw = d.out_Tcw + 16 * (size_t)n;

    InBlock in(m);
    const int pS = in.add(p->Scw, 64 * (size_t)n), pN = in.add(p->Snc, 64 * (size_t)n), pi = in.add(p->edge_i, 4 * (size_t)E),
              pj = in.add(p->edge_j, 4 * (size_t)E), pc = in.add(p->edge_corrected, (size_t)E), pr = in.add(p->ref, 4 * (size_t)P),
              px = in.add(xw, 12 * (size_t)P), pf = in.add(free_of.data(), 4 * (size_t)n), pvo = in.add(vtx_off.data(), 4 * ((size_t)n + 1)),
              pve = in.add(vtx_edge.data(), 4 * vtx_edge.size()), ppo = in.add(pair_off.data(), 4 * pair_off.size()),
              ppe = in.add(pair_edge.data(), 4 * pair_edge.size()), pph = in.add(pair_hi.data(), 4 * (size_t)npairs),
              ppl = in.add(pair_lo.data(), 4 * (size_t)npairs);
    EgGpu g;
    if (split_ms && split_count) g.prof.start(split_ms, split_count, ORBM_EG_SPLIT_N);
    g.prof.pre(s);
    MTRY(in.upload(s));
    d.Scw = in.at<double>(pS); d.Snc = in.at<double>(pN); d.edge_i = in.at<int32_t>(pi); d.edge_j = in.at<int32_t>(pj);
    d.edge_corrected = in.at<uint8_t>(pc); d.ref = in.at<int32_t>(pr); d.xw_in = in.at<float>(px); d.free_of = in.at<int32_t>(pf);
    d.vtx_off = in.dev_at<int32_t>(pvo); d.vtx_edge = in.at<int32_t>(pve); d.pair_off = in.dev_at<int32_t>(ppo);
    d.pair_edge = in.at<int32_t>(ppe); d.pair_hi = in.at<int32_t>(pph); d.pair_lo = in.at<int32_t>(ppl);
    if (N) MHIPCHK(hipMemsetAsync(d.H0, 0, szd * N * N, s));
    if (N) MHIPCHK(hipMemsetAsync(d.x, 0, szd * N, s));
    MHIPCHK(hipMemsetAsync(d.out, 0, 64, s));
    if (n) MHIPCHK(hipMemcpyAsync(d.est[0], d.Scw, 64 * (size_t)n, hipMemcpyDeviceToDevice, s));
    if (E) hipLaunchKernelGGL(k_eg_measure, dim3(eg_blocks(E)), dim3(EG_T), 0, s, d);
    MHIPCHK(hipGetLastError());
    g.prof.post(ORBM_EG_SPLIT_UPLOAD, s);

    g.d = d; g.s = s; g.pin = (double *)m->lba_pin.get(); g.spd_y = d.y; g.spd_flag = (int *)(w + o_flag);
    LbaRun run = {0, 0, 0, 0};
    if (E > 0 && nf > 0) {
        lba_optimize(g, n_iterations, run, 1e-16);              // :794, :986-987
        MTRY(g.status);
    }
    if (run.iterations == 0 && E > 0) MTRY(g.errors_now(g.chi2_initial));
    g.prof.pre(s);
    if (n) hipLaunchKernelGGL(k_eg_output, dim3(eg_blocks(n)), dim3(EG_T), 0, s, d, g.cur);           // :992-1010
    if (P) hipLaunchKernelGGL(k_eg_points, dim3(eg_blocks(P)), dim3(EG_T), 0, s, d, g.cur);           // :1013-1043
    MHIPCHK(hipGetLastError());
    std::vector<double> unread;
    if (!Scw_out) { unread.resize(8 * (size_t)n + 1); Scw_out = unread.data(); }
    void *const host[3] = {Scw_out, Tcw, xw};
    const size_t parts[3] = {64 * (size_t)n, 64 * (size_t)n, 12 * (size_t)P};
    MTRY(orbm_d2h_split(m, host, parts, 3, d.out_S, s));
    g.prof.post(ORBM_EG_SPLIT_OUTPUT, s);
    MTRY(orbm_sync(m, s));
    g.prof.drain();
    if (stats) *stats = {run.iterations, run.trials, run.lambda, g.chi2_initial, run.iterations ? run.chi2 : g.chi2_initial};
    return ORBX_OK;
}
}   // namespace

extern "C" int orbm_optimize_essential_graph(orbm_matcher *m, const orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw,
                                             double *Scw_out, orbp_eg_stats *stats)
{
    return eg_run(m, p, n_iterations, Tcw, xw, Scw_out, stats, nullptr, nullptr);
}
extern "C" int orbm_optimize_essential_graph_split(orbm_matcher *m, const orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw,
                                                   double *Scw_out, orbp_eg_stats *stats, double *split_ms, int32_t *split_count)
{
    if (!split_ms || !split_count) return mfail(ORBX_E_INVALID, "optimize_essential_graph_split: NULL split_ms or split_count");
    return eg_run(m, p, n_iterations, Tcw, xw, Scw_out, stats, split_ms, split_count);
}
