// orbm_eg.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044 of WChen09/My-SLAM, on g2o) on the GPU:
// orbm_optimize_essential_graph (include/orbm.h) over the flat problem of orbp_optimize_essential_graph (include/orbp.h).  Host and
// kernels run one text for the edges (orbp_eg_body.h); the host drives lm_optimize (orbp_lm_body.h) with launches as its passes, as
// orbm_bundle_adjustment does (orbm_opt.h: what they share), and the 7N x 7N system goes to orbm_spd.hip's many-workgroup solve.
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
//                 k_eg_reduce_out  one workgroup: chi2 and computeScale's x . (lambda x + b), each by opt_block_sum (orbm_opt.h has
//                                  the tree), into the 64 bytes the host reads
//   at the end    k_eg_output, k_eg_points, one copy home
// H0 is zeroed once a call: the graph does not change, so every iteration rewrites the same blocks.  The estimates are double
// buffered ([cur] and the trial's), so accept is a flip and reject nothing.
//
// Kept because the machines are shared (DESIGN.md sections 22 to 24): plain launches in stream order, no cooperative launch, no
// grid-wide barrier, no spin-wait, nothing between workgroups but kernel boundaries, no atomic; every loop is bounded by a count
// known at launch; a failed pivot leaves x = 0 through the solve's flag and nothing traps.
#include "orbm_opt.h"
#include "ws_layout.h"
#include "orbp_internal.h"
#include "orbp_eg_body.h"
#include "orbp_lm_body.h"
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
    for (int i = tid; i < d.N; i += EG_RT) scale += lm_scale_term(d.x[i], d.b0[i], lambda);
    chi = opt_block_sum<EG_RT>(chi, sh);
    scale = opt_block_sum<EG_RT>(scale, sh);
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

// "the passes of a problem" for lm_optimize (orbp_lm_body.h), as kernel launches on the handle's stream (OptGpu, orbm_opt.h)
struct EgGpu : OptGpu {
    EgDev d = {};
    int *spd_flag = nullptr;                // orbm_spd_solve_device's; its y is d.y
    double chi2_initial = 0;

    bool stop() const { return status != ORBX_OK; }
    int read_out(double lambda)             // the one small block: reduce, copy, synchronise
    {
        prof.pre(s);
        hipLaunchKernelGGL(k_eg_reduce_out, dim3(1), dim3(EG_RT), 0, s, d, lambda);
        return read_back(ORBM_EG_SPLIT_READ_BACK);
    }
    int errors_now(double &chi)             // computeActiveErrors + activeChi2 at the current estimates
    {
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_UPDATE_ERRORS, s, hipLaunchKernelGGL(k_eg_errors, dim3(opt_blocks(d.E, EG_T)), dim3(EG_T), 0, s, d, cur));
        MTRY(read_out(0.));
        chi = pin[OUT_CHI];
        return ORBX_OK;
    }
    int do_linearize(bool first, bool with_errors, double &chi)
    {
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_LINEARIZE, s, hipLaunchKernelGGL(k_eg_linearize, dim3(opt_blocks(d.E, EG_EPB)), dim3(EG_T), 0, s, d, cur));
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
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_STAGE, s, hipLaunchKernelGGL(k_eg_stage, dim3(opt_blocks(d.N, EG_T), d.N), dim3(EG_T), 0, s, d, lambda));
        SPLIT_GROUP(prof, ORBM_EG_SPLIT_SOLVE, s, MTRY(orbm_spd_solve_device(d.W, d.bw, d.y, d.x, spd_flag, d.out + OUT_OK, d.N, s)));
        prof.pre(s);
        hipLaunchKernelGGL(k_eg_update, dim3(opt_blocks(d.n, EG_T)), dim3(EG_T), 0, s, d, cur);
        hipLaunchKernelGGL(k_eg_errors, dim3(opt_blocks(d.E, EG_T)), dim3(EG_T), 0, s, d, 1 - cur);
        prof.post(ORBM_EG_SPLIT_UPDATE_ERRORS, s);
        MTRY(read_out(lambda));             // checks the launches above as well
        chi = pin[OUT_CHI]; scale = pin[OUT_SCALE]; ok = pin[OUT_OK] != 0.;
        return ORBX_OK;
    }
    void linearize(bool first, bool with_errors, double &chi, double &maxdiag)
    {
        maxdiag = 0;                        // computeLambdaInit returns the user's value
        if (status == ORBX_OK) status = do_linearize(first, with_errors, chi);
    }
    void trial(double lambda, double &chi, double &scale, bool &ok) { if (status == ORBX_OK) status = do_trial(lambda, chi, scale, ok); }
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

    EgGpu g; EgDev &d = g.d;
    d.n = n; d.fixed = p->fixed; d.nf = nf; d.N = 7 * nf; d.E = E; d.P = P; d.npairs = npairs; d.fix_scale = p->fix_scale;
    const size_t N = (size_t)d.N, szd = sizeof(double), sn = (size_t)n, sE = (size_t)E;
    WsLayout ws;
    ws.take(d.meas, 8 * sE); ws.take(d.est[0], 8 * sn); ws.take(d.est[1], 8 * sn); ws.take(d.err, 7 * sE);
    ws.take(d.Ji, 49 * sE); ws.take(d.Jj, 49 * sE); ws.take(d.chi_e, sE); ws.take(d.H0, N * N);
    ws.take(d.b0, N); ws.take(d.W, N * N); ws.take(d.bw, N); ws.take(d.y, N); ws.take(d.x, N); ws.take(d.out, 8); ws.take(g.spd_flag, 16);
    uint8_t *res = nullptr;
    ws.take(res, 64 * sn + 64 * sn + 12 * (size_t)P);           // the results back to back: one copy home
    MTRY(orbm_ensure_opt(m, ws.bytes()));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    ws.bind(m->d_opt.get());
    d.out_S = (double *)res; d.out_Tcw = (float *)(d.out_S + 8 * sn); d.out_xw = d.out_Tcw + 16 * sn;

    InBlock in(m);
    const int pS = in.add(p->Scw, 64 * (size_t)n), pN = in.add(p->Snc, 64 * (size_t)n), pi = in.add(p->edge_i, 4 * (size_t)E),
              pj = in.add(p->edge_j, 4 * (size_t)E), pc = in.add(p->edge_corrected, (size_t)E), pr = in.add(p->ref, 4 * (size_t)P),
              px = in.add(xw, 12 * (size_t)P), pf = in.add(free_of.data(), 4 * (size_t)n), pvo = in.add(vtx_off.data(), 4 * ((size_t)n + 1)),
              pve = in.add(vtx_edge.data(), 4 * vtx_edge.size()), ppo = in.add(pair_off.data(), 4 * pair_off.size()),
              ppe = in.add(pair_edge.data(), 4 * pair_edge.size()), pph = in.add(pair_hi.data(), 4 * (size_t)npairs),
              ppl = in.add(pair_lo.data(), 4 * (size_t)npairs);
    g.m = m; g.s = s; g.pin = (double *)m->opt_pin.get(); g.out = d.out;
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
    if (E) hipLaunchKernelGGL(k_eg_measure, dim3(opt_blocks(E, EG_T)), dim3(EG_T), 0, s, d);
    MHIPCHK(hipGetLastError());
    g.prof.post(ORBM_EG_SPLIT_UPLOAD, s);

    LmRun run = {0, 0, 0, 0};
    if (E > 0 && nf > 0) {
        lm_optimize(g, n_iterations, run, 1e-16);               // :794, :986-987
        MTRY(g.status);
    }
    if (run.iterations == 0 && E > 0) MTRY(g.errors_now(g.chi2_initial));
    g.prof.pre(s);
    if (n) hipLaunchKernelGGL(k_eg_output, dim3(opt_blocks(n, EG_T)), dim3(EG_T), 0, s, d, g.cur);    // :992-1010
    if (P) hipLaunchKernelGGL(k_eg_points, dim3(opt_blocks(P, EG_T)), dim3(EG_T), 0, s, d, g.cur);    // :1013-1043
    MHIPCHK(hipGetLastError());
    std::vector<double> unread;
    if (!Scw_out) { unread.resize(8 * sn + 1); Scw_out = unread.data(); }
    MTRY(g.download({Scw_out, Tcw, xw}, {64 * sn, 64 * sn, 12 * (size_t)P}, d.out_S, ORBM_EG_SPLIT_OUTPUT));
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
