// orbm_pnp.hip -- the hypotheses of PnPsolver::iterate (src/PnPsolver.cc:182-210 of WChen09/My-SLAM: compute_pose on the drawn set,
// then CheckInliers) for ALL candidate key frames of Tracking::Relocalization (src/Tracking.cc:1348-1509) in one launch:
// orbm_pnp_hypotheses / orbm_pnp_hypotheses_device (include/orbm.h).  The draws stay on the host (orbp_pnp_draw); a hypothesis is a
// set of 4 to 8 correspondence indices of its problem.
//
// One wave per hypothesis in the frame of orbm_hyp.h (flat index, problem search, mask rows, vote).  The solve is
// epnp_compute_pose of orbp_epnp_body.h, the host solver's text, run uniformly by the wave: its matrices (the 12 x 12 Jacobi's B and
// V, the eigenvectors, L, the small SVDs) are indexed at run time, so they live in a wave-private piece of LDS (sizeof(PnpWaveLds)
// bytes per wave) instead of scratch; every lane reads the same address (a broadcast) and writes the same value.  Every sum runs in
// the host's order: no cross-lane reduction.  No workgroup barrier, no atomics; lane 0 writes the wave's results with vector stores.
#include "orbm_hyp.h"
#include "orbp_epnp_body.h"

#define PNP_WAVES (M_THREADS / 64)

struct PnpWaveLds {
    EpnpWork wk;
    double pws[3 * ORBM_PNP_MAX_SET], us[2 * ORBM_PNP_MAX_SET], alphas[4 * ORBM_PNP_MAX_SET], pcs[3 * ORBM_PNP_MAX_SET];
};

__global__ __launch_bounds__(M_THREADS) void k_pnp_hypotheses(
    int n_problems, const int32_t *__restrict__ off, const float *__restrict__ p2d_all, const float *__restrict__ p3d_all,
    const float *__restrict__ err_all, const orbm_pnp_camera *__restrict__ cams, const int32_t *__restrict__ hyp_off,
    const int32_t *__restrict__ samples, const int64_t *__restrict__ mask_off, int32_t *__restrict__ n_inliers, double *__restrict__ Rt,
    uint32_t *__restrict__ masks)
{
    __shared__ PnpWaveLds lds[PNP_WAVES];
    const int lane = threadIdx.x & 63;
    const long long hl = hyp_wave_index(PNP_WAVES);
    if (hl >= hyp_off[n_problems]) return;      // whole waves leave
    const HypFrame f = hyp_frame(n_problems, off, hyp_off, mask_off, masks, hl);
    const int h = f.h, p = f.p, n = f.n;
    const long long c0 = f.c0;
    double *out = Rt + 12 * (long long)h;
    if (n <= 0) {                               // nothing to sample from: refused by the host variant
        if (lane == 0) {
            n_inliers[h] = 0;
            for (int i = 0; i < 12; i++) out[i] = 0.0;
        }
        return;
    }
    const float *p2d = p2d_all + 2 * c0, *p3d = p3d_all + 3 * c0, *err = err_all + c0;
    const orbm_pnp_camera cam = cams[p];
    const int set = min(max(cam.set_size, 4), ORBM_PNP_MAX_SET);      // another size is refused by the host variant
    PnpWaveLds &L = lds[threadIdx.x >> 6];
    for (int k = 0; k < set; k++) {
        const int idx = min(max(samples[ORBM_PNP_MAX_SET * (long long)h + k], 0), n - 1);      // an index outside the problem must not read outside it
        for (int i = 0; i < 3; i++) L.pws[3 * k + i] = p3d[3 * (long long)idx + i];
        for (int i = 0; i < 2; i++) L.us[2 * k + i] = p2d[2 * (long long)idx + i];
    }
    EpnpProblem e;
    e.fu = cam.fx; e.fv = cam.fy; e.uc = cam.cx; e.vc = cam.cy; e.n = set;
    e.pws = L.pws; e.us = L.us; e.alphas = L.alphas; e.pcs = L.pcs;
    double R[9], t[3];
    epnp_compute_pose(e, L.wk, R, t);
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inl = false;
        if (i < n) inl = epnp_check_one(R, t, e.fu, e.fv, e.uc, e.vc, p3d + 3 * (long long)i, p2d + 2 * (long long)i, err[i]);
        count += hyp_vote(f, inl, base, lane);
    }
    if (lane == 0) {
        n_inliers[h] = count;
#pragma unroll
        for (int i = 0; i < 9; i++) out[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) out[9 + i] = t[i];
    }
}

static void pnp_launch(int n_problems, int total_hyp, const int32_t *off, const float *p2d, const float *p3d, const float *max_err,
                       const orbm_pnp_camera *cams, const int32_t *hyp_off, const int32_t *samples, const int64_t *mask_off, int32_t *n_inliers,
                       double *Rt, uint32_t *masks, hipStream_t s)
{
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((total_hyp + PNP_WAVES - 1) / PNP_WAVES), dim3(M_THREADS), 0, s, n_problems, off, p2d, p3d, max_err,
                       cams, hyp_off, samples, mask_off, n_inliers, Rt, masks);
}

extern "C" int orbm_pnp_hypotheses(orbm_matcher *m, int n_problems, const int32_t *off, const float *p2d, const float *p3d, const float *max_err,
                                   const orbm_pnp_camera *cams, const int32_t *hyp_off, const int32_t *samples, const int64_t *mask_off,
                                   int32_t *n_inliers, double *Rt, uint32_t *masks)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(off, hyp_off, mask_off, cams)) return mfail(ORBX_E_INVALID, "NULL buffer");
    int total, H;
    int64_t MW;
    MTRY(check_hyp_csr(n_problems, off, hyp_off, mask_off, 28, "correspondences", 24, total, H, MW));
    if (H == 0) return ORBX_OK;
    if (any_null(samples, n_inliers, Rt) || (MW > 0 && !masks)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (total > 0 && any_null(p2d, p3d, max_err)) return mfail(ORBX_E_INVALID, "NULL buffer");
    for (int p = 0; p < n_problems; p++) {
        if (hyp_off[p + 1] == hyp_off[p]) continue;
        const int n = off[p + 1] - off[p], set = cams[p].set_size;
        if (set < 4 || set > ORBM_PNP_MAX_SET) return mfail(ORBX_E_INVALID, "problem %d: set_size %d outside [4, %d]", p, set, ORBM_PNP_MAX_SET);
        for (long long hh = hyp_off[p]; hh < hyp_off[p + 1]; hh++) {
            const int32_t *sm = samples + ORBM_PNP_MAX_SET * hh;
            for (int k = 0; k < set; k++) {
                if (sm[k] < 0 || sm[k] >= n) return mfail(ORBX_E_INVALID, "problem %d: sample index %d outside [0, %d)", p, sm[k], n);
                for (int j = 0; j < k; j++)
                    if (sm[j] == sm[k]) return mfail(ORBX_E_INVALID, "problem %d: sample index %d repeated in one sample", p, sm[k]);
            }
        }
    }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out holds the 12 doubles per hypothesis first (8-byte aligned at its start), then the counts, then the mask words
    const size_t B = (size_t)n_problems, N = (size_t)total, Hs = (size_t)H;
    const OutBlock out({{Rt, Hs * 96}, {n_inliers, Hs * 4}, {masks, (size_t)MW * 4}});
    MTRY(orbm_grow(m, 0, 0, (long long)out.words()));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pm = in.add(mask_off, (B + 1) * 8), po = in.add(off, (B + 1) * 4), p2 = in.add(p2d, N * 8), p3 = in.add(p3d, N * 12),
              pe = in.add(max_err, N * 4), pc = in.add(cams, B * sizeof(orbm_pnp_camera)), ph = in.add(hyp_off, (B + 1) * 4),
              ps = in.add(samples, Hs * 4 * ORBM_PNP_MAX_SET);
    MTRY(in.upload(s));
    pnp_launch(n_problems, H, in.dev_at<int32_t>(po), in.dev_at<float>(p2), in.dev_at<float>(p3), in.dev_at<float>(pe), in.dev_at<orbm_pnp_camera>(pc),
               in.dev_at<int32_t>(ph), in.dev_at<int32_t>(ps), in.dev_at<int64_t>(pm), out.dev_at<int32_t>(m, 1), out.dev_at<double>(m, 0),
               out.dev_at<uint32_t>(m, 2), s);
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_pnp_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_p2d,
                                          const float *d_p3d, const float *d_max_err, const orbm_pnp_camera *d_cams, const int32_t *d_hyp_off,
                                          const int32_t *d_samples, const int64_t *d_mask_off, int32_t *d_n_inliers, double *d_Rt,
                                          uint32_t *d_masks, void *hip_stream)
{
    MTRY(check_problem_count(n_problems));
    if (total_hypotheses < 0) return mfail(ORBX_E_INVALID, "total_hypotheses=%d", total_hypotheses);
    if (n_problems == 0 || total_hypotheses == 0) return ORBX_OK;
    if (any_null(d_off, d_p2d, d_p3d, d_max_err, d_cams, d_hyp_off, d_samples, d_mask_off, d_n_inliers, d_Rt, d_masks))
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_off, d_p2d, d_p3d, d_max_err, d_cams, d_hyp_off, d_samples, d_n_inliers, d_masks) || misaligned(7, d_mask_off, d_Rt))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned, Rt and mask_off 8-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    pnp_launch(n_problems, total_hypotheses, d_off, d_p2d, d_p3d, d_max_err, d_cams, d_hyp_off, d_samples, d_mask_off, d_n_inliers, d_Rt, d_masks, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
