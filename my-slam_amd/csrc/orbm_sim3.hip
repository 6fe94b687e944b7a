// orbm_sim3.hip -- the hypotheses of Sim3Solver::iterate (src/Sim3Solver.cc:163-181 of WChen09/My-SLAM) for ALL candidate key frames
// of LoopClosing::ComputeSim3 (src/LoopClosing.cc:253-343) in one launch: orbm_sim3_hypotheses / orbm_sim3_hypotheses_device
// (include/orbm.h).  The draws stay on the host (orbp_sim3_draw); a hypothesis is a triple of correspondence indices of its problem.
//
// One wave per hypothesis in the frame of orbm_hyp.h (flat index, problem search, mask rows, vote).  Every lane runs
// sim3_from_triple (orbm_sim3_body.h, the host solver's text) on the three gathered point pairs: the work is uniform, and 64
// redundant solves cost what one does.  No LDS, no barrier, no atomics; lane 0 writes the wave's results with vector stores.
#include "orbm_hyp.h"
#include "orbm_sim3_body.h"

#define SIM3_WAVES (M_THREADS / 64)

__global__ __launch_bounds__(M_THREADS) void k_sim3_hypotheses(
    int n_problems, const int32_t *__restrict__ off, const float *__restrict__ x1_all, const float *__restrict__ x2_all,
    const float *__restrict__ e1_all, const float *__restrict__ e2_all, const orbm_sim3_camera *__restrict__ cams,
    const int32_t *__restrict__ hyp_off, const int32_t *__restrict__ triples, const int64_t *__restrict__ mask_off,
    int32_t *__restrict__ n_inliers, float *__restrict__ sRt, uint32_t *__restrict__ masks)
{
    const int lane = threadIdx.x & 63;
    const long long hl = hyp_wave_index(SIM3_WAVES);
    if (hl >= hyp_off[n_problems]) return;      // whole waves leave
    const HypFrame f = hyp_frame(n_problems, off, hyp_off, mask_off, masks, hl);
    const int h = f.h, p = f.p, n = f.n;
    const long long c0 = f.c0;
    float *out = sRt + 13 * (long long)h;
    if (n <= 0) {                               // nothing to sample from: refused by the host variant
        if (lane == 0) {
            n_inliers[h] = 0;
            for (int i = 0; i < 13; i++) out[i] = 0.f;
        }
        return;
    }
    const float *x1 = x1_all + 3 * c0, *x2 = x2_all + 3 * c0, *e1 = e1_all + c0, *e2 = e2_all + c0;
    const orbm_sim3_camera cam = cams[p];
    const Sim3Cam K1 = {cam.K1[0], cam.K1[1], cam.K1[2], cam.K1[3]}, K2 = {cam.K2[0], cam.K2[1], cam.K2[2], cam.K2[3]};
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int idx = min(max(triples[3 * (long long)h + k], 0), n - 1);      // an index outside the problem must not read outside it
#pragma unroll
        for (int i = 0; i < 3; i++) { P1[k][i] = x1[3 * (long long)idx + i]; P2[k][i] = x2[3 * (long long)idx + i]; }
    }
    Sim3Hyp hyp;
    sim3_from_triple(P1, P2, cam.fix_scale != 0, hyp);
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inl = false;
        if (i < n) inl = sim3_check_one(hyp, x1 + 3 * (long long)i, x2 + 3 * (long long)i, K1, K2, e1[i], e2[i]);
        count += hyp_vote(f, inl, base, lane);
    }
    if (lane == 0) {
        n_inliers[h] = count;
        out[0] = hyp.s;
#pragma unroll
        for (int i = 0; i < 9; i++) out[1 + i] = hyp.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) out[10 + i] = hyp.t[i];
    }
}

static void sim3_launch(int n_problems, int total_hyp, const int32_t *off, const float *x1, const float *x2, const float *e1, const float *e2,
                        const orbm_sim3_camera *cams, const int32_t *hyp_off, const int32_t *triples, const int64_t *mask_off,
                        int32_t *n_inliers, float *sRt, uint32_t *masks, hipStream_t s)
{
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((total_hyp + SIM3_WAVES - 1) / SIM3_WAVES), dim3(M_THREADS), 0, s, n_problems, off, x1, x2, e1, e2,
                       cams, hyp_off, triples, mask_off, n_inliers, sRt, masks);
}

extern "C" int orbm_sim3_hypotheses(orbm_matcher *m, int n_problems, const int32_t *off, const float *x3dc1, const float *x3dc2,
                                    const float *max_err1, const float *max_err2, const orbm_sim3_camera *cams, const int32_t *hyp_off,
                                    const int32_t *triples, const int64_t *mask_off, int32_t *n_inliers, float *sRt, uint32_t *masks)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(off, hyp_off, mask_off, cams)) return mfail(ORBX_E_INVALID, "NULL buffer");
    int total, H;
    int64_t MW;
    MTRY(check_hyp_csr(n_problems, off, hyp_off, mask_off, 28, "correspondences", 26, total, H, MW));
    if (H == 0) return ORBX_OK;
    if (any_null(triples, n_inliers, sRt) || (MW > 0 && !masks)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (total > 0 && any_null(x3dc1, x3dc2, max_err1, max_err2)) return mfail(ORBX_E_INVALID, "NULL buffer");
    for (int p = 0; p < n_problems; p++) {
        const int n = off[p + 1] - off[p];
        for (long long k = 3ll * hyp_off[p]; k < 3ll * hyp_off[p + 1]; k++)
            if (triples[k] < 0 || triples[k] >= n)
                return mfail(ORBX_E_INVALID, "problem %d: triple index %d outside [0, %d)", p, triples[k], n);
    }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out holds the counts, the 13 floats per hypothesis, then the mask words
    const size_t B = (size_t)n_problems, N = (size_t)total, Hs = (size_t)H;
    const OutBlock out({{n_inliers, Hs * 4}, {sRt, Hs * 52}, {masks, (size_t)MW * 4}});
    MTRY(orbm_grow(m, 0, 0, (long long)out.words()));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int po = in.add(off, (B + 1) * 4), p1 = in.add(x3dc1, N * 12), p2 = in.add(x3dc2, N * 12), pe1 = in.add(max_err1, N * 4),
              pe2 = in.add(max_err2, N * 4), pc = in.add(cams, B * sizeof(orbm_sim3_camera)), ph = in.add(hyp_off, (B + 1) * 4),
              pt = in.add(triples, Hs * 12), pm = in.add(mask_off, (B + 1) * 8);
    MTRY(in.upload(s));
    sim3_launch(n_problems, H, in.dev_at<int32_t>(po), in.dev_at<float>(p1), in.dev_at<float>(p2), in.dev_at<float>(pe1), in.dev_at<float>(pe2),
                in.dev_at<orbm_sim3_camera>(pc), in.dev_at<int32_t>(ph), in.dev_at<int32_t>(pt), in.dev_at<int64_t>(pm),
                out.dev_at<int32_t>(m, 0), out.dev_at<float>(m, 1), out.dev_at<uint32_t>(m, 2), s);
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_sim3_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_x3dc1,
                                           const float *d_x3dc2, const float *d_max_err1, const float *d_max_err2,
                                           const orbm_sim3_camera *d_cams, const int32_t *d_hyp_off, const int32_t *d_triples,
                                           const int64_t *d_mask_off, int32_t *d_n_inliers, float *d_sRt, uint32_t *d_masks, void *hip_stream)
{
    MTRY(check_problem_count(n_problems));
    if (total_hypotheses < 0) return mfail(ORBX_E_INVALID, "total_hypotheses=%d", total_hypotheses);
    if (n_problems == 0 || total_hypotheses == 0) return ORBX_OK;
    if (any_null(d_off, d_x3dc1, d_x3dc2, d_max_err1, d_max_err2, d_cams, d_hyp_off, d_triples, d_mask_off, d_n_inliers, d_sRt, d_masks))
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_off, d_x3dc1, d_x3dc2, d_max_err1, d_max_err2, d_cams, d_hyp_off, d_triples, d_n_inliers, d_sRt, d_masks) ||
        misaligned(7, d_mask_off))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned, mask_off 8-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    sim3_launch(n_problems, total_hypotheses, d_off, d_x3dc1, d_x3dc2, d_max_err1, d_max_err2, d_cams, d_hyp_off, d_triples, d_mask_off,
                d_n_inliers, d_sRt, d_masks, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
