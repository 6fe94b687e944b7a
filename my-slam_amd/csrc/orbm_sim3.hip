// orbm_sim3.hip -- the hypotheses of Sim3Solver::iterate (src/Sim3Solver.cc:163-181 of WChen09/My-SLAM) for ALL candidate key frames
// of LoopClosing::ComputeSim3 (src/LoopClosing.cc:253-343) in one launch: orbm_sim3_hypotheses / orbm_sim3_hypotheses_device
// (include/orbm.h).  The draws stay on the host (orbp_sim3_draw); a hypothesis is a triple of correspondence indices of its problem.
//
// One wave per hypothesis, SIM3_WAVES waves to a workgroup, hypotheses by flat index (problem = binary search over hyp_off), so the
// waves of a workgroup read the correspondence arrays of one problem except at a problem's end.  Every lane runs sim3_from_triple
// (orbm_sim3_body.h, the host solver's text) on the three gathered point pairs: the work is uniform, and 64 redundant solves cost
// what one does.  The lanes then stride over the problem's correspondences; a ballot is 64 bits of the mask and its popcount adds to
// the count.  No LDS, no barrier, no atomics; lane 0 writes the wave's results with vector stores.
#include "orbm_internal.h"
#include "orbm_sim3_body.h"

#define SIM3_WAVES (M_THREADS / 64)

__global__ __launch_bounds__(M_THREADS) void k_sim3_hypotheses(
    int n_problems, const int32_t *__restrict__ off, const float *__restrict__ x1_all, const float *__restrict__ x2_all,
    const float *__restrict__ e1_all, const float *__restrict__ e2_all, const orbm_sim3_camera *__restrict__ cams,
    const int32_t *__restrict__ hyp_off, const int32_t *__restrict__ triples, const int64_t *__restrict__ mask_off,
    int32_t *__restrict__ n_inliers, float *__restrict__ sRt, uint32_t *__restrict__ masks)
{
    const int lane = threadIdx.x & 63;
    const long long hl = (long long)blockIdx.x * SIM3_WAVES + (threadIdx.x >> 6);
    const int total = hyp_off[n_problems];
    if (hl >= total) return;                    // whole waves leave
    const int h = __builtin_amdgcn_readfirstlane((int)hl);
    int lo = 0, hi = n_problems - 1;            // the last p with hyp_off[p] <= h (problems without hypotheses are stepped over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hyp_off[mid] <= h) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
    const long long c0 = off[p];
    const int n = off[p + 1] - off[p];
    const int W = (n + 31) >> 5;
    uint32_t *mk = masks + mask_off[p] + (long long)(h - hyp_off[p]) * W;
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
        const unsigned long long b = __ballot(inl);
        count += __popcll(b);
        if (lane == 0) {
            mk[base >> 5] = (uint32_t)b;
            if ((base >> 5) + 1 < W) mk[(base >> 5) + 1] = (uint32_t)(b >> 32);
        }
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

static int sim3_check_counts(int n_problems)
{
    if (n_problems < 0) return mfail(ORBX_E_INVALID, "n_problems=%d", n_problems);
    if (n_problems > (1 << 24)) return mfail(ORBX_E_CAPACITY, "request beyond 2^24 problems");
    return ORBX_OK;
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
    MTRY(sim3_check_counts(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (!off || !hyp_off || !mask_off || !cams) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (off[0] != 0 || hyp_off[0] != 0 || mask_off[0] != 0) return mfail(ORBX_E_INVALID, "off[0], hyp_off[0] and mask_off[0] must be 0");
    for (int p = 0; p < n_problems; p++) {
        if (off[p + 1] < off[p]) return mfail(ORBX_E_INVALID, "off not monotone at %d", p);
        if (hyp_off[p + 1] < hyp_off[p]) return mfail(ORBX_E_INVALID, "hyp_off not monotone at %d", p);
        const int64_t W = ((int64_t)off[p + 1] - off[p] + 31) / 32;
        if (mask_off[p + 1] != mask_off[p] + W * ((int64_t)hyp_off[p + 1] - hyp_off[p]))
            return mfail(ORBX_E_INVALID, "mask_off[%d] is not mask_off[%d] + hypotheses * ceil(n / 32)", p + 1, p);
    }
    const int total = off[n_problems], H = hyp_off[n_problems];
    const int64_t MW = mask_off[n_problems];
    if (H == 0) return ORBX_OK;
    if (total > (1 << 28) || H > (1 << 26) || MW > (1ll << 29)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 correspondences / 2^26 hypotheses / 2^29 mask words");
    if (!triples || !n_inliers || !sRt || (MW > 0 && !masks)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (total > 0 && (!x3dc1 || !x3dc2 || !max_err1 || !max_err2)) return mfail(ORBX_E_INVALID, "NULL buffer");
    for (int p = 0; p < n_problems; p++) {
        const int n = off[p + 1] - off[p];
        for (long long k = 3ll * hyp_off[p]; k < 3ll * hyp_off[p + 1]; k++)
            if (triples[k] < 0 || triples[k] >= n)
                return mfail(ORBX_E_INVALID, "problem %d: triple index %d outside [0, %d)", p, triples[k], n);
    }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out holds the counts, the 13 floats per hypothesis, then the mask words
    const size_t Hs = (size_t)H, words = 14 * Hs + (size_t)MW;
    MTRY(orbm_grow(m, 0, 0, (long long)words));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    const size_t B = (size_t)n_problems, N = (size_t)total;
    InBlock in(m);
    const int po = in.add(off, (B + 1) * 4), p1 = in.add(x3dc1, N * 12), p2 = in.add(x3dc2, N * 12), pe1 = in.add(max_err1, N * 4),
              pe2 = in.add(max_err2, N * 4), pc = in.add(cams, B * sizeof(orbm_sim3_camera)), ph = in.add(hyp_off, (B + 1) * 4),
              pt = in.add(triples, Hs * 12), pm = in.add(mask_off, (B + 1) * 8);
    MTRY(in.upload(s));
    int32_t *d_cnt = m->d_out;
    float *d_sRt = reinterpret_cast<float *>(m->d_out + Hs);
    uint32_t *d_masks = reinterpret_cast<uint32_t *>(m->d_out + 14 * Hs);
    sim3_launch(n_problems, H, in.dev_at<int32_t>(po), in.dev_at<float>(p1), in.dev_at<float>(p2), in.dev_at<float>(pe1), in.dev_at<float>(pe2),
                in.dev_at<orbm_sim3_camera>(pc), in.dev_at<int32_t>(ph), in.dev_at<int32_t>(pt), in.dev_at<int64_t>(pm), d_cnt, d_sRt, d_masks, s);
    MHIPCHK(hipGetLastError());
    void *host[3] = {n_inliers, sRt, masks};
    const size_t parts[3] = {Hs * 4, Hs * 52, (size_t)MW * 4};
    MTRY(orbm_d2h_split(m, host, parts, 3, m->d_out, s));
    MTRY(orbm_sync(m, s));
    return ORBX_OK;
}

extern "C" int orbm_sim3_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_x3dc1,
                                           const float *d_x3dc2, const float *d_max_err1, const float *d_max_err2,
                                           const orbm_sim3_camera *d_cams, const int32_t *d_hyp_off, const int32_t *d_triples,
                                           const int64_t *d_mask_off, int32_t *d_n_inliers, float *d_sRt, uint32_t *d_masks, void *hip_stream)
{
    MTRY(sim3_check_counts(n_problems));
    if (total_hypotheses < 0) return mfail(ORBX_E_INVALID, "total_hypotheses=%d", total_hypotheses);
    if (n_problems == 0 || total_hypotheses == 0) return ORBX_OK;
    if (!d_off || !d_x3dc1 || !d_x3dc2 || !d_max_err1 || !d_max_err2 || !d_cams || !d_hyp_off || !d_triples || !d_mask_off || !d_n_inliers ||
        !d_sRt || !d_masks)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if ((((uintptr_t)d_off | (uintptr_t)d_x3dc1 | (uintptr_t)d_x3dc2 | (uintptr_t)d_max_err1 | (uintptr_t)d_max_err2 | (uintptr_t)d_cams |
          (uintptr_t)d_hyp_off | (uintptr_t)d_triples | (uintptr_t)d_n_inliers | (uintptr_t)d_sRt | (uintptr_t)d_masks) & 3) ||
        ((uintptr_t)d_mask_off & 7))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned, mask_off 8-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    sim3_launch(n_problems, total_hypotheses, d_off, d_x3dc1, d_x3dc2, d_max_err1, d_max_err2, d_cams, d_hyp_off, d_triples, d_mask_off,
                d_n_inliers, d_sRt, d_masks, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
