// orbm_init.hip -- the monocular Initializer (src/Initializer.cc of WChen09/My-SLAM) on the GPU: every hypothesis of
// FindHomography (:148-171) and FindFundamental (:199-222) in one launch (orbm_init_hypotheses / _device), and the 4 or 8 CheckRT
// passes of ReconstructF / ReconstructH (:494-497, :698-718) in one launch (orbm_init_check_rt / _device).  The draws, the two
// walks that keep the best score, the candidate motions and the acceptance rules stay on the host (orbp_init.cc).
//
// k_init_hypotheses: one wave per hypothesis = (index set, model) in the frame of orbm_hyp.h (flat index, problem search, mask
// rows, vote).  The solve (orbp_init_body.h, the host solver's text) is run uniformly by the wave: the Jacobi's 16 x 9 / 9 x 9
// matrix, its V, the column norms and their order are indexed at run time, so they live in a wave-private piece of LDS
// (sizeof(InitWork) bytes per wave) instead of scratch; every lane reads the same address (a broadcast) and writes the same value.
// The score is the reference's float sum in match order, term 1 then term 2 of every match: the lanes compute the terms, and the
// wave adds them one readlane at a time on the uniform path, so the sum is the host's to the bit.  No workgroup barrier, no atomics;
// lane 0 writes the wave's results with vector stores.
//
// k_init_check_rt: one lane per (motion, match); init_motion_prepare is redone by every lane (a dozen products).
#include "orbm_hyp.h"
#include "orbp_init_body.h"

#define INIT_WAVES (M_THREADS / 64)

__global__ __launch_bounds__(M_THREADS) void k_init_hypotheses(
    int n_problems, const int32_t *__restrict__ off, const float *__restrict__ uv_all, const float *__restrict__ pn_all,
    const orbm_init_params *__restrict__ params, const int32_t *__restrict__ hyp_off, const int32_t *__restrict__ sets,
    const int32_t *__restrict__ models, const int64_t *__restrict__ mask_off, float *__restrict__ score_M, int32_t *__restrict__ n_inliers,
    uint32_t *__restrict__ masks)
{
    __shared__ InitWork lds[INIT_WAVES];
    const int lane = threadIdx.x & 63;
    const long long hl = hyp_wave_index(INIT_WAVES);
    if (hl >= hyp_off[n_problems]) return;      // whole waves leave
    const HypFrame f = hyp_frame(n_problems, off, hyp_off, mask_off, masks, hl);
    const int h = f.h, p = f.p, n = f.n;
    const long long c0 = f.c0;
    float *out = score_M + 10 * (long long)h;
    if (n <= 0) {                               // nothing to sample from: refused by the host variant
        if (lane == 0) {
            n_inliers[h] = 0;
            for (int i = 0; i < 10; i++) out[i] = 0.f;
        }
        return;
    }
    const float *uv = uv_all + 4 * c0, *pn = pn_all + 4 * c0;
    const orbm_init_params par = params[p];
    const bool is_h = models[h] == INIT_MODEL_H;            // another model is refused by the host variant
    InitWork &L = lds[threadIdx.x >> 6];
    for (int j = 0; j < 8; j++) {
        const int idx = min(max(sets[8 * (long long)h + j], 0), n - 1);     // an index outside the problem must not read outside it
        const float *q = pn + 4 * (long long)idx;
        if (is_h) init_fill_h_rows(L.B, j, q[0], q[1], q[2], q[3]);
        else init_fill_f_row(L.B, j, q[0], q[1], q[2], q[3]);
    }
    float T1[9], T2[9], T2x[9], v[9], M[9], H12[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { T1[i] = par.T1[i]; T2[i] = par.T2[i]; H12[i] = 0.f; }
    if (is_h) {
        init_null_vector(L, 16, v);
        init_inv33(T2, T2x);
        init_finish_h(v, T1, T2x, M, H12);
    } else {
        init_zero_row(L.B, 8);
        init_null_vector(L, 9, v);
        init_transpose33(T2, T2x);
        init_finish_f(v, T1, T2x, L, M);
    }
    const float inv_s2 = init_inv_sigma2(par.sigma);
    float score = 0.f;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inl = false;
        float s1 = 0.f, s2 = 0.f;
        if (i < n) {
            const float *q = uv + 4 * (long long)i;
            const float u1 = q[0], v1 = q[1], u2 = q[2], v2 = q[3];
            inl = is_h ? init_check_h_one(M, H12, u1, v1, u2, v2, inv_s2, s1, s2) : init_check_f_one(M, u1, v1, u2, v2, inv_s2, s1, s2);
        }
        count += hyp_vote(f, inl, base, lane);
        // the reference's sum (:363, :379 / :441, :459): match order, term 1 then term 2, in float
        const int lim = min(64, n - base);
        for (int k = 0; k < lim; k++) {
            score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s1), k));
            score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s2), k));
        }
    }
    if (lane == 0) {
        n_inliers[h] = count;
        out[0] = score;
#pragma unroll
        for (int i = 0; i < 9; i++) out[1 + i] = M[i];
    }
}

__global__ __launch_bounds__(M_THREADS) void k_init_check_rt(
    int n, int n_motions, const float *__restrict__ uv, const uint8_t *__restrict__ inliers, const float *__restrict__ Rt, float fx, float fy,
    float cx, float cy, float th2, uint8_t *__restrict__ status, float *__restrict__ cos_parallax, float *__restrict__ p3d)
{
    const long long g = (long long)blockIdx.x * M_THREADS + threadIdx.x;
    if (g >= (long long)n * n_motions) return;
    const int k = (int)(g / n), i = (int)(g - (long long)k * n);
    const InitCam cam = {fx, fy, cx, cy};
    float X[3] = {0.f, 0.f, 0.f}, c = 0.f;
    int st = INIT_RT_NOT_INLIER;
    if (inliers[i]) {
        InitMotion mo;
        init_motion_prepare(cam, Rt + 12 * (long long)k, mo);
        const float *q = uv + 4 * (long long)i;
        st = init_check_rt_one(cam, mo, q[0], q[1], q[2], q[3], th2, X, c);
    }
    status[g] = (uint8_t)st;
    cos_parallax[g] = c;
    p3d[3 * g] = X[0]; p3d[3 * g + 1] = X[1]; p3d[3 * g + 2] = X[2];
}

static void init_launch(int n_problems, int total_hyp, const int32_t *off, const float *uv, const float *pn, const orbm_init_params *params,
                        const int32_t *hyp_off, const int32_t *sets, const int32_t *models, const int64_t *mask_off, float *score_M,
                        int32_t *n_inliers, uint32_t *masks, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_hypotheses, dim3((total_hyp + INIT_WAVES - 1) / INIT_WAVES), dim3(M_THREADS), 0, s, n_problems, off, uv, pn, params,
                       hyp_off, sets, models, mask_off, score_M, n_inliers, masks);
}

extern "C" int orbm_init_hypotheses(orbm_matcher *m, int n_problems, const int32_t *off, const float *uv, const float *pn,
                                    const orbm_init_params *params, const int32_t *hyp_off, const int32_t *sets, const int32_t *models,
                                    const int64_t *mask_off, float *score_M, int32_t *n_inliers, uint32_t *masks)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(off, hyp_off, mask_off, params)) return mfail(ORBX_E_INVALID, "NULL buffer");
    int total, H;
    int64_t MW;
    MTRY(check_hyp_csr(n_problems, off, hyp_off, mask_off, 26, "matches", 24, total, H, MW));
    if (H == 0) return ORBX_OK;
    if (any_null(sets, models, score_M, n_inliers) || (MW > 0 && !masks)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (total > 0 && any_null(uv, pn)) return mfail(ORBX_E_INVALID, "NULL buffer");
    for (int p = 0; p < n_problems; p++) {
        const int n = off[p + 1] - off[p];
        for (long long hh = hyp_off[p]; hh < hyp_off[p + 1]; hh++) {
            if (models[hh] != INIT_MODEL_H && models[hh] != INIT_MODEL_F)
                return mfail(ORBX_E_INVALID, "problem %d: model %d is neither H (0) nor F (1)", p, models[hh]);
            for (int k = 0; k < 8; k++)
                if (sets[8 * hh + k] < 0 || sets[8 * hh + k] >= n)
                    return mfail(ORBX_E_INVALID, "problem %d: set index %d outside [0, %d)", p, sets[8 * hh + k], n);
        }
    }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out holds the 10 floats per hypothesis, the counts, then the mask words
    const size_t B = (size_t)n_problems, N = (size_t)total, Hs = (size_t)H;
    const OutBlock out({{score_M, Hs * 40}, {n_inliers, Hs * 4}, {masks, (size_t)MW * 4}});
    MTRY(orbm_grow(m, 0, 0, (long long)out.words()));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pm = in.add(mask_off, (B + 1) * 8), po = in.add(off, (B + 1) * 4), pu = in.add(uv, N * 16), pp = in.add(pn, N * 16),
              pc = in.add(params, B * sizeof(orbm_init_params)), ph = in.add(hyp_off, (B + 1) * 4), ps = in.add(sets, Hs * 32),
              pmd = in.add(models, Hs * 4);
    MTRY(in.upload(s));
    init_launch(n_problems, H, in.dev_at<int32_t>(po), in.dev_at<float>(pu), in.dev_at<float>(pp), in.dev_at<orbm_init_params>(pc),
                in.dev_at<int32_t>(ph), in.dev_at<int32_t>(ps), in.dev_at<int32_t>(pmd), in.dev_at<int64_t>(pm), out.dev_at<float>(m, 0),
                out.dev_at<int32_t>(m, 1), out.dev_at<uint32_t>(m, 2), s);
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_init_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_uv,
                                           const float *d_pn, const orbm_init_params *d_params, const int32_t *d_hyp_off, const int32_t *d_sets,
                                           const int32_t *d_models, const int64_t *d_mask_off, float *d_score_M, int32_t *d_n_inliers,
                                           uint32_t *d_masks, void *hip_stream)
{
    MTRY(check_problem_count(n_problems));
    if (total_hypotheses < 0) return mfail(ORBX_E_INVALID, "total_hypotheses=%d", total_hypotheses);
    if (n_problems == 0 || total_hypotheses == 0) return ORBX_OK;
    if (any_null(d_off, d_uv, d_pn, d_params, d_hyp_off, d_sets, d_models, d_mask_off, d_score_M, d_n_inliers, d_masks))
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_off, d_uv, d_pn, d_params, d_hyp_off, d_sets, d_models, d_score_M, d_n_inliers, d_masks) || misaligned(7, d_mask_off))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned, mask_off 8-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    init_launch(n_problems, total_hypotheses, d_off, d_uv, d_pn, d_params, d_hyp_off, d_sets, d_models, d_mask_off, d_score_M, d_n_inliers,
                d_masks, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

static int rt_check_counts(int n, int n_motions)
{
    if (n < 0 || n_motions < 0) return mfail(ORBX_E_INVALID, "n=%d n_motions=%d", n, n_motions);
    if (n > (1 << 24) || n_motions > ORBM_INIT_MAX_MOTIONS) return mfail(ORBX_E_CAPACITY, "request beyond 2^24 matches / %d motions", ORBM_INIT_MAX_MOTIONS);
    return ORBX_OK;
}

static void rt_launch(int n, int n_motions, const float *uv, const uint8_t *inliers, const float *Rt, const float *K, float th2, uint8_t *status,
                      float *cosp, float *p3d, hipStream_t s)
{
    const long long pairs = (long long)n * n_motions;
    hipLaunchKernelGGL(k_init_check_rt, dim3((unsigned)((pairs + M_THREADS - 1) / M_THREADS)), dim3(M_THREADS), 0, s, n, n_motions, uv, inliers, Rt,
                       K[0], K[1], K[2], K[3], th2, status, cosp, p3d);
}

extern "C" int orbm_init_check_rt(orbm_matcher *m, int n, const float *uv, const uint8_t *inliers, const float *K, float th2, int n_motions,
                                  const float *Rt, uint8_t *status, float *cos_parallax, float *p3d)
{
    MTRY(rt_check_counts(n, n_motions));
    if (n == 0 || n_motions == 0) return ORBX_OK;
    if (any_null(uv, inliers, K, Rt, status, cos_parallax, p3d)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out holds the points (3 floats per pair), the cosines, then the status bytes
    const size_t pairs = (size_t)n * n_motions;
    const OutBlock out({{p3d, pairs * 12}, {cos_parallax, pairs * 4}, {status, pairs}});
    MTRY(orbm_grow(m, 0, 0, (long long)out.words()));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pu = in.add(uv, (size_t)n * 16), pr = in.add(Rt, (size_t)n_motions * 48), pi = in.add(inliers, (size_t)n);
    MTRY(in.upload(s));
    rt_launch(n, n_motions, in.dev_at<float>(pu), in.dev_at<uint8_t>(pi), in.dev_at<float>(pr), K, th2, out.dev_at<uint8_t>(m, 2),
              out.dev_at<float>(m, 1), out.dev_at<float>(m, 0), s);
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_init_check_rt_device(orbm_matcher *m, int n, const float *d_uv, const uint8_t *d_inliers, const float *K, float th2,
                                         int n_motions, const float *d_Rt, uint8_t *d_status, float *d_cos_parallax, float *d_p3d, void *hip_stream)
{
    MTRY(rt_check_counts(n, n_motions));
    if (n == 0 || n_motions == 0) return ORBX_OK;
    if (any_null(d_uv, d_inliers, K, d_Rt, d_status, d_cos_parallax, d_p3d)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_uv, d_Rt, d_cos_parallax, d_p3d))
        return mfail(ORBX_E_INVALID, "device float arrays must be 4-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    rt_launch(n, n_motions, d_uv, d_inliers, d_Rt, K, th2, d_status, d_cos_parallax, d_p3d, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
