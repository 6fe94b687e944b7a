// orbm_sim3opt.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241 of WChen09/My-SLAM, on g2o) for a batch of independent
// problems in one launch: the loop candidates of one round of LoopClosing::ComputeSim3 (src/LoopClosing.cc:287-343) that returned a
// Scm.  orbm_optimize_sim3_batch / orbm_optimize_sim3_batch_device (include/orbm.h).  The kernel runs the text of the host path
// orbp_optimize_sim3 (orbp_sim3opt.cc): csrc/orbp_sim3opt_body.h holds the Sim3 algebra, the two computeErrors, the numeric
// Jacobian, Huber, the 7x7 solve and the Levenberg loop for both; only the order of the sums over the pairs differs (DESIGN.md
// section 21).
//
// One workgroup of 256 threads per problem; thread t owns the pairs t, t + 256, ... of its problem in every pass, so no pair's flag
// is read by a thread that did not write it and n has no upper limit.  The estimate, the Levenberg state and the 7x7 solve are held
// redundantly by every thread: all of them read the same reduced sums from LDS after a barrier, hence take the same branches, and
// every barrier is reached by the whole workgroup.  The 15 estimates of a linearisation (the estimate and +-1e-9 along the 7 axes)
// and their inverses are computed once, by threads 0..14, into LDS.  The loops are bounded at compile time ((5 | 10) iterations x 10
// trials); there is no wait on another workgroup and no atomic.
//
// Sums over pairs (the 28 + 7 entries of the normal equations and the robust chi2): every thread adds its own pairs in ascending
// order from 0 (e12 before e21 within a pair), then a fixed tree: inside a wave a butterfly over the lane bits 0, 1, ..., 5 (lane l
// adds the value of lane l ^ 1, then l ^ 2, ... l ^ 32; both partners add the same two numbers, so all 64 lanes end with the same
// bits), then the four wave totals as (w0 + w1) + (w2 + w3).  The result depends on the problem alone, not on the batch around it.
#include "orbm_hyp.h"
#include "orbp_sim3opt_body.h"

#define S3O_THREADS 256
#define S3O_WAVES (S3O_THREADS / 64)

struct S3oShared {
    S3oSim e[S3O_NLIN], inv[S3O_NLIN];          // one linearisation
    double wave[S3O_WAVES][S3O_NSYS];           // the wave totals of one reduction
    double J[14][S3O_THREADS];                  // every thread's 2 x 7 Jacobian of the edge it is at (s3o_edge)
};

// The fixed tree of the file comment: acc[v] of every thread -> the same total in acc[v] of every thread.  Two barriers, each
// reached by the whole workgroup; the second keeps the next reduction's wave totals from overtaking this one's readers.
template <int NV>
__device__ __forceinline__ void s3o_reduce(double *acc, S3oShared &sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        // the butterfly of opt_wave_sum (orbm_opt.h), written out: as a call it leaves this kernel another register allocation
        double a = acc[v];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m, 64);
        if (lane == 0) sh.wave[w][v] = a;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = (sh.wave[0][v] + sh.wave[1][v]) + (sh.wave[2][v] + sh.wave[3][v]);
    __syncthreads();
}

// what s3o_optimize (orbp_sim3opt_body.h) calls: the passes over the active pairs of one problem
struct S3oDeviceProblem {
    int n;
    const float *x1c, *x2c, *obs1, *obs2, *inv_sigma2_1, *inv_sigma2_2;
    S3oCam cam1, cam2;
    double huber_delta;
    bool fix_scale;
    const uint8_t *removed;
    S3oShared *sh;

    __device__ __forceinline__ void system(const S3oSim &T, double *sys) const
    {
        if (threadIdx.x < S3O_NLIN) s3o_lin_entry(T, threadIdx.x, fix_scale, sh->e[threadIdx.x], sh->inv[threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int v = 0; v < S3O_NSYS; v++) sys[v] = 0;
        for (int i = threadIdx.x; i < n; i += S3O_THREADS)
            if (!removed[i])
                s3o_pair<true>(sh->e, sh->inv, cam1, cam2, x1c + 3 * (size_t)i, x2c + 3 * (size_t)i, obs1 + 2 * (size_t)i,
                               obs2 + 2 * (size_t)i, inv_sigma2_1[i], inv_sigma2_2[i], huber_delta, sys, &sh->J[0][threadIdx.x], S3O_THREADS);
        s3o_reduce<S3O_NSYS>(sys, *sh);
    }
    __device__ __forceinline__ double chi2(const S3oSim &T) const
    {
        S3oSim e, inv;
        s3o_lin_entry(T, 0, fix_scale, e, inv);
        double sum[1] = {0};
        for (int i = threadIdx.x; i < n; i += S3O_THREADS)
            if (!removed[i])
                s3o_pair<false>(&e, &inv, cam1, cam2, x1c + 3 * (size_t)i, x2c + 3 * (size_t)i, obs1 + 2 * (size_t)i, obs2 + 2 * (size_t)i,
                                inv_sigma2_1[i], inv_sigma2_2[i], huber_delta, sum, nullptr, 0);
        s3o_reduce<1>(sum, *sh);
        return sum[0];
    }
    __device__ __forceinline__ bool bad(const S3oSim &T, const S3oSim &Tinv, int i, float th2) const
    {
        return s3o_pair_bad(T, Tinv, cam1, cam2, x1c + 3 * (size_t)i, x2c + 3 * (size_t)i, obs1 + 2 * (size_t)i, obs2 + 2 * (size_t)i,
                            inv_sigma2_1[i], inv_sigma2_2[i], th2);
    }
};

__global__ __launch_bounds__(S3O_THREADS) void k_optimize_sim3(
    const int32_t *__restrict__ off, const float *__restrict__ x1c_all, const float *__restrict__ x2c_all,
    const float *__restrict__ obs1_all, const float *__restrict__ obs2_all, const float *__restrict__ inv_sigma2_1_all,
    const float *__restrict__ inv_sigma2_2_all, const float *__restrict__ cams, const float *__restrict__ th2_all,
    const int32_t *__restrict__ fix_scale_all, const double *S12_in, double *S12_out, uint8_t *flags_all, int32_t *__restrict__ n_in)
{
    __shared__ S3oShared sh;
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long e0 = off[p];
    S3oDeviceProblem P;
    P.n = off[p + 1] - off[p];
    P.x1c = x1c_all + 3 * e0; P.x2c = x2c_all + 3 * e0; P.obs1 = obs1_all + 2 * e0; P.obs2 = obs2_all + 2 * e0;
    P.inv_sigma2_1 = inv_sigma2_1_all + e0; P.inv_sigma2_2 = inv_sigma2_2_all + e0;
    const float *K = cams + 8 * (long long)p;
    P.cam1 = {K[0], K[1], K[2], K[3]};
    P.cam2 = {K[4], K[5], K[6], K[7]};
    const float th2 = th2_all[p];
    P.huber_delta = (double)__fsqrt_rn(th2);    // const float deltaHuber = sqrt(th2) (:1095)
    P.fix_scale = fix_scale_all[p] != 0;
    uint8_t *flags = flags_all + e0;
    P.removed = flags;
    P.sh = &sh;
    const int n = P.n;
    const double *Sin = S12_in + 8 * (long long)p;
    double *Sout = S12_out + 8 * (long long)p;

    for (int i = tid; i < n; i += S3O_THREADS) flags[i] = 0;
    S3oSim est = {{Sin[0], Sin[1], Sin[2], Sin[3]}, Sin[4], Sin[5], Sin[6], Sin[7]};
    const S3oSim init = est;
    S3oSim err_est = est;
    if (n > 0) s3o_optimize(P, est, err_est, P.fix_scale, 5);                      // :1182
    double bad[1] = {0};
    {
        const S3oSim inv = s3o_inverse(err_est);
        for (int i = tid; i < n; i += S3O_THREADS) {
            const bool b = P.bad(err_est, inv, i, th2);
            flags[i] = b ? 1 : 0;
            bad[0] += b ? 1.0 : 0.0;
        }
    }
    s3o_reduce<1>(bad, sh);                     // a count: exact in double
    const int n_bad = (int)bad[0];
    if (n - n_bad < 10) {                       // :1211-1212: g2oS12 stays as it came
        if (tid == 0) {
            if (Sin != Sout) {
                Sout[0] = init.qx; Sout[1] = init.qy; Sout[2] = init.qz; Sout[3] = init.qw;
                Sout[4] = init.t0; Sout[5] = init.t1; Sout[6] = init.t2; Sout[7] = init.s;
            }
            n_in[p] = 0;
        }
        return;
    }
    s3o_optimize(P, est, err_est, P.fix_scale, n_bad > 0 ? 10 : 5);                // :1205-1217
    double good[1] = {0};
    {
        const S3oSim inv = s3o_inverse(err_est);
        for (int i = tid; i < n; i += S3O_THREADS) {
            if (flags[i]) continue;
            if (P.bad(err_est, inv, i, th2)) flags[i] = 1;
            else good[0] += 1.0;
        }
    }
    s3o_reduce<1>(good, sh);
    if (tid == 0) {
        Sout[0] = est.qx; Sout[1] = est.qy; Sout[2] = est.qz; Sout[3] = est.qw;
        Sout[4] = est.t0; Sout[5] = est.t1; Sout[6] = est.t2; Sout[7] = est.s;
        n_in[p] = (int)good[0];
    }
}

extern "C" int orbm_optimize_sim3_batch(orbm_matcher *m, int n_problems, const int32_t *off, const float *x1c, const float *x2c,
                                        const float *obs1, const float *obs2, const float *inv_sigma2_1, const float *inv_sigma2_2,
                                        const float *cams, const float *th2, const int32_t *fix_scale, double *S12, uint8_t *flags,
                                        int32_t *n_in)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(off, cams, th2, fix_scale, S12, n_in)) return mfail(ORBX_E_INVALID, "NULL buffer");
    int total;
    MTRY(check_off_csr(n_problems, off, "pairs", total));
    if (total > 0 && any_null(x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, flags)) return mfail(ORBX_E_INVALID, "NULL buffer");
    for (size_t i = 0; i < 8 * (size_t)n_problems; i++)
        if (!std::isfinite(S12[i])) return mfail(ORBX_E_INVALID, "S12 of problem %d is not finite", (int)(i / 8));
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out (3 * max_q ints) holds S12 (16 words a problem), the counts, then the flags
    const size_t B = (size_t)n_problems, N = (size_t)total;
    const OutBlock out({{S12, B * 64}, {n_in, B * 4}, {flags, N}});
    MTRY(orbm_grow(m, (long long)((out.words() + 2) / 3), 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int po = in.add(off, (B + 1) * 4), pa = in.add(x1c, N * 12), pb = in.add(x2c, N * 12), pc = in.add(obs1, N * 8),
              pd = in.add(obs2, N * 8), pe = in.add(inv_sigma2_1, N * 4), pf = in.add(inv_sigma2_2, N * 4), pk = in.add(cams, B * 32),
              pt = in.add(th2, B * 4), px = in.add(fix_scale, B * 4), ps = in.add(S12, B * 64);
    MTRY(in.upload(s));
    hipLaunchKernelGGL(k_optimize_sim3, dim3(n_problems), dim3(S3O_THREADS), 0, s, in.dev_at<int32_t>(po), in.at<float>(pa), in.at<float>(pb),
                       in.at<float>(pc), in.at<float>(pd), in.at<float>(pe), in.at<float>(pf), in.dev_at<float>(pk), in.dev_at<float>(pt),
                       in.dev_at<int32_t>(px), in.dev_at<double>(ps), out.dev_at<double>(m, 0), out.dev_at<uint8_t>(m, 2),
                       out.dev_at<int32_t>(m, 1));
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_optimize_sim3_batch_device(orbm_matcher *m, int n_problems, const int32_t *d_off, const float *d_x1c, const float *d_x2c,
                                               const float *d_obs1, const float *d_obs2, const float *d_inv_sigma2_1,
                                               const float *d_inv_sigma2_2, const float *d_cams, const float *d_th2,
                                               const int32_t *d_fix_scale, double *d_S12, uint8_t *d_flags, int32_t *d_n_in, void *hip_stream)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(d_off, d_x1c, d_x2c, d_obs1, d_obs2, d_inv_sigma2_1, d_inv_sigma2_2, d_cams, d_th2, d_fix_scale, d_S12, d_flags, d_n_in))
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_off, d_x1c, d_x2c, d_obs1, d_obs2, d_inv_sigma2_1, d_inv_sigma2_2, d_cams, d_th2, d_fix_scale, d_n_in))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned");
    if (misaligned(7, d_S12)) return mfail(ORBX_E_INVALID, "d_S12 must be 8-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    hipLaunchKernelGGL(k_optimize_sim3, dim3(n_problems), dim3(S3O_THREADS), 0, s, d_off, d_x1c, d_x2c, d_obs1, d_obs2, d_inv_sigma2_1,
                       d_inv_sigma2_2, d_cams, d_th2, d_fix_scale, d_S12, d_S12, d_flags, d_n_in);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
