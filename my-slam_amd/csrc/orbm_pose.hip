// orbm_pose.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:239-451 of WChen09/My-SLAM, on g2o) for a batch of independent
// problems in one launch: the frames of a step, or the candidate key frames of Tracking::Relocalization (src/Tracking.cc:1447-1478).
// orbm_pose_optimization_batch / orbm_pose_optimization_batch_device (include/orbm.h).  The arithmetic is csrc/orbp_pose_body.h, the
// text the host path orbp_pose_optimization (orbp_pose.cc) runs as well; this file owns the order of the sums over the edges
// (DESIGN.md section 14).
//
// One workgroup of 256 threads per problem; thread t owns the edges t, t + 256, ... of its problem in every pass, so no edge's flag
// is read by a thread that did not write it.  The pose, the Levenberg state and the 6x6 solve are held redundantly by every thread:
// all of them read the same reduced sums from one LDS block after a barrier, hence take the same branches, and every barrier is
// reached by the whole workgroup.  The loops are bounded at compile time (4 rounds x 10 iterations x 10 trials); there is no wait
// on another workgroup and no atomic.
//
// Sums over edges (the 21 + 6 entries of the normal equations and the robust chi2): every thread adds its own edges in ascending
// order from 0, then a fixed tree: 8 threads per sum add 32 of the 256 partials each (partial k*8 + c for k = 0..31), one thread
// adds those 8 as ((0+1)+(2+3))+((4+5)+(6+7)).  The result depends on the problem alone, not on the batch around it.
#include "orbm_hyp.h"
#include "orbp_pose_body.h"

#define POSE_THREADS 256
#define POSE_PSTRIDE (POSE_THREADS + 8)         // partial row stride (doubles): the 8 threads of a sum read different banks

// The fixed tree of the file comment: acc[v] of every thread -> the same total in acc[v] of every thread.  Three barriers, each
// reached by the whole workgroup.
template <int NV>
__device__ __forceinline__ void pose_reduce(double (&acc)[NV], double *part, double *mid, double *out)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int v = 0; v < NV; v++) part[v * POSE_PSTRIDE + tid] = acc[v];
    __syncthreads();
    if (tid < NV * 8) {
        const int v = tid >> 3, c = tid & 7;
        double s = 0;
#pragma unroll 8
        for (int k = 0; k < POSE_THREADS / 8; k++) s += part[v * POSE_PSTRIDE + k * 8 + c];
        mid[tid] = s;
    }
    __syncthreads();
    if (tid < NV) {
        const double *q = mid + 8 * tid;
        out[tid] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = out[v];
}

// The passes of a problem for pose_rounds: a thread's edges in ascending order, then the tree
struct PoseBlock {
    PoseCam cam;
    PoseEdges E;
    int n;
    double *part, *mid, *out;

    template <bool SYSTEM>
    __device__ __forceinline__ void pass(const Se3 &T, bool robust, double (&acc)[SYSTEM ? POSE_NSYS : 1])
    {
        constexpr int NV = SYSTEM ? POSE_NSYS : 1;
#pragma unroll
        for (int v = 0; v < NV; v++) acc[v] = 0;
        for (int i = threadIdx.x; i < n; i += POSE_THREADS)
            if (!E.outlier[i]) {
                PoseEdge e;
                pose_edge_load(e, E, i);
                pose_edge_error(e, T, cam);
                pose_edge_sums<SYSTEM>(e, cam, robust, acc);
            }
        pose_reduce<NV>(acc, part, mid, out);
    }
    __device__ __forceinline__ void system(const Se3 &T, bool robust, double (&sys)[POSE_NSYS]) { pass<true>(T, robust, sys); }
    __device__ __forceinline__ double chi2(const Se3 &T, bool robust)
    {
        double acc[1];
        pass<false>(T, robust, acc);
        return acc[0];
    }
    __device__ __forceinline__ int flag(const Se3 &est, const Se3 &err_est)
    {
        double bad[1] = {0};
        for (int i = threadIdx.x; i < n; i += POSE_THREADS) {
            PoseEdge e;
            pose_edge_load(e, E, i);
            pose_edge_error(e, E.outlier[i] ? est : err_est, cam);
            const bool o = pose_edge_is_outlier(e);
            E.outlier[i] = o ? 1 : 0;
            bad[0] += o ? 1.0 : 0.0;
        }
        pose_reduce<1>(bad, part, mid, out);    // a count: exact in double
        return (int)bad[0];
    }
};

__global__ __launch_bounds__(POSE_THREADS) void k_pose_optimization(
    const int32_t *__restrict__ off, const float *__restrict__ obs_all, const float *__restrict__ u_right_all,
    const float *__restrict__ inv_sigma2_all, const float *__restrict__ xw_all, const orbm_pose_camera *__restrict__ cams,
    const float *Tcw_in, float *Tcw_out, uint8_t *outlier_all, int32_t *__restrict__ n_good)
{
    __shared__ double part[POSE_NSYS * POSE_PSTRIDE];
    __shared__ double mid[POSE_NSYS * 8];
    __shared__ double out[POSE_NSYS];
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long e0 = off[p];
    PoseBlock B;
    B.n = off[p + 1] - off[p];
    B.E = {obs_all + 2 * e0, u_right_all ? u_right_all + e0 : nullptr, inv_sigma2_all + e0, xw_all + 3 * e0, outlier_all + e0};
    B.part = part; B.mid = mid; B.out = out;
    const float *Tin = Tcw_in + 16 * (long long)p;
    float *Tout = Tcw_out + 16 * (long long)p;

    for (int i = tid; i < B.n; i += POSE_THREADS) B.E.outlier[i] = 0;
    if (B.n < 3) {                              // src/Optimizer.cc:363-364: the pose stays as it came
        if (Tin != Tout && tid < 16) Tout[tid] = Tin[tid];
        if (tid == 0) n_good[p] = 0;
        return;
    }
    B.cam = {cams[p].fx, cams[p].fy, cams[p].cx, cams[p].cy, cams[p].bf};
    const Se3 init = se3_from_Tcw(Tin);
    Se3 est;
    const int n_bad = pose_rounds(B, B.n, init, est);
    if (tid == 0) {
        se3_to_Tcw(est, Tout);
        n_good[p] = B.n - n_bad;
    }
}

extern "C" int orbm_pose_optimization_batch(orbm_matcher *m, int n_problems, const int32_t *off, const float *obs, const float *u_right,
                                            const float *inv_sigma2, const float *xw, const orbm_pose_camera *cams, float *Tcw,
                                            uint8_t *outlier, int32_t *n_good)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(off, cams, Tcw, n_good)) return mfail(ORBX_E_INVALID, "NULL buffer");
    int total;
    MTRY(check_off_csr(n_problems, off, "observations", total));
    if (total > 0 && any_null(obs, inv_sigma2, xw, outlier)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (u_right)
        for (int p = 0; p < n_problems; p++) {
            if (cams[p].bf != 0.0f) continue;
            for (int i = off[p]; i < off[p + 1]; i++)
                if (u_right[i] >= 0) return mfail(ORBX_E_INVALID, "problem %d has a stereo edge (u_right[%d] >= 0) but its camera's bf is 0", p, i);
        }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    // d_out (3 * max_q ints) holds the poses, the counts, then the flags
    const size_t B = (size_t)n_problems, N = (size_t)total;
    const OutBlock out({{Tcw, B * 64}, {n_good, B * 4}, {outlier, N}});
    MTRY(orbm_grow(m, (long long)((out.words() + 2) / 3), 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int po = in.add(off, (B + 1) * 4), pb = in.add(obs, N * 8), pu = in.add(u_right, u_right ? N * 4 : 0), pi = in.add(inv_sigma2, N * 4),
              px = in.add(xw, N * 12), pc = in.add(cams, B * sizeof(orbm_pose_camera)), pt = in.add(Tcw, B * 64);
    MTRY(in.upload(s));
    hipLaunchKernelGGL(k_pose_optimization, dim3(n_problems), dim3(POSE_THREADS), 0, s, in.dev_at<int32_t>(po), in.at<float>(pb), in.at<float>(pu),
                       in.at<float>(pi), in.at<float>(px), in.dev_at<orbm_pose_camera>(pc), in.dev_at<float>(pt), out.dev_at<float>(m, 0),
                       out.dev_at<uint8_t>(m, 2), out.dev_at<int32_t>(m, 1));
    MHIPCHK(hipGetLastError());
    return out.download(m, s);
}

extern "C" int orbm_pose_optimization_batch_device(orbm_matcher *m, int n_problems, const int32_t *d_off, const float *d_obs,
                                                   const float *d_u_right, const float *d_inv_sigma2, const float *d_xw,
                                                   const orbm_pose_camera *d_cams, float *d_Tcw, uint8_t *d_outlier, int32_t *d_n_good,
                                                   void *hip_stream)
{
    MTRY(check_problem_count(n_problems));
    if (n_problems == 0) return ORBX_OK;
    if (any_null(d_off, d_obs, d_inv_sigma2, d_xw, d_cams, d_Tcw, d_outlier, d_n_good)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (misaligned(3, d_off, d_obs, d_u_right, d_inv_sigma2, d_xw, d_cams, d_Tcw, d_n_good))
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    hipLaunchKernelGGL(k_pose_optimization, dim3(n_problems), dim3(POSE_THREADS), 0, s, d_off, d_obs, d_u_right, d_inv_sigma2, d_xw, d_cams,
                       d_Tcw, d_Tcw, d_outlier, d_n_good);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
