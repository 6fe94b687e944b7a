// orbm_triangulate.hip -- the per-match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:288-434 of WChen09/My-SLAM)
// for all matches of a call in one launch: orbm_triangulate_matches / orbm_triangulate_matches_device (include/orbm.h).
//
// One lane per match, wave64, one wave per workgroup (a few hundred to a few thousand matches: the waves spread over the CUs).
// The camera blocks are read at wave-uniform addresses (scalar loads): key frame 1 has one block, and the lanes of a wave are
// served one second view at a time (with one second view per call, the reference's own use, that is one pass).  The kernel body is
// tri_lanes() (orbm_tri_body.h), which k_triangulate_queries (orbm_newpoints.hip) instantiates as well.
//
// Arithmetic: the reference's float expressions, operation by operation, no contraction -- 3x3 * 3x1 products
// as cv::gemm's small-matrix path (float sum left to right, then (float)(t0*alpha + c*beta) in double), Mat::dot and cv::norm
// accumulated in double, `alpha*row - row` (:325-328) as cv::addWeighted's float kernel evaluates it in double, double constants
// compared in double, cos / atan2 of :314 / :316 correctly rounded.  The 4x4 cv::SVD of :331 is NOT imitated: the right singular
// vector of the smallest singular value comes from a one-sided (Hestenes) Jacobi in fp64 on the float matrix, at most
// TRI_MAX_SWEEPS sweeps, + - * / sqrt only; x3D = v[0:3] / v[3] is rounded to float once.  tests/triangulation_oracle.py is the
// same sequence of operations in numpy.
//
// The two 4x4 fp64 matrices of the Jacobi live in named registers (D4 columns, every access a compile-time member): a private
// array indexed by a loop variable would go to scratch memory.
#include "orbm_internal.h"
#include "orbm_tri_body.h"

__global__ __launch_bounds__(TRI_THREADS) void k_triangulate(
    const orbm_camera *__restrict__ cam1, const orbx_keypoint *__restrict__ kps1, const float2 *__restrict__ keys1,
    const float *__restrict__ ur1, const float *__restrict__ depth1, int n1,
    const orbm_camera *__restrict__ cams2, int ncams2, const int32_t *__restrict__ off2, const orbx_keypoint *__restrict__ kps2,
    const float2 *__restrict__ keys2, const float *__restrict__ ur2, const float *__restrict__ depth2,
    const int32_t *__restrict__ matches, int n, uint8_t *__restrict__ status, float *__restrict__ x3d)
{
    tri_lanes(blockIdx.x * TRI_THREADS + threadIdx.x, n,
              [&](int k, int &idx1, int &idx2, int &v) {
                  idx1 = matches[3 * (long long)k]; idx2 = matches[3 * (long long)k + 1]; v = matches[3 * (long long)k + 2];
                  return true;
              },
              cam1, kps1, keys1, ur1, depth1, n1, cams2, ncams2, off2, kps2, keys2, ur2, depth2, status, x3d);
}

static void tri_launch(const orbm_camera *cam1, const orbx_keypoint *kps1, const float *keys1, const float *ur1, const float *depth1, int n1,
                       const orbm_camera *cams2, int ncams2, const int32_t *off2, const orbx_keypoint *kps2, const float *keys2,
                       const float *ur2, const float *depth2, const int32_t *matches, int n, uint8_t *status, float *x3d, hipStream_t s)
{
    hipLaunchKernelGGL(k_triangulate, dim3((n + TRI_THREADS - 1) / TRI_THREADS), dim3(TRI_THREADS), 0, s, cam1, kps1,
                       reinterpret_cast<const float2 *>(keys1), ur1, depth1, n1, cams2, ncams2, off2, kps2,
                       reinterpret_cast<const float2 *>(keys2), ur2, depth2, matches, n, status, x3d);
}

// the cameras and the feature ranges of the second views, as both entry points that take them from the host require them
int orbm_tri_check_views(const orbm_camera *cam1, const orbm_camera *cams2, int nviews, const int32_t *off2)
{
    if (cam1->nlevels < 1 || cam1->nlevels > ORBX_MAX_LEVELS) return mfail(ORBX_E_INVALID, "key frame 1 has nlevels=%d", cam1->nlevels);
    if (off2[0] != 0) return mfail(ORBX_E_INVALID, "off2[0] must be 0");
    for (int v = 0; v < nviews; v++) {
        if (off2[v + 1] < off2[v]) return mfail(ORBX_E_INVALID, "off2 not monotone at %d", v);
        if (cams2[v].nlevels < 1 || cams2[v].nlevels > ORBX_MAX_LEVELS) return mfail(ORBX_E_INVALID, "second view %d has nlevels=%d", v, cams2[v].nlevels);
    }
    return ORBX_OK;
}

static int tri_check_counts(int n1, int ncams2, int n)
{
    if (n < 0 || n1 < 0 || ncams2 < 0) return mfail(ORBX_E_INVALID, "n=%d n1=%d ncams2=%d", n, n1, ncams2);
    if (n > (1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 matches");
    return ORBX_OK;
}

extern "C" int orbm_triangulate_matches(orbm_matcher *m, const orbm_camera *cam1, const orbx_keypoint *kps_un1, const float *keys_xy1,
                                        const float *u_right1, const float *depth1, int n1,
                                        const orbm_camera *cams2, int ncams2, const int32_t *off2, const orbx_keypoint *kps_un2,
                                        const float *keys_xy2, const float *u_right2, const float *depth2,
                                        const int32_t *matches, int n, uint8_t *status, float *x3d)
{
    MTRY(tri_check_counts(n1, ncams2, n));
    if (n == 0) return ORBX_OK;
    if (!cam1 || !cams2 || !off2 || !kps_un1 || !keys_xy1 || !u_right1 || !depth1 || !kps_un2 || !keys_xy2 || !u_right2 || !depth2 ||
        !matches || !status || !x3d)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (ncams2 < 1) return mfail(ORBX_E_INVALID, "ncams2=%d with n=%d matches", ncams2, n);
    MTRY(orbm_tri_check_views(cam1, cams2, ncams2, off2));
    const int n2 = off2[ncams2];
    for (int k = 0; k < n; k++) {
        const int idx1 = matches[3 * (size_t)k], idx2 = matches[3 * (size_t)k + 1], v = matches[3 * (size_t)k + 2];
        if (v < 0 || v >= ncams2) return mfail(ORBX_E_INVALID, "match %d: view %d outside [0,%d)", k, v, ncams2);
        if (idx1 < 0 || idx1 >= n1) return mfail(ORBX_E_INVALID, "match %d: feature index %d outside [0,%d)", k, idx1, n1);
        if (idx2 < 0 || idx2 >= off2[v + 1] - off2[v]) return mfail(ORBX_E_INVALID, "match %d: feature index %d outside [0,%d)", k, idx2, off2[v + 1] - off2[v]);
        const int o1 = kps_un1[idx1].octave, o2 = kps_un2[(size_t)off2[v] + idx2].octave;
        if (o1 < 0 || o1 >= cam1->nlevels) return mfail(ORBX_E_INVALID, "match %d: octave %d of %d levels", k, o1, cam1->nlevels);
        if (o2 < 0 || o2 >= cams2[v].nlevels) return mfail(ORBX_E_INVALID, "match %d: octave %d of %d levels", k, o2, cams2[v].nlevels);
    }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, ((long long)4 * n + 2) / 3, 0, 0));          // d_out holds 3 * max_q ints: x3d (3 n floats), then status (n bytes)
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pc1 = in.add(cam1, sizeof(orbm_camera)), pc2 = in.add(cams2, (size_t)ncams2 * sizeof(orbm_camera)), po = in.add(off2, ((size_t)ncams2 + 1) * 4);
    const int pk1 = in.add(kps_un1, (size_t)n1 * sizeof(orbx_keypoint)), px1 = in.add(keys_xy1, (size_t)n1 * 8), pu1 = in.add(u_right1, (size_t)n1 * 4), pd1 = in.add(depth1, (size_t)n1 * 4);
    const int pk2 = in.add(kps_un2, (size_t)n2 * sizeof(orbx_keypoint)), px2 = in.add(keys_xy2, (size_t)n2 * 8), pu2 = in.add(u_right2, (size_t)n2 * 4), pd2 = in.add(depth2, (size_t)n2 * 4);
    const int pm = in.add(matches, (size_t)n * 12);
    MTRY(in.upload(s));
    float *d_x3d = reinterpret_cast<float *>(m->d_out.get());
    uint8_t *d_status = reinterpret_cast<uint8_t *>(m->d_out + 3 * (size_t)n);
    tri_launch(in.at<orbm_camera>(pc1), in.at<orbx_keypoint>(pk1), in.at<float>(px1), in.at<float>(pu1), in.at<float>(pd1), n1,
               in.at<orbm_camera>(pc2), ncams2, in.at<int32_t>(po), in.at<orbx_keypoint>(pk2), in.at<float>(px2), in.at<float>(pu2), in.at<float>(pd2),
               in.at<int32_t>(pm), n, d_status, d_x3d, s);
    MHIPCHK(hipGetLastError());
    void *host[2] = {x3d, status};
    const size_t parts[2] = {(size_t)n * 12, (size_t)n};
    MTRY(orbm_d2h_split(m, host, parts, 2, m->d_out, s));
    return orbm_sync(m, s);
}

extern "C" int orbm_triangulate_matches_device(orbm_matcher *m, const orbm_camera *d_cam1, const orbx_keypoint *d_kps_un1,
                                               const float *d_keys_xy1, const float *d_u_right1, const float *d_depth1, int n1,
                                               const orbm_camera *d_cams2, int ncams2, const int32_t *d_off2, const orbx_keypoint *d_kps_un2,
                                               const float *d_keys_xy2, const float *d_u_right2, const float *d_depth2,
                                               const int32_t *d_matches, int n, uint8_t *d_status, float *d_x3d, void *hip_stream)
{
    MTRY(tri_check_counts(n1, ncams2, n));
    if (n == 0) return ORBX_OK;
    if (!d_cam1 || !d_cams2 || !d_off2 || !d_kps_un1 || !d_keys_xy1 || !d_u_right1 || !d_depth1 || !d_kps_un2 || !d_keys_xy2 || !d_u_right2 ||
        !d_depth2 || !d_matches || !d_status || !d_x3d)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (ncams2 < 1) return mfail(ORBX_E_INVALID, "ncams2=%d with n=%d matches", ncams2, n);
    if (((uintptr_t)d_keys_xy1 | (uintptr_t)d_keys_xy2) & 7) return mfail(ORBX_E_INVALID, "d_keys_xy must be 8-byte aligned");
    if (((uintptr_t)d_cam1 | (uintptr_t)d_cams2 | (uintptr_t)d_kps_un1 | (uintptr_t)d_kps_un2 | (uintptr_t)d_matches | (uintptr_t)d_off2) & 3)
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    tri_launch(d_cam1, d_kps_un1, d_keys_xy1, d_u_right1, d_depth1, n1, d_cams2, ncams2, d_off2, d_kps_un2, d_keys_xy2, d_u_right2, d_depth2,
               d_matches, n, d_status, d_x3d, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
