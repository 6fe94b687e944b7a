// orbm_frustum.hip -- Frame::isInFrustum (src/Frame.cc:269-325 of WChen09/My-SLAM) for every local MapPoint of a frame in one
// launch: the loop of Tracking::SearchLocalPoints (src/Tracking.cc:1174-1187).  orbm_frustum / orbm_frustum_device
// (include/orbm.h); orbm_search_local_points (orbm_grid.hip) launches the same kernel with the window outputs switched on.
//
// One lane per MapPoint, wave64, one wave per workgroup (a few thousand points: the waves spread over the CUs).  The frame block
// is read at wave-uniform addresses (scalar loads).  No loops, no LDS, no scratch.
//
// Arithmetic: the reference's float expressions, operation by operation, no contraction -- Pc = mRcw*P+mtcw
// as cv::gemm's small-matrix path (float sum left to right, then (float)(t0*alpha + c*beta) in double), 1.0f/PcZ a float division,
// cv::norm and Mat::dot accumulated in double, viewCos = dot / (double)dist rounded to float once, MapPoint::PredictScale
// (src/MapPoint.cc:402-417) as float division, logf, float division, ceil.  logf is the correctly rounded fp32 logarithm: the
// fp64 log rounded to float once.  tests/frustum_oracle.py is the same sequence of operations in numpy.
#include "orbm_internal.h"
#include "orbm_project.h"

#define FRU_THREADS 64

// fru_gemm_row, fru_dot3, fru_predict_scale: orbm_project.h (shared with orbm_fuse.hip)

struct FruOut { float u, v, ur, view_cos; int level; };

// Frame::isInFrustum for one MapPoint; o is valid when the result is ORBM_FRUSTUM_IN_VIEW
__device__ __forceinline__ int fru_one(const orbm_frame_view *__restrict__ V, float Px, float Py, float Pz, float Nx, float Ny, float Nz,
                                       float mf_max, float mf_min, float cos_limit, FruOut &o)
{
    // 3D in camera coordinates :277
    const float PcX = fru_gemm_row(V->Rcw, V->tcw[0], Px, Py, Pz);
    const float PcY = fru_gemm_row(V->Rcw + 3, V->tcw[1], Px, Py, Pz);
    const float PcZ = fru_gemm_row(V->Rcw + 6, V->tcw[2], Px, Py, Pz);
    if (PcZ < 0.0f) return ORBM_FRUSTUM_BEHIND;                                         // :283 (+-0 and NaN pass)
    const float invz = __fdiv_rn(1.0f, PcZ);                                            // :287
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(V->fx, PcX), invz), V->cx);           // :288
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(V->fy, PcY), invz), V->cy);           // :289
    if (u < V->bounds[0] || u > V->bounds[1]) return ORBM_FRUSTUM_OUT_X;                // :291 (NaN passes)
    if (v < V->bounds[2] || v > V->bounds[3]) return ORBM_FRUSTUM_OUT_Y;                // :293
    const float max_distance = __fmul_rn(1.2f, mf_max);                                 // src/MapPoint.cc:382
    const float min_distance = __fmul_rn(0.8f, mf_min);                                 // src/MapPoint.cc:376
    const float POx = __fsub_rn(Px, V->Ow[0]), POy = __fsub_rn(Py, V->Ow[1]), POz = __fsub_rn(Pz, V->Ow[2]);   // :299
    const float dist = (float)sqrt(fru_dot3(POx, POy, POz, POx, POy, POz));             // :300
    if (dist < min_distance || dist > max_distance) return ORBM_FRUSTUM_DISTANCE;       // :302
    const float view_cos = (float)(fru_dot3(POx, POy, POz, Nx, Ny, Nz) / (double)dist); // :308
    if (view_cos < cos_limit) return ORBM_FRUSTUM_VIEW_COS;                             // :310 (NaN passes)
    // MapPoint::PredictScale, src/MapPoint.cc:402-417 (orbm_project.h)
    int level;
    if (!fru_predict_scale(mf_max, dist, V->log_scale_factor, V->nlevels, level)) return ORBM_FRUSTUM_UNDEFINED;
    o.u = u; o.v = v; o.ur = __fsub_rn(u, __fmul_rn(V->mbf, invz)); o.view_cos = view_cos; o.level = level;   // :318-322
    return ORBM_FRUSTUM_IN_VIEW;
}

// WINDOWS: also the window of ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:64-71, :127-133) per point, for
// k_area_list; a point not in view gets a window nothing falls into (r < 0)
template <bool WINDOWS>
__global__ __launch_bounds__(FRU_THREADS) void k_frustum(
    const orbm_frame_view *__restrict__ V, int n, const uint8_t *__restrict__ skip, const float *__restrict__ xw,
    const float *__restrict__ normal, const float *__restrict__ mf_max, const float *__restrict__ mf_min, float cos_limit,
    uint8_t *__restrict__ status, float *__restrict__ proj_x, float *__restrict__ proj_y, float *__restrict__ proj_xr,
    int32_t *__restrict__ pred_level, float *__restrict__ view_cos, float th, float *__restrict__ wx, float *__restrict__ wy,
    float *__restrict__ wr, int32_t *__restrict__ wmin, int32_t *__restrict__ wmax)
{
    const int i = blockIdx.x * FRU_THREADS + threadIdx.x;
    if (i >= n) return;
    FruOut o = {0.f, 0.f, 0.f, 0.f, 0};
    int st = ORBM_FRUSTUM_SKIPPED;
    if (!skip[i]) {
        const long long b = 3 * (long long)i;
        st = fru_one(V, xw[b], xw[b + 1], xw[b + 2], normal[b], normal[b + 1], normal[b + 2], mf_max[i], mf_min[i], cos_limit, o);
    }
    const bool in_view = st == ORBM_FRUSTUM_IN_VIEW;
    status[i] = (uint8_t)st;
    proj_x[i] = in_view ? o.u : 0.f; proj_y[i] = in_view ? o.v : 0.f; proj_xr[i] = in_view ? o.ur : 0.f;
    pred_level[i] = in_view ? o.level : 0; view_cos[i] = in_view ? o.view_cos : 0.f;
    if (WINDOWS) {
        float r = -1.0f;
        if (in_view) {
            r = (double)o.view_cos > 0.998 ? 2.5f : 4.0f;                       // RadiusByViewingCos :127-133
            if (th != 1.0f) r = __fmul_rn(r, th);                               // :49, :67-68
            r = __fmul_rn(r, V->scale_factors[o.level]);                        // :71
        }
        wx[i] = in_view ? o.u : 0.f; wy[i] = in_view ? o.v : 0.f; wr[i] = r;
        wmin[i] = in_view ? o.level - 1 : 0; wmax[i] = in_view ? o.level : 0;
    }
}

void orbm_frustum_launch(const orbm_frame_view *d_view, int n, const uint8_t *d_skip, const float *d_xw, const float *d_normal,
                         const float *d_mf_max, const float *d_mf_min, float cos_limit, uint8_t *d_status, float *d_proj_x,
                         float *d_proj_y, float *d_proj_xr, int32_t *d_pred_level, float *d_view_cos, const FrustumWindows *w,
                         hipStream_t s)
{
    const dim3 grid((n + FRU_THREADS - 1) / FRU_THREADS), block(FRU_THREADS);
    if (w)
        hipLaunchKernelGGL(k_frustum<true>, grid, block, 0, s, d_view, n, d_skip, d_xw, d_normal, d_mf_max, d_mf_min, cos_limit, d_status,
                           d_proj_x, d_proj_y, d_proj_xr, d_pred_level, d_view_cos, w->th, w->x, w->y, w->r, w->min_level, w->max_level);
    else
        hipLaunchKernelGGL(k_frustum<false>, grid, block, 0, s, d_view, n, d_skip, d_xw, d_normal, d_mf_max, d_mf_min, cos_limit, d_status,
                           d_proj_x, d_proj_y, d_proj_xr, d_pred_level, d_view_cos, 1.0f, (float *)nullptr, (float *)nullptr,
                           (float *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
}

// the checks orbm_frustum and orbm_search_local_points share; n > 0
int orbm_frustum_check(const orbm_frame_view *view, const uint8_t *skip, const float *xw, const float *normal, const float *mf_max,
                       const float *mf_min, const uint8_t *status, const float *proj_x, const float *proj_y, const float *proj_xr,
                       const int32_t *pred_level, const float *view_cos, const int *n_to_match)
{
    if (!view || !skip || !xw || !normal || !mf_max || !mf_min || !status || !proj_x || !proj_y || !proj_xr || !pred_level || !view_cos ||
        !n_to_match)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (view->nlevels < 1 || view->nlevels > ORBX_MAX_LEVELS) return mfail(ORBX_E_INVALID, "the frame has nlevels=%d", view->nlevels);
    return ORBX_OK;
}

extern "C" int orbm_frustum(orbm_matcher *m, const orbm_frame_view *view, int n, const uint8_t *skip, const float *xw, const float *normal,
                            const float *mf_max, const float *mf_min, float viewing_cos_limit, uint8_t *status, float *proj_x, float *proj_y,
                            float *proj_xr, int32_t *pred_level, float *view_cos, int *n_to_match)
{
    if (n < 0) return mfail(ORBX_E_INVALID, "n=%d MapPoints", n);
    if (n > (1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 MapPoints");
    if (n == 0) return ORBX_OK;
    MTRY(orbm_frustum_check(view, skip, xw, normal, mf_max, mf_min, status, proj_x, proj_y, proj_xr, pred_level, view_cos, n_to_match));
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, 2ll * n, 0, 0));          // d_out holds 3 * max_q ints: five arrays of n words, then the n status bytes
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pv = in.add(view, sizeof(orbm_frame_view)), ps = in.add(skip, (size_t)n), px = in.add(xw, (size_t)n * 12),
              pn = in.add(normal, (size_t)n * 12), pa = in.add(mf_max, (size_t)n * 4), pi = in.add(mf_min, (size_t)n * 4);
    MTRY(in.upload(s));
    float *o = reinterpret_cast<float *>(m->d_out.get());
    const size_t N = (size_t)n;
    uint8_t *d_status = reinterpret_cast<uint8_t *>(m->d_out + 5 * N);
    orbm_frustum_launch(in.at<orbm_frame_view>(pv), n, in.at<uint8_t>(ps), in.at<float>(px), in.at<float>(pn), in.at<float>(pa),
                        in.at<float>(pi), viewing_cos_limit, d_status, o, o + N, o + 2 * N, m->d_out + 3 * N, o + 4 * N, nullptr, s);
    MHIPCHK(hipGetLastError());
    void *host[6] = {proj_x, proj_y, proj_xr, pred_level, view_cos, status};
    const size_t parts[6] = {N * 4, N * 4, N * 4, N * 4, N * 4, N};
    MTRY(orbm_d2h_split(m, host, parts, 6, m->d_out, s));
    MTRY(orbm_sync(m, s));
    int cnt = 0;
    for (int i = 0; i < n; i++) cnt += status[i] == ORBM_FRUSTUM_IN_VIEW;
    *n_to_match = cnt;                          // nToMatch, src/Tracking.cc:1185
    return ORBX_OK;
}

extern "C" int orbm_frustum_device(orbm_matcher *m, const orbm_frame_view *d_view, int n, const uint8_t *d_skip, const float *d_xw,
                                   const float *d_normal, const float *d_mf_max, const float *d_mf_min, float viewing_cos_limit,
                                   uint8_t *d_status, float *d_proj_x, float *d_proj_y, float *d_proj_xr, int32_t *d_pred_level,
                                   float *d_view_cos, void *hip_stream)
{
    if (n < 0) return mfail(ORBX_E_INVALID, "n=%d MapPoints", n);
    if (n == 0) return ORBX_OK;
    if (!d_view || !d_skip || !d_xw || !d_normal || !d_mf_max || !d_mf_min || !d_status || !d_proj_x || !d_proj_y || !d_proj_xr ||
        !d_pred_level || !d_view_cos)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (((uintptr_t)d_view | (uintptr_t)d_xw | (uintptr_t)d_normal | (uintptr_t)d_mf_max | (uintptr_t)d_mf_min | (uintptr_t)d_proj_x |
         (uintptr_t)d_proj_y | (uintptr_t)d_proj_xr | (uintptr_t)d_pred_level | (uintptr_t)d_view_cos) & 3)
        return mfail(ORBX_E_INVALID, "device arrays must be 4-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    orbm_frustum_launch(d_view, n, d_skip, d_xw, d_normal, d_mf_max, d_mf_min, viewing_cos_limit, d_status, d_proj_x, d_proj_y, d_proj_xr,
                        d_pred_level, d_view_cos, nullptr, s);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}
