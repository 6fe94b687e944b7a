// orbm_grid.hip -- the 64x48 Frame grid and windowed searches on gfx950.
// Reference (WChen09/My-SLAM): src/Frame.cc:230-245 AssignFeaturesToGrid, :382-392 PosInGrid,
// :327-380 GetFeaturesInArea; consumers: ORBmatcher::SearchByProjection (src/ORBmatcher.cc:1397-1430),
// SearchForInitialization (:425-457).  The window maths is fp32 exactly as written there (no
// contraction: __f*_rn); candidate ORDER is the reference's (cell column, cell row, push_back order),
// because "first candidate wins a tie" depends on it.
#include <algorithm>
#include <vector>

#include <climits>
#include <utility>
#include "orbm_window.h"

// -------------------------------------------------------------------------------------------------
// k_grid_build: one 1024-thread workgroup.  Count per cell (LDS atomics) -> scan -> scatter -> each
// cell's short list is sorted ascending, which restores push_back order (keypoint index order).
// grid_build_body is that workgroup's work, shared with k_grid_build_views (one workgroup per key frame of orbm_fuse_views), so the
// push_back order exists once.  LDS: 2 x 3072 + 1 counters and 17 wave sums = 24.1 KB per workgroup; a CU holds two 1024-thread
// workgroups (32 waves), 48 KB of its 160 KB.
// -------------------------------------------------------------------------------------------------
#define G_THREADS 1024
__device__ __forceinline__ void grid_build_body(const OrbmGrid &g, const orbx_keypoint *__restrict__ kps)
{
    __shared__ int cnt[ORBM_GRID_CELLS];
    __shared__ int start[ORBM_GRID_CELLS + 1];
    __shared__ int wsum[G_THREADS / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < ORBM_GRID_CELLS; c += G_THREADS) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < g.n; i += G_THREADS) {
        const orbx_keypoint kp = kps[i];
        g.kx[i] = kp.x; g.ky[i] = kp.y; g.koct[i] = kp.octave;
        const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, g.min_x), g.inv_w));   // PosInGrid :384
        const int py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, g.min_y), g.inv_h));   // :385
        int cell = -1;
        if (px >= 0 && px < ORBM_GRID_COLS && py >= 0 && py < ORBM_GRID_ROWS) {
            cell = px * ORBM_GRID_ROWS + py;
            atomicAdd(&cnt[cell], 1);
        }
        g.cell_of[i] = cell;
    }
    __syncthreads();
    // exclusive scan of 3072 counts: 3 per thread
    const int c0 = tid * 3;
    const int a = cnt[c0], b = cnt[c0 + 1], c = cnt[c0 + 2];
    int inc = a + b + c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        int w = lane < G_THREADS / 64 ? wsum[lane] : 0, wi = w;
#pragma unroll
        for (int o = 1; o < G_THREADS / 64; o <<= 1) {
            const int t = __shfl_up(wi, o);
            if (lane >= o) wi += t;
        }
        if (lane < G_THREADS / 64) wsum[lane] = wi - w;
        if (lane == G_THREADS / 64 - 1) wsum[G_THREADS / 64] = wi;
    }
    __syncthreads();
    const int ex = wsum[wave] + inc - (a + b + c);
    start[c0] = ex; start[c0 + 1] = ex + a; start[c0 + 2] = ex + a + b;
    if (tid == 0) start[ORBM_GRID_CELLS] = wsum[G_THREADS / 64];
    cnt[c0] = 0; cnt[c0 + 1] = 0; cnt[c0 + 2] = 0;
    __syncthreads();
    for (int i = tid; i <= ORBM_GRID_CELLS; i += G_THREADS) g.cell_start[i] = start[i];
    for (int i = tid; i < g.n; i += G_THREADS) {
        const int cell = g.cell_of[i];
        if (cell >= 0) g.items[start[cell] + atomicAdd(&cnt[cell], 1)] = i;
    }
    __syncthreads();
    __threadfence_block();
    for (int cl = tid; cl < ORBM_GRID_CELLS; cl += G_THREADS) {     // insertion sort of a short list
        const int s = start[cl], e = start[cl + 1];
        for (int i = s + 1; i < e; i++) {
            const int v = g.items[i];
            int j = i - 1;
            while (j >= s && g.items[j] > v) { g.items[j + 1] = g.items[j]; j--; }
            g.items[j + 1] = v;
        }
    }
}
__global__ __launch_bounds__(G_THREADS) void k_grid_build(OrbmGrid g, const orbx_keypoint *__restrict__ kps) { grid_build_body(g, kps); }
// one workgroup per view: view blockIdx.x owns grids[blockIdx.x] (its slices of the feature arrays, of items and of cell_start) and the
// keypoints kps + off[blockIdx.x]
__global__ __launch_bounds__(G_THREADS) void k_grid_build_views(const OrbmGrid *__restrict__ grids, const int32_t *__restrict__ off,
                                                               const orbx_keypoint *__restrict__ kps)
{
    const OrbmGrid g = grids[blockIdx.x];
    grid_build_body(g, kps + off[blockIdx.x]);
}
void orbm_grid_build_views_launch(const OrbmGrid *d_grids, const int32_t *d_off, const orbx_keypoint *d_kps, int nviews, hipStream_t s)
{
    hipLaunchKernelGGL(k_grid_build_views, dim3(nviews), dim3(G_THREADS), 0, s, d_grids, d_off, d_kps);
}

// one wave per window; MODE 0 = count, 1 = write the list at off[q] in the reference's order
template <int MODE>
__global__ __launch_bounds__(M_THREADS) void k_area_list(OrbmGrid g, const float *__restrict__ qx, const float *__restrict__ qy,
                                                        const float *__restrict__ qr, const int32_t *__restrict__ minl,
                                                        const int32_t *__restrict__ maxl, int nq,
                                                        int32_t *__restrict__ counts, const int32_t *__restrict__ off,
                                                        int32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (M_THREADS / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int mn = minl[q], mx = maxl[q];
    const int base = MODE == 1 ? off[q] : 0;
    const int n = window_walk(g, x, y, r, lane, [&](int i) { return in_window(g, i, x, y, r, mn, mx); },
                              [&](int i, int pos) { if (MODE == 1) out[base + pos] = i; });
    if (MODE == 0 && lane == 0) counts[q] = n;
}

// fused window query + best / second-best (strict '<': first candidate wins ties, a tie with the best
// becomes the second best).  Key = distance << 22 | position in the reference's candidate order; a keypoint
// masked by skip[] is no member of the window and takes no position.
__global__ __launch_bounds__(M_THREADS) void k_search_area(OrbmGrid g, const uint8_t *__restrict__ qdesc,
                                                          const float *__restrict__ qx, const float *__restrict__ qy,
                                                          const float *__restrict__ qr, const int32_t *__restrict__ minl,
                                                          const int32_t *__restrict__ maxl, int nq,
                                                          const uint8_t *__restrict__ tdesc, const uint8_t *__restrict__ skip,
                                                          int32_t *__restrict__ best_idx, int32_t *__restrict__ best_d,
                                                          int32_t *__restrict__ second_d)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (M_THREADS / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int mn = minl[q], mx = maxl[q];
    const uint4 *Q = reinterpret_cast<const uint4 *>(qdesc) + 2 * (long long)q;
    const uint4 q0 = Q[0], q1 = Q[1];
    const uint32_t none = (256u << 22) | 0x3FFFFFu;
    uint32_t bp = none, s2 = 256;
    int bidx = -1;
    window_walk(g, x, y, r, lane, [&](int i) { return in_window(g, i, x, y, r, mn, mx) && !(skip && skip[i]); },
                [&](int i, int pos) {
                    const uint4 *Tj = reinterpret_cast<const uint4 *>(tdesc) + 2 * (long long)i;
                    const uint32_t d = (uint32_t)hamming256(q0, q1, Tj[0], Tj[1]);
                    const uint32_t p = (d << 22) | (uint32_t)min(pos, 0x3FFFFF);
                    if (p < bp) { s2 = bp >> 22; bp = p; bidx = i; }
                    else if (d < s2) s2 = d;
                });
    uint32_t B, S;
    wave_best2<22>(bp, s2, B, S);
    if (B == none ? lane == 0 : bp == B) {      // positions are unique: one lane holds the winner; an empty window is -1 / 256 / 256
        const int d = (int)(B >> 22);
        best_d[q] = d;
        second_d[q] = (int)S;
        best_idx[q] = d < 256 ? bidx : -1;
    }
}

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
// cv::undistortPoints(src, dst, K, distCoeffs, noArray(), K) of OpenCV 3.1.0 for one point (cvUndistortPoints: camera matrix
// and coefficients converted to double, ITERS = 5, no tilt, R = I, P = K).  Called by Frame::UndistortKeyPoints (src/Frame.cc:421)
// and Frame::ComputeImageBounds (:449).
static inline void undistort_point(float xin, float yin, double fx, double fy, double cx, double cy, const double k[5],
                                   float *xout, float *yout)
{
    const double ifx = 1. / fx, ify = 1. / fy;
    double x = xin, y = yin;
    const double x0 = x = (x - cx) * ifx;
    const double y0 = y = (y - cy) * ify;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);     // k4..k6 = 0
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = fx * x + 0 * y + cx, yy = 0 * x + fy * y + cy, ww = 1. / (0 * x + 0 * y + 1);
    *xout = (float)(xx * ww);
    *yout = (float)(yy * ww);
}

extern "C" int orbm_undistort_keypoints(const orbx_keypoint *kps, int n, float fx, float fy, float cx, float cy,
                                        const float *dist, int ndist, orbx_keypoint *kps_un)
{
    if (n < 0 || (n > 0 && (!kps || !kps_un)) || !dist || (ndist != 4 && ndist != 5)) return mfail(ORBX_E_INVALID, "bad argument");
    if (dist[0] == 0.0f) {                     // :406-410
        if (kps_un != kps) memmove(kps_un, kps, sizeof(orbx_keypoint) * (size_t)n);
        return ORBX_OK;
    }
    const double k[5] = {dist[0], dist[1], dist[2], dist[3], ndist == 5 ? dist[4] : 0.0};
    for (int i = 0; i < n; i++) {
        orbx_keypoint kp = kps[i];
        undistort_point(kps[i].x, kps[i].y, fx, fy, cx, cy, k, &kp.x, &kp.y);
        kps_un[i] = kp;
    }
    return ORBX_OK;
}

extern "C" int orbm_image_bounds(int width, int height, float fx, float fy, float cx, float cy, const float *dist, int ndist,
                                 float bounds[4])
{
    if (!dist || !bounds || (ndist != 4 && ndist != 5)) return mfail(ORBX_E_INVALID, "bad argument");
    if (dist[0] == 0.0f) { bounds[0] = 0.0f; bounds[1] = (float)width; bounds[2] = 0.0f; bounds[3] = (float)height; return ORBX_OK; }
    const double k[5] = {dist[0], dist[1], dist[2], dist[3], ndist == 5 ? dist[4] : 0.0};
    const float cxs[4] = {0.f, (float)width, 0.f, (float)width}, cys[4] = {0.f, 0.f, (float)height, (float)height};
    float ux[4], uy[4];
    for (int i = 0; i < 4; i++) undistort_point(cxs[i], cys[i], fx, fy, cx, cy, k, &ux[i], &uy[i]);
    bounds[0] = std::min(ux[0], ux[2]); bounds[1] = std::max(ux[1], ux[3]);      // :451-454
    bounds[2] = std::min(uy[0], uy[1]); bounds[3] = std::max(uy[2], uy[3]);
    return ORBX_OK;
}

// Builds a grid slot.  The keypoints are staged in the pinned arena of the current call (the caller has run orbm_arena_begin) and
// go to the handle's d_out (a temporary block when that is too small); the kernel is queued on the handle's stream.
int orbm_grid_build_into(orbm_matcher *m, int slot, const orbx_keypoint *kps_un, int n, float assign_min_x, float assign_min_y,
                         float inv_w, float inv_h, float query_min_x, float query_min_y)
{
    MTRY(orbm_grid_ensure(m, slot));
    OrbmGrid &g = slot ? m->grid2 : m->grid;
    g.min_x = assign_min_x; g.min_y = assign_min_y; g.inv_w = inv_w; g.inv_h = inv_h; g.qmin_x = query_min_x; g.qmin_y = query_min_y;
    g.n = n;
    hipStream_t s = m->stream;
    orbx_keypoint *d_kps = reinterpret_cast<orbx_keypoint *>(m->d_out.get());
    const size_t need = (size_t)n * sizeof(orbx_keypoint);
    DevBuf<orbx_keypoint> tmp;                 // freed on every return path; on success after the synchronisation below
    if (need > m->d_out.bytes()) { MTRY(tmp.grow(need, mfail, "grid keypoint staging")); d_kps = tmp; }
    if (n > 0) MTRY(orbm_h2d(m, d_kps, kps_un, need, s));
    hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(G_THREADS), 0, s, g, d_kps);
    MHIPCHK(hipGetLastError());
    if (tmp) MHIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

// the body of orbm_grid_build / orbm_grid_build_kf: slot `grid` of the handle, synchronous
static int grid_build(orbm_matcher *m, const orbx_keypoint *kps_un, int n, float assign_min_x, float assign_min_y, float inv_w, float inv_h,
                      float query_min_x, float query_min_y)
{
    MHIPCHK(hipSetDevice(m->device));
    m->grid_ok = false;
    MTRY(orbm_grow(m, 0, n, 0));
    MTRY(orbm_arena_begin(m));
    MTRY(orbm_grid_build_into(m, 0, kps_un, n, assign_min_x, assign_min_y, inv_w, inv_h, query_min_x, query_min_y));
    MTRY(orbm_sync(m, m->stream));
    m->grid_ok = true;
    return ORBX_OK;
}

extern "C" int orbm_grid_build(orbm_matcher *m, const orbx_keypoint *kps_un, int n,
                               float min_x, float max_x, float min_y, float max_y)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n < 0) return mfail(ORBX_E_INVALID, "n=%d keypoints", n);
    if (n > 0 && !kps_un) return mfail(ORBX_E_INVALID, "NULL keypoints");
    if (!(max_x > min_x) || !(max_y > min_y)) return mfail(ORBX_E_INVALID, "empty image bounds");
    return grid_build(m, kps_un, n, min_x, min_y, (float)ORBM_GRID_COLS / (max_x - min_x),     // src/Frame.cc:212
                      (float)ORBM_GRID_ROWS / (max_y - min_y), min_x, min_y);                  // :213
}

// number of keypoints in the handle's grid, -1 when there is none (never built, or dropped by a workspace growth)
extern "C" int orbm_grid_count(const orbm_matcher *m) { return (m && m->grid_ok) ? m->grid.n : -1; }

// A key frame's grid.  KeyFrame copies mGrid from the Frame it was made of (src/KeyFrame.cc:48-54), so the cells were filled by
// Frame::PosInGrid with Frame's float mnMinX / mnMinY and mfGridElementWidthInv / HeightInv (src/Frame.cc:382-392: assign_*, inv_*),
// while KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-606) subtracts the key frame's own mnMinX / mnMinY, which are ints
// (include/KeyFrame.h:190-193: query_*).  With the shipped calibration (k1 == 0) the two origins coincide.
extern "C" int orbm_grid_build_kf(orbm_matcher *m, const orbx_keypoint *kps_un, int n, float assign_min_x, float assign_min_y,
                                  float inv_w, float inv_h, float query_min_x, float query_min_y)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n < 0) return mfail(ORBX_E_INVALID, "n=%d keypoints", n);
    if (n > 0 && !kps_un) return mfail(ORBX_E_INVALID, "NULL keypoints");
    if (!(inv_w > 0.f) || !(inv_h > 0.f)) return mfail(ORBX_E_INVALID, "grid cell sizes must be positive");
    return grid_build(m, kps_un, n, assign_min_x, assign_min_y, inv_w, inv_h, query_min_x, query_min_y);
}

// The window arrays of nq queries as parts of a call's input block, and the two passes of k_area_list over them.  The counts of
// pass 0 land in d_out[0, nq) (nq <= max_q: the caller has grown the handle), which is free until the distances are queued.
struct WindowParts {
    int x, y, r, mn, mx;
    WindowParts(InBlock &in, const float *qx, const float *qy, const float *qr, const int32_t *min_level, const int32_t *max_level, int nq)
        : x(in.add(qx, (size_t)nq * 4)), y(in.add(qy, (size_t)nq * 4)), r(in.add(qr, (size_t)nq * 4)),
          mn(in.add(min_level, (size_t)nq * 4)), mx(in.add(max_level, (size_t)nq * 4)) {}
    WindowParts(InBlock &in, int nq)            // room only: a kernel writes the windows
        : x(in.reserve((size_t)nq * 4)), y(in.reserve((size_t)nq * 4)), r(in.reserve((size_t)nq * 4)), mn(in.reserve((size_t)nq * 4)),
          mx(in.reserve((size_t)nq * 4)) {}
};
template <int MODE>
static int launch_area_list(orbm_matcher *m, const InBlock &in, const WindowParts &w, int nq, int32_t *d_counts, const int32_t *d_off,
                            int32_t *d_list, hipStream_t s)
{
    hipLaunchKernelGGL(k_area_list<MODE>, dim3((nq + 3) / 4), dim3(M_THREADS), 0, s, m->grid, in.at<float>(w.x), in.at<float>(w.y),
                       in.at<float>(w.r), in.at<int32_t>(w.mn), in.at<int32_t>(w.mx), nq, d_counts, d_off, d_list);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_features_in_area(orbm_matcher *m, const float *x, const float *y, const float *r,
                                     const int32_t *min_level, const int32_t *max_level, int nq,
                                     int32_t *cand_off, int32_t *cand_idx, int cap_idx)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (!m->grid_ok) return mfail(ORBX_E_INVALID, "orbm_grid_build has not been called");
    if (nq < 0 || !cand_off) return mfail(ORBX_E_INVALID, "bad argument");
    cand_off[0] = 0;
    if (nq == 0) return 0;
    if (!x || !y || !r || !min_level || !max_level) return mfail(ORBX_E_INVALID, "NULL window array");
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, nq, 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const WindowParts w(in, x, y, r, min_level, max_level, nq);
    const int poff = in.reserve((size_t)nq * 4);
    MTRY(in.upload(s));
    MTRY(launch_area_list<0>(m, in, w, nq, m->d_out, nullptr, nullptr, s));
    std::vector<int32_t> cnt(nq);
    MTRY(orbm_d2h(m, cnt.data(), m->d_out, (size_t)nq * 4, s));
    MTRY(orbm_sync(m, s));
    for (int i = 0; i < nq; i++) cand_off[i + 1] = cand_off[i] + cnt[i];
    const int total = cand_off[nq];
    if (total > cap_idx) return mfail(ORBX_E_CAPACITY, "%d candidates, caller capacity %d", total, cap_idx);
    if (total == 0) return 0;
    if (!cand_idx) return mfail(ORBX_E_INVALID, "cand_idx is NULL");
    MTRY(orbm_grow(m, 0, 0, total));
    MTRY(in.fill(poff, cand_off, s));
    MTRY(launch_area_list<1>(m, in, w, nq, nullptr, in.at<int32_t>(poff), m->d_idx, s));
    MTRY(orbm_d2h(m, cand_idx, m->d_idx, (size_t)total * 4, s));
    MTRY(orbm_sync(m, s));
    return total;
}

extern "C" int orbm_search_area_best2_device(orbm_matcher *m, const uint8_t *d_qdesc, const float *d_x, const float *d_y,
                                             const float *d_r, const int32_t *d_min_level, const int32_t *d_max_level, int nq,
                                             const uint8_t *d_train_desc, const uint8_t *d_skip,
                                             int32_t *d_best_idx, int32_t *d_best_d, int32_t *d_second_d, void *hip_stream)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (!m->grid_ok) return mfail(ORBX_E_INVALID, "orbm_grid_build has not been called");
    if (nq <= 0) return nq == 0 ? ORBX_OK : mfail(ORBX_E_INVALID, "nq < 0");
    if (!d_qdesc || !d_x || !d_y || !d_r || !d_min_level || !d_max_level || !d_train_desc || !d_best_idx || !d_best_d || !d_second_d)
        return mfail(ORBX_E_INVALID, "NULL device pointer");
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    hipLaunchKernelGGL(k_search_area, dim3((nq + 3) / 4), dim3(M_THREADS), 0, s, m->grid, d_qdesc, d_x, d_y, d_r, d_min_level,
                       d_max_level, nq, d_train_desc, d_skip, d_best_idx, d_best_d, d_second_d);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_search_area_best2(orbm_matcher *m, const uint8_t *qdesc, const float *x, const float *y, const float *r,
                                      const int32_t *min_level, const int32_t *max_level, int nq,
                                      const uint8_t *train_desc, const uint8_t *skip,
                                      int32_t *best_idx, int32_t *best_d, int32_t *second_d)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (!m->grid_ok) return mfail(ORBX_E_INVALID, "orbm_grid_build has not been called");
    if (nq < 0) return mfail(ORBX_E_INVALID, "nq=%d", nq);
    if (nq == 0) return ORBX_OK;
    MTRY(orbm_grow(m, nq, 0, 0));
    if (!qdesc || !x || !y || !r || !min_level || !max_level || !best_idx || !best_d || !second_d || (m->grid.n > 0 && !train_desc))
        return mfail(ORBX_E_INVALID, "NULL buffer");
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    int32_t *o_bi = m->d_out, *o_bd = m->d_out + nq, *o_sd = m->d_out + 2 * (size_t)nq;
    const size_t nb4 = (size_t)nq * 4, nt = (size_t)m->grid.n;
    InBlock in(m);
    const WindowParts w(in, x, y, r, min_level, max_level, nq);
    const int pq = in.add(qdesc, (size_t)nq * 32), pt = in.add(train_desc, nt * 32), ps = in.add(skip, skip ? nt : 0);
    MTRY(in.upload(s));
    MTRY(orbm_search_area_best2_device(m, in.at<uint8_t>(pq), in.at<float>(w.x), in.at<float>(w.y), in.at<float>(w.r), in.at<int32_t>(w.mn),
                                       in.at<int32_t>(w.mx), nq, nt > 0 ? in.at<uint8_t>(pt) : m->d_t, in.at<uint8_t>(ps), o_bi, o_bd, o_sd, s));
    void *const hosts[3] = {best_idx, best_d, second_d};
    const size_t parts[3] = {nb4, nb4, nb4};
    MTRY(orbm_d2h_split(m, hosts, parts, 3, o_bi, s));
    MTRY(orbm_sync(m, s));
    return ORBX_OK;
}

// GetFeaturesInArea for nq windows AND the distance of every candidate to its window's descriptor, for the matchers whose scan
// is sequential on the host (SearchForInitialization, SearchByProjection(Frame, Frame)): inputs go up in one copy, counts come
// back, offsets go up, lists and distances come back -- two synchronisations.  (One pass into fixed per-window slots was
// measured: the fullest windows need > 128 slots, and copying nq x slots back costs more than the second round trip.)
// The caller has grown the handle to nq queries.  Returns the number of candidates.
int orbm_area_pairs(orbm_matcher *m, const float *x, const float *y, const float *r, const int32_t *mn, const int32_t *mx, int nq,
                    const uint8_t *qdesc, const uint8_t *train_desc, int n_train,
                    std::vector<int32_t> &off, std::vector<int32_t> &idx, std::vector<int32_t> &dist)
{
    off.assign((size_t)nq + 1, 0);
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const WindowParts w(in, x, y, r, mn, mx, nq);
    const int pq = in.add(qdesc, (size_t)nq * 32), pt = in.add(train_desc, (size_t)n_train * 32);
    const int poff = in.reserve(((size_t)nq + 1) * 4);      // filled after the counts are known
    MTRY(in.upload(s));
    MTRY(launch_area_list<0>(m, in, w, nq, m->d_out, nullptr, nullptr, s));
    std::vector<int32_t> cnt((size_t)nq);
    MTRY(orbm_d2h(m, cnt.data(), m->d_out, (size_t)nq * 4, s));
    MTRY(orbm_sync(m, s));
    for (int i = 0; i < nq; i++) off[i + 1] = off[i] + cnt[i];
    const int total = off[nq];
    idx.assign((size_t)std::max(total, 1), 0); dist.assign((size_t)std::max(total, 1), 0);
    if (total == 0) return 0;
    MTRY(orbm_grow(m, 0, 0, total));                 // d_idx / d_out hold nothing yet
    MTRY(in.fill(poff, off.data(), s));
    MTRY(launch_area_list<1>(m, in, w, nq, nullptr, in.at<int32_t>(poff), m->d_idx, s));
    orbm_launch_dist_csr(in.at<uint8_t>(pq), nq, in.at<uint8_t>(pt), in.at<int32_t>(poff), m->d_idx, total, m->d_out, s);
    MHIPCHK(hipGetLastError());
    MTRY(orbm_d2h(m, idx.data(), m->d_idx, (size_t)total * 4, s));
    MTRY(orbm_d2h(m, dist.data(), m->d_out, (size_t)total * 4, s));
    MTRY(orbm_sync(m, s));
    return total;
}

// ---- ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520) ----
extern "C" int orbm_search_for_initialization(orbm_matcher *m, const orbx_keypoint *kps1, const uint8_t *desc1, int n1,
                                              const orbx_keypoint *kps2, const uint8_t *desc2, int n2,
                                              float *prev_matched, int window_size, float nnratio, int check_orientation,
                                              int32_t *matches12, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n1 < 0 || n2 < 0 || !matches12 || !nmatches || (n1 > 0 && (!kps1 || !desc1 || !prev_matched)) || (n2 > 0 && (!kps2 || !desc2)))
        return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;                       // :408
    if (n1 == 0 || n2 == 0) return ORBX_OK;
    if (!m->grid_ok || m->grid.n != n2) return mfail(ORBX_E_INVALID, "orbm_grid_build(frame 2) has not been called (grid holds %d keypoints, n2 = %d)", m->grid_ok ? m->grid.n : -1, n2);
    // the queries: keypoints of frame 1 on level 0 (:421-423), their windows and descriptors
    AreaQueries Q;
    for (int i = 0; i < n1; i++)
        if (kps1[i].octave <= 0) Q.add(i, prev_matched[2 * i], prev_matched[2 * i + 1], (float)window_size, kps1[i].octave, kps1[i].octave);
    const int nq = Q.size();
    if (nq == 0) return ORBX_OK;
    MTRY(Q.run(m, desc1, desc2, n2));
    const std::vector<int32_t> &off = Q.off, &idx = Q.idx, &dist = Q.dist;
    // the sequential scan (:418-487)
    std::vector<int> matched_dist((size_t)n2, INT_MAX), matches21((size_t)n2, -1);
    RotHist rot;                                     // tag = i1
    int nm = 0;
    for (int k = 0; k < nq; k++) {
        const int i1 = Q.src[k];
        if (off[k + 1] == off[k]) continue;          // :427
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int c = off[k]; c < off[k + 1]; c++) {
            const int i2 = idx[c], d = dist[c];
            if (matched_dist[i2] <= d) continue;     // :444
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = i2; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist <= ORBM_TH_LOW && (float)bestDist < (float)bestDist2 * nnratio) {     // :459-461
            if (matches21[bestIdx2] >= 0) { matches12[matches21[bestIdx2]] = -1; nm--; }
            matches12[i1] = bestIdx2;
            matches21[bestIdx2] = i1;
            matched_dist[bestIdx2] = bestDist;
            nm++;
            if (check_orientation) MTRY(rot.add(kps1[i1].angle, kps2[bestIdx2].angle, i1));
        }
    }
    if (check_orientation)                           // :489-510
        rot.cull([&](int i1) { if (matches12[i1] >= 0) { matches12[i1] = -1; nm--; } });
    for (int i1 = 0; i1 < n1; i1++)                  // :513-516
        if (matches12[i1] >= 0) { prev_matched[2 * i1] = kps2[matches12[i1]].x; prev_matched[2 * i1 + 1] = kps2[matches12[i1]].y; }
    *nmatches = nm;
    return ORBX_OK;
}

// ---- ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (src/ORBmatcher.cc:1328-1470) ----
extern "C" int orbm_search_by_projection_last(orbm_matcher *m, int n_last, const uint8_t *has_point, const float *xw, const uint8_t *mp_desc,
                                              const int32_t *mp_obs, const orbx_keypoint *kps_last, const float *Tcw, const float *Tlw,
                                              float fx, float fy, float cx, float cy, float mb, float mbf, const float bounds[4],
                                              const float *scale_factors, int nlevels, const orbx_keypoint *kps_cur, const uint8_t *desc_cur,
                                              const float *u_right, int n_cur, float th, int mono, int check_orientation,
                                              int32_t *cur_obs, int32_t *cur_match, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n_last < 0 || n_cur < 0 || !Tcw || !Tlw || !bounds || !scale_factors || nlevels < 1 || !nmatches ||
        (n_last > 0 && (!has_point || !xw || !mp_desc || !mp_obs || !kps_last)) || (n_cur > 0 && (!kps_cur || !desc_cur || !cur_obs || !cur_match)))
        return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n_cur; i++) cur_match[i] = -1;
    if (n_last == 0 || n_cur == 0) return ORBX_OK;
    if (!m->grid_ok || m->grid.n != n_cur) return mfail(ORBX_E_INVALID, "orbm_grid_build(current frame) has not been called");
    float twc[3];                                   // :1342-1350
    camera_center(Tcw, twc);
    const float tlc2 = gemm_row(Tlw, 2, twc);
    const bool forward = tlc2 > mb && !mono, backward = -tlc2 > mb && !mono;
    // projections (:1352-1394): one window per last-frame feature that survives the checks
    AreaQueries Q;
    std::vector<float> invz;
    for (int i = 0; i < n_last; i++) {
        if (!has_point[i]) continue;
        const float *X = xw + 3 * (size_t)i;
        const float xc = gemm_row(Tcw, 0, X), yc = gemm_row(Tcw, 1, X), zc = gemm_row(Tcw, 2, X);
        const float invzc = (float)(1.0 / zc);
        if (invzc < 0) continue;
        const float u = fx * xc * invzc + cx, v = fy * yc * invzc + cy;
        if (u < bounds[0] || u > bounds[1]) continue;
        if (v < bounds[2] || v > bounds[3]) continue;
        const int oct = kps_last[i].octave;
        if (oct < 0 || oct >= nlevels) return mfail(ORBX_E_INVALID, "last-frame keypoint %d on octave %d of %d", i, oct, nlevels);
        const float radius = th * scale_factors[oct];
        if (forward) Q.add(i, u, v, radius, oct, -1);
        else if (backward) Q.add(i, u, v, radius, 0, oct);
        else Q.add(i, u, v, radius, oct - 1, oct + 1);
        invz.push_back(invzc);
    }
    const int nq = Q.size();
    if (nq == 0) return ORBX_OK;
    MTRY(Q.run(m, mp_desc, desc_cur, n_cur));
    const std::vector<int32_t> &off = Q.off, &idx = Q.idx, &dist = Q.dist;
    // the sequential scan (:1396-1444)
    RotHist rot;                                     // tag = the current frame's feature
    int nm = 0;
    for (int k = 0; k < nq; k++) {
        if (off[k + 1] == off[k]) continue;
        const int iLast = Q.src[k];
        int bestDist = 256, bestIdx2 = -1;
        for (int c = off[k]; c < off[k + 1]; c++) {
            const int i2 = idx[c];
            if (cur_obs[i2] > 0) continue;
            if (u_right && u_right[i2] > 0) {
                const float ur = Q.x[k] - mbf * invz[k];
                const float er = fabsf(ur - u_right[i2]);
                if (er > Q.r[k]) continue;
            }
            const int d = dist[c];
            if (d < bestDist) { bestDist = d; bestIdx2 = i2; }
        }
        if (bestDist <= ORBM_TH_HIGH) {
            cur_obs[bestIdx2] = mp_obs[iLast];
            cur_match[bestIdx2] = iLast;
            nm++;
            if (check_orientation) MTRY(rot.add(kps_last[iLast].angle, kps_cur[bestIdx2].angle, bestIdx2));
        }
    }
    if (check_orientation)                           // :1447-1466
        rot.cull([&](int i2) { cur_obs[i2] = -1; cur_match[i2] = -1; nm--; });
    *nmatches = nm;
    return ORBX_OK;
}

// ---- ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
// (src/ORBmatcher.cc:1472-1599), in three pieces so that a caller holding real MapPoint objects can keep calling its own
// MapPoint::PredictScale between the projection and the search (mfMaxDistance is not reachable from outside the class) ----
extern "C" int orbm_project_points(const float *Tcw, float fx, float fy, float cx, float cy, const float bounds[4],
                                   const float *xw, int n, float *u, float *v, float *invzc, float *dist3d, uint8_t *in_image)
{
    if (!Tcw || !bounds || n < 0 || (n > 0 && (!xw || !u || !v || !in_image))) return mfail(ORBX_E_INVALID, "bad argument");
    float Ow[3];                                    // Ow = -Rcw^T tcw (:1478)
    camera_center(Tcw, Ow);
    for (int i = 0; i < n; i++) {
        const float *X = xw + 3 * (size_t)i;
        const float xc = gemm_row(Tcw, 0, X), yc = gemm_row(Tcw, 1, X), zc = gemm_row(Tcw, 2, X);   // :1498
        const float iz = (float)(1.0 / zc);                                                            // :1502
        u[i] = fx * xc * iz + cx; v[i] = fy * yc * iz + cy;                                            // :1504-1505
        in_image[i] = !(u[i] < bounds[0] || u[i] > bounds[1] || v[i] < bounds[2] || v[i] > bounds[3]); // :1507-1510
        if (invzc) invzc[i] = iz;
        if (dist3d) {                               // cv::norm(x3Dw - Ow) (:1513-1514): float difference, double accumulation
            double nn = 0;
            for (int k = 0; k < 3; k++) { const float po = X[k] - Ow[k]; nn += (double)po * (double)po; }
            dist3d[i] = (float)sqrt(nn);
        }
    }
    return ORBX_OK;
}

extern "C" int orbm_predict_scale(float mf_max_distance, float current_dist, float log_scale_factor, int n_levels)
{
    const float ratio = mf_max_distance / current_dist;                // src/MapPoint.cc:407
    int nScale = (int)ceilf(logf(ratio) / log_scale_factor);          // :410 (log of a float: logf)
    if (nScale < 0) nScale = 0;
    else if (nScale >= n_levels) nScale = n_levels - 1;
    return nScale;
}

extern "C" int orbm_search_by_projection_kf(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v,
                                            const int32_t *pred_level, const uint8_t *mp_desc, const float *kf_angle,
                                            const float *scale_factors, int nlevels, const orbx_keypoint *kps_cur, const uint8_t *desc_cur,
                                            int n_cur, float th, int orb_dist, int check_orientation,
                                            uint8_t *cur_has_point, int32_t *cur_match, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n_mp < 0 || n_cur < 0 || !scale_factors || nlevels < 1 || !nmatches ||
        (n_mp > 0 && (!use || !proj_u || !proj_v || !pred_level || !mp_desc || (check_orientation && !kf_angle))) ||
        (n_cur > 0 && (!kps_cur || !desc_cur || !cur_has_point || !cur_match)))
        return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n_cur; i++) cur_match[i] = -1;
    if (n_mp == 0 || n_cur == 0) return ORBX_OK;
    if (!m->grid_ok || m->grid.n != n_cur) return mfail(ORBX_E_INVALID, "orbm_grid_build(current frame) has not been called");
    AreaQueries Q;
    for (int i = 0; i < n_mp; i++) {
        if (!use[i]) continue;
        const int lv = pred_level[i];
        if (lv < 0 || lv >= nlevels) return mfail(ORBX_E_INVALID, "MapPoint %d predicted on level %d of %d", i, lv, nlevels);
        Q.add(i, proj_u[i], proj_v[i], th * scale_factors[lv], lv - 1, lv + 1);       // :1526, :1528
    }
    const int nq = Q.size();
    if (nq == 0) return ORBX_OK;
    MTRY(Q.run(m, mp_desc, desc_cur, n_cur));
    const std::vector<int32_t> &off = Q.off, &idx = Q.idx, &dist = Q.dist;
    // the sequential scan (:1538-1575): an assignment blocks the slot for every later MapPoint
    RotHist rot;                                     // tag = the current frame's feature
    int nm = 0;
    for (int k = 0; k < nq; k++) {
        if (off[k + 1] == off[k]) continue;
        int bestDist = 256, bestIdx2 = -1;
        for (int c = off[k]; c < off[k + 1]; c++) {
            const int i2 = idx[c];
            if (cur_has_point[i2]) continue;
            const int d = dist[c];
            if (d < bestDist) { bestDist = d; bestIdx2 = i2; }
        }
        if (bestDist <= orb_dist && bestIdx2 >= 0) {
            cur_has_point[bestIdx2] = 1;
            cur_match[bestIdx2] = Q.src[k];
            nm++;
            if (check_orientation) MTRY(rot.add(kf_angle[Q.src[k]], kps_cur[bestIdx2].angle, bestIdx2));
        }
    }
    if (check_orientation)                           // :1577-1596
        rot.cull([&](int i2) { cur_has_point[i2] = 0; cur_match[i2] = -1; nm--; });
    *nmatches = nm;
    return ORBX_OK;
}

// The scan of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:73-122) over the windows'
// candidates and distances: query k belongs to MapPoint src[k], has radius r[k] and the candidates idx / dist[off[k] .. off[k + 1]).
// Returns the number of assignments.
static int map_scan(int nq, const int *src, const float *r, const int32_t *off, const int32_t *idx, const int32_t *dist, const float *proj_xr,
                    const float *u_right, const orbx_keypoint *kps_cur, const int32_t *mp_obs, float nnratio, int32_t *cur_obs,
                    int32_t *cur_match)
{
    int nm = 0;
    for (int k = 0; k < nq; k++) {
        if (off[k + 1] == off[k]) continue;
        const int iMP = src[k];
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (int c = off[k]; c < off[k + 1]; c++) {
            const int i2 = idx[c];
            if (cur_obs[i2] > 0) continue;
            if (u_right && u_right[i2] > 0) {
                const float er = fabsf(proj_xr[iMP] - u_right[i2]);
                if (er > r[k]) continue;
            }
            const int d = dist[c];
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestLevel2 = bestLevel; bestLevel = kps_cur[i2].octave; bestIdx = i2; }
            else if (d < bestDist2) { bestLevel2 = kps_cur[i2].octave; bestDist2 = d; }
        }
        if (bestDist <= ORBM_TH_HIGH) {
            if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) continue;
            cur_obs[bestIdx] = mp_obs[iMP];
            cur_match[bestIdx] = iMP;
            nm++;
        }
    }
    return nm;
}

// ---- ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:45-125) ----
extern "C" int orbm_search_by_projection_map(orbm_matcher *m, int n_mp, const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                             const float *proj_xr, const int32_t *pred_level, const float *view_cos, const uint8_t *mp_desc,
                                             const int32_t *mp_obs, const float *scale_factors, int nlevels, const orbx_keypoint *kps_cur,
                                             const uint8_t *desc_cur, const float *u_right, int n_cur, float th, float nnratio,
                                             int32_t *cur_obs, int32_t *cur_match, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n_mp < 0 || n_cur < 0 || !scale_factors || nlevels < 1 || !nmatches || (u_right && !proj_xr) ||
        (n_mp > 0 && (!in_view || !proj_x || !proj_y || !pred_level || !view_cos || !mp_desc || !mp_obs)) ||
        (n_cur > 0 && (!kps_cur || !desc_cur || !cur_obs || !cur_match)))
        return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n_cur; i++) cur_match[i] = -1;
    if (n_mp == 0 || n_cur == 0) return ORBX_OK;
    if (!m->grid_ok || m->grid.n != n_cur) return mfail(ORBX_E_INVALID, "orbm_grid_build(frame) has not been called");
    const bool bFactor = th != 1.0;
    AreaQueries Q;
    for (int i = 0; i < n_mp; i++) {
        if (!in_view[i]) continue;
        const int lv = pred_level[i];
        if (lv < 0 || lv >= nlevels) return mfail(ORBX_E_INVALID, "MapPoint %d predicted on level %d of %d", i, lv, nlevels);
        float rr = view_cos[i] > 0.998 ? 2.5f : 4.0f;         // RadiusByViewingCos
        if (bFactor) rr *= th;
        Q.add(i, proj_x[i], proj_y[i], rr * scale_factors[lv], lv - 1, lv);
    }
    const int nq = Q.size();
    if (nq == 0) return ORBX_OK;
    MTRY(Q.run(m, mp_desc, desc_cur, n_cur));
    *nmatches = map_scan(nq, Q.src.data(), Q.r.data(), Q.off.data(), Q.idx.data(), Q.dist.data(), proj_xr, u_right, kps_cur, mp_obs, nnratio,
                         cur_obs, cur_match);
    return ORBX_OK;
}

// ---- Tracking::SearchLocalPoints (src/Tracking.cc:1174-1199): Frame::isInFrustum for every local MapPoint, then the search above
// on the points in view.  k_frustum (orbm_frustum.hip) writes one window per MapPoint into the call's device block, the count pass
// reads them there, and the frustum outputs come back with the counts.  The host then knows the points in view: their descriptors,
// the offsets of all windows (for the list pass) and of the windows in view (for the distances; the candidates of the empty windows
// in between take no room, so both describe the same list) go up in one copy, lists and distances come back. ----
extern "C" int orbm_search_local_points(orbm_matcher *m, const orbm_frame_view *view, int n, const uint8_t *skip, const float *xw,
                                        const float *normal, const float *mf_max, const float *mf_min, float viewing_cos_limit,
                                        const uint8_t *mp_desc, const int32_t *mp_obs, const orbx_keypoint *kps_cur, const uint8_t *desc_cur,
                                        const float *u_right, int n_cur, float th, float nnratio,
                                        uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, int32_t *pred_level, float *view_cos,
                                        int *n_to_match, int32_t *cur_obs, int32_t *cur_match, int *nmatches)
{
    if (n < 0 || n_cur < 0) return mfail(ORBX_E_INVALID, "n=%d MapPoints, n_cur=%d keypoints", n, n_cur);
    if (n > (1 << 27)) return mfail(ORBX_E_CAPACITY, "request beyond 2^27 MapPoints");
    if (n == 0) return ORBX_OK;                     // nothing to project, nToMatch = 0: no search (:1189)
    MTRY(orbm_frustum_check(view, skip, xw, normal, mf_max, mf_min, status, proj_x, proj_y, proj_xr, pred_level, view_cos, n_to_match));
    if (!mp_desc || !mp_obs || !nmatches || (n_cur > 0 && (!kps_cur || !desc_cur || !cur_obs || !cur_match))) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (u_right && !(view->mbf > 0.f)) return mfail(ORBX_E_INVALID, "u_right given, but the frame has mbf=%g", (double)view->mbf);
    if (!m) return orbm_no_handle();
    if (n_cur > 0 && (!m->grid_ok || m->grid.n != n_cur)) return mfail(ORBX_E_INVALID, "orbm_grid_build(frame) has not been called");
    *nmatches = 0;
    for (int i = 0; i < n_cur; i++) cur_match[i] = -1;
    if (n_cur == 0)                                 // a frame without keypoints: every window is empty
        return orbm_frustum(m, view, n, skip, xw, normal, mf_max, mf_min, viewing_cos_limit, status, proj_x, proj_y, proj_xr, pred_level, view_cos, n_to_match);
    MHIPCHK(hipSetDevice(m->device));
    const size_t N = (size_t)n;
    MTRY(orbm_grow(m, (25ll * n) / 12 + 2, 0, 0));  // d_out: the counts and five arrays of n words, then the n status bytes
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pv = in.add(view, sizeof(orbm_frame_view)), ps = in.add(skip, N), px = in.add(xw, N * 12), pn = in.add(normal, N * 12),
              pa = in.add(mf_max, N * 4), pi = in.add(mf_min, N * 4), pt = in.add(desc_cur, (size_t)n_cur * 32);
    in.device_only_from_here();
    const WindowParts w(in, n);
    const size_t off_bytes = ((N + 1) * 4 + 63) & ~(size_t)63;
    const int p2 = in.reserve(2 * off_bytes + N * 32);      // second trip: off of all windows, off of those in view, their descriptors
    MTRY(in.upload(s));
    int32_t *d_counts = m->d_out;
    float *o = reinterpret_cast<float *>(m->d_out + N);
    uint8_t *d_status = reinterpret_cast<uint8_t *>(m->d_out + 6 * N);
    const FrustumWindows fw = {th, in.dev_at<float>(w.x), in.dev_at<float>(w.y), in.dev_at<float>(w.r), in.dev_at<int32_t>(w.mn), in.dev_at<int32_t>(w.mx)};
    orbm_frustum_launch(in.at<orbm_frame_view>(pv), n, in.at<uint8_t>(ps), in.at<float>(px), in.at<float>(pn), in.at<float>(pa),
                        in.at<float>(pi), viewing_cos_limit, d_status, o, o + N, o + 2 * N, m->d_out + 4 * N, o + 4 * N, &fw, s);
    MHIPCHK(hipGetLastError());
    MTRY(launch_area_list<0>(m, in, w, n, d_counts, nullptr, nullptr, s));
    std::vector<int32_t> cnt(N);
    void *host[7] = {cnt.data(), proj_x, proj_y, proj_xr, pred_level, view_cos, status};
    const size_t parts[7] = {N * 4, N * 4, N * 4, N * 4, N * 4, N * 4, N};
    MTRY(orbm_d2h_split(m, host, parts, 7, m->d_out, s));
    MTRY(orbm_sync(m, s));
    // the points in view: their windows, in MapPoint order
    int32_t *off_all = reinterpret_cast<int32_t *>(in.host_at(p2)), *off_view = reinterpret_cast<int32_t *>(in.host_at(p2) + off_bytes);
    uint8_t *desc_view = in.host_at(p2) + 2 * off_bytes;
    std::vector<int> src;
    std::vector<float> radius;
    const bool bFactor = th != 1.0;                 // src/ORBmatcher.cc:49
    off_all[0] = 0; off_view[0] = 0;
    for (int i = 0; i < n; i++) {
        off_all[i + 1] = off_all[i] + cnt[i];
        if (status[i] != ORBM_FRUSTUM_IN_VIEW) continue;
        float r = view_cos[i] > 0.998 ? 2.5f : 4.0f;   // RadiusByViewingCos, as k_frustum computed it
        if (bFactor) r *= th;
        radius.push_back(r * view->scale_factors[pred_level[i]]);
        memcpy(desc_view + 32 * src.size(), mp_desc + 32 * (size_t)i, 32);
        src.push_back(i);
        off_view[src.size()] = off_all[i + 1];
    }
    const int nq = (int)src.size(), total = off_all[n];
    *n_to_match = nq;                               // nToMatch, :1185
    if (nq == 0 || total == 0) return ORBX_OK;      // :1189, or no keypoint in any window
    MTRY(orbm_grow(m, 0, 0, total));                // d_idx / d_out hold nothing any more
    MTRY(in.send(p2, 2 * off_bytes + (size_t)nq * 32, s));
    const int32_t *d_off_all = in.dev_at<int32_t>(p2), *d_off_view = reinterpret_cast<const int32_t *>(in.dev_at<uint8_t>(p2) + off_bytes);
    MTRY(launch_area_list<1>(m, in, w, n, nullptr, d_off_all, m->d_idx, s));
    orbm_launch_dist_csr(in.dev_at<uint8_t>(p2) + 2 * off_bytes, nq, in.at<uint8_t>(pt), d_off_view, m->d_idx, total, m->d_out, s);
    MHIPCHK(hipGetLastError());
    std::vector<int32_t> idx((size_t)total), dist((size_t)total);
    MTRY(orbm_d2h(m, idx.data(), m->d_idx, (size_t)total * 4, s));
    MTRY(orbm_d2h(m, dist.data(), m->d_out, (size_t)total * 4, s));
    MTRY(orbm_sync(m, s));
    *nmatches = map_scan(nq, src.data(), radius.data(), off_view, idx.data(), dist.data(), proj_xr, u_right, kps_cur, mp_obs, nnratio, cur_obs, cur_match);
    return ORBX_OK;
}
