// orbm_kf.hip -- the windowed ORBmatcher methods of the LocalMapping / LoopClosing threads on gfx950.
// Reference (WChen09/My-SLAM), all in src/ORBmatcher.cc:
//   :290-403   SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)      orbm_search_by_projection_sim3
//   :522-655   SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)                   orbm_search_by_bow_kf (orbm_bow.hip, beside its sibling)
//   :657-823   SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bStereo)  orbm_search_for_triangulation (orbm_newpoints.hip)
//   :825-975   Fuse(KeyFrame*, vpMapPoints, th)                                 orbm_fuse
//   :977-1100  Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint)               orbm_fuse_sim3
//   :1102-1326 SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)         orbm_search_by_sim3
// Division of labour, as for the Tracking-thread matchers (orbm_grid.hip): the cv::Mat algebra of a call (a handful of 3x3
// products per MapPoint) runs on the host with OpenCV 3.1.0's arithmetic (orbm_sim3_decompose, orbm_project_points_kf, ...);
// MapPoint::PredictScale stays with the caller's MapPoint; the windows (KeyFrame::GetFeaturesInArea), the per-candidate
// predicates and the Hamming distances run on the GPU.  Three of the window searches carry no state from one MapPoint to the next
// (Fuse x 2, SearchBySim3's two directions), so their selection runs on the GPU too, one wave per query (k_search_kf);
// SearchByProjection(KeyFrame*, Scw, ...) blocks a key-frame slot for every later MapPoint (:375, :396), so its candidate lists and
// distances come back and the reference's scan runs on the host.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbm_window.h"

// -------------------------------------------------------------------------------------------------
// host side: cv::Mat algebra as OpenCV 3.1.0 evaluates it
// -------------------------------------------------------------------------------------------------
// (gemm3 / gemm_row / camera_center: orbm_internal.h)

// Scw -> [Rcw|tcw] (row-major 4x4) and Ow: src/ORBmatcher.cc:299-303 and :986-990.
//   scw = sqrt(sRcw.row(0).dot(sRcw.row(0)))   Mat::dot accumulates in double; the sqrt is a double one, stored in a float
//   Rcw = sRcw/scw, tcw = Scw.col(3)/scw       Mat / s is MatOp_AddEx with alpha = 1./s, materialised by convertTo, whose 32f kernel
//                                              multiplies by (float)alpha in float
//   Ow = -Rcw.t()*tcw
extern "C" int orbm_sim3_decompose(const float *Scw, float *Tcw, float *Ow)
{
    if (!Scw || !Tcw || !Ow) return mfail(ORBX_E_INVALID, "NULL argument");
    double dd = 0;
    for (int k = 0; k < 3; k++) dd += (double)Scw[k] * (double)Scw[k];
    const float scw = (float)sqrt(dd);
    const float inv = (float)(1.0 / (double)scw);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) Tcw[4 * i + j] = Scw[4 * i + j] * inv + 0.0f;
    Tcw[12] = 0.f; Tcw[13] = 0.f; Tcw[14] = 0.f; Tcw[15] = 1.f;
    camera_center(Tcw, Ow);
    return ORBX_OK;
}

// SearchBySim3's :1119-1121: sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (3x3 row-major, 3-vectors)
extern "C" int orbm_sim3_relative(float s12, const float *R12, const float *t12, float *sR12, float *sR21, float *t21)
{
    if (!R12 || !t12 || !sR12 || !sR21 || !t21) return mfail(ORBX_E_INVALID, "NULL argument");
    const float a12 = (float)(double)s12, a21 = (float)(1.0 / (double)s12);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { sR12[3 * i + j] = R12[3 * i + j] * a12 + 0.0f; sR21[3 * i + j] = R12[3 * j + i] * a21 + 0.0f; }
    for (int r = 0; r < 3; r++) t21[r] = gemm3(sR21 + 3 * r, 1, t12, -1.0, 0.f, 0.0);
    return ORBX_OK;
}

// The projection block of :320-355, :852-885, :1008-1043 for n world points: p3Dc = Rcw*p3Dw+tcw, the depth test, u / v, KeyFrame::
// IsInImage (bounds = the key frame's int mnMinX, mnMaxX, mnMinY, mnMaxY as floats; [min, max)), PO = p3Dw - Ow, dist = cv::norm(PO)
// (double accumulation), and with normals the viewing-angle test PO.dot(Pn) < 0.5*dist (Mat::dot: double).  ok[i] = every one of
// those tests passed; the distance-invariance test and PredictScale belong to the caller's MapPoint.  Ow == NULL: -Rcw^T tcw.
extern "C" int orbm_project_points_kf(const float *Tcw, const float *Ow, float fx, float fy, float cx, float cy, const float bounds[4],
                                      const float *xw, const float *normal, int n, float *u, float *v, float *invz, float *dist3d,
                                      uint8_t *ok)
{
    if (!Tcw || !bounds || n < 0 || (n > 0 && (!xw || !u || !v || !dist3d || !ok))) return mfail(ORBX_E_INVALID, "bad argument");
    float ow[3];
    if (Ow) memcpy(ow, Ow, sizeof ow); else camera_center(Tcw, ow);
    for (int i = 0; i < n; i++) {
        const float *X = xw + 3 * (size_t)i;
        const float xc = gemm_row(Tcw, 0, X), yc = gemm_row(Tcw, 1, X), zc = gemm_row(Tcw, 2, X);
        const float iz = 1 / zc;
        const float x = xc * iz, y = yc * iz;
        u[i] = fx * x + cx; v[i] = fy * y + cy;
        bool good = !(zc < 0.0f) && (u[i] >= bounds[0] && u[i] < bounds[1] && v[i] >= bounds[2] && v[i] < bounds[3]);
        float PO[3];
        double nn = 0;
        for (int k = 0; k < 3; k++) { PO[k] = X[k] - ow[k]; nn += (double)PO[k] * (double)PO[k]; }
        const float dist = (float)sqrt(nn);
        if (normal) {
            double dot = 0;
            for (int k = 0; k < 3; k++) dot += (double)PO[k] * (double)normal[3 * (size_t)i + k];
            if (dot < 0.5 * dist) good = false;
        }
        dist3d[i] = dist;
        if (invz) invz[i] = iz;
        ok[i] = good;
    }
    return ORBX_OK;
}

// SearchBySim3's :1158-1179 (and :1238-1259 with the roles swapped): p = sR*(R_A x + t_A) + t, depth, u / v, IsInImage of the other
// key frame, dist3D = cv::norm(p).  `1.0/z` is a double division rounded by the float it initialises.
extern "C" int orbm_project_points_sim3(const float *TAw, const float *sR, const float *t, float fx, float fy, float cx, float cy,
                                        const float boundsB[4], const float *xw, int n, float *u, float *v, float *dist3d, uint8_t *ok)
{
    if (!TAw || !sR || !t || !boundsB || n < 0 || (n > 0 && (!xw || !u || !v || !dist3d || !ok))) return mfail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < n; i++) {
        const float *X = xw + 3 * (size_t)i;
        const float pA[3] = {gemm_row(TAw, 0, X), gemm_row(TAw, 1, X), gemm_row(TAw, 2, X)};
        float pB[3];
        for (int r = 0; r < 3; r++) pB[r] = gemm3(sR + 3 * r, 1, pA, 1.0, t[r], 1.0);
        const float iz = (float)(1.0 / pB[2]);
        const float x = pB[0] * iz, y = pB[1] * iz;
        u[i] = fx * x + cx; v[i] = fy * y + cy;
        double nn = 0;
        for (int k = 0; k < 3; k++) nn += (double)pB[k] * (double)pB[k];
        dist3d[i] = (float)sqrt(nn);
        ok[i] = !(pB[2] < 0.0f) && (u[i] >= boundsB[0] && u[i] < boundsB[1] && v[i] >= boundsB[2] && v[i] < boundsB[3]);
    }
    return ORBX_OK;
}

// -------------------------------------------------------------------------------------------------
// kernels
// -------------------------------------------------------------------------------------------------
struct KfGate {                 // Fuse's reprojection test (:914-938); on = 0 for the variants without one
    int on;
    const float *q_ur;          // per query: ur = u - bf*invz
    const float *t_uright;      // per key-frame feature: mvuRight
    float inv_sigma2[ORBX_MAX_LEVELS];
};

// One wave per projected MapPoint: KeyFrame::GetFeaturesInArea(u, v, radius) in the reference's order, the octave window
// [level - 1, level] (:380, :911, :1067, :1207), Fuse's chi-square gate, the Hamming distance, strict '<' (first candidate wins a tie).
__global__ __launch_bounds__(M_THREADS) void k_search_kf(OrbmGrid g, const uint8_t *__restrict__ qdesc, const float *__restrict__ qx,
                                                        const float *__restrict__ qy, const float *__restrict__ qr,
                                                        const int32_t *__restrict__ qlevel, int nq, const uint8_t *__restrict__ tdesc,
                                                        KfGate gate, int32_t *__restrict__ best_idx, int32_t *__restrict__ best_d)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (M_THREADS / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int lv = qlevel[q];
    const float ur = gate.on ? gate.q_ur[q] : 0.f;
    const uint4 *Q = reinterpret_cast<const uint4 *>(qdesc) + 2 * (long long)q;
    const uint4 q0 = Q[0], q1 = Q[1];
    int bidx;
    // window, octave window, gate, distance and the packed key: kf_window_search (orbm_window.h), shared with k_fuse_views
    const uint32_t bp = kf_window_search(g, x, y, r, lv, gate.on != 0, ur, gate.t_uright, [&](int l) { return gate.inv_sigma2[l]; }, q0, q1,
                                         tdesc, lane, bidx);
    const uint32_t B = wave_min_u32(bp);
    if (B == KF_KEY_NONE) {
        if (lane == 0) { best_idx[q] = -1; best_d[q] = 256; }
    } else if (bp == B) {                       // positions are unique: one lane holds the winner
        best_idx[q] = bidx; best_d[q] = (int)(B >> 22);
    }
}

// the compacted queries of one stateless window search, and its launch
struct KfQueries {
    std::vector<int> src;                   // original MapPoint index
    std::vector<float> x, y, r, ur;
    std::vector<int32_t> level;
    std::vector<uint8_t> desc;
    int build(int n_mp, const uint8_t *use, const float *u, const float *v, const float *proj_ur, const int32_t *pred_level, const uint8_t *mp_desc,
              const float *scale_factors, int nlevels, float th)
    {
        for (int i = 0; i < n_mp; i++) {
            if (!use[i]) continue;
            const int lv = pred_level[i];
            if (lv < 0 || lv >= nlevels) return mfail(ORBX_E_INVALID, "MapPoint %d predicted on level %d of %d", i, lv, nlevels);
            src.push_back(i); x.push_back(u[i]); y.push_back(v[i]); r.push_back(th * scale_factors[lv]); level.push_back(lv);
            if (proj_ur) ur.push_back(proj_ur[i]);
        }
        desc.resize(src.size() * 32);
        for (size_t k = 0; k < src.size(); k++) memcpy(&desc[k * 32], mp_desc + (size_t)src[k] * 32, 32);
        return ORBX_OK;
    }
};

// queues one k_search_kf over grid slot g; results land in d_res[0 .. nq) (indices) and d_res[nq .. 2 nq) (distances)
static int launch_search_kf(orbm_matcher *m, const OrbmGrid &g, const KfQueries &Q, const uint8_t *desc_kf, int n_kf, const float *u_right_kf,
                            const float *inv_level_sigma2, int nlevels, int32_t *d_res, InBlock &in, hipStream_t s)
{
    const int nq = (int)Q.src.size();
    const int px = in.add(Q.x.data(), (size_t)nq * 4), py = in.add(Q.y.data(), (size_t)nq * 4), pr = in.add(Q.r.data(), (size_t)nq * 4);
    const int pl = in.add(Q.level.data(), (size_t)nq * 4), pd = in.add(Q.desc.data(), (size_t)nq * 32), pt = in.add(desc_kf, (size_t)n_kf * 32);
    const bool gated = u_right_kf != nullptr;
    const int pu = gated ? in.add(Q.ur.data(), (size_t)nq * 4) : -1, pk = gated ? in.add(u_right_kf, (size_t)n_kf * 4) : -1;
    MTRY(in.upload(s));
    KfGate gate = {};
    gate.on = gated ? 1 : 0;
    if (gated) {
        gate.q_ur = in.at<float>(pu); gate.t_uright = in.at<float>(pk);
        for (int l = 0; l < ORBX_MAX_LEVELS; l++) gate.inv_sigma2[l] = l < nlevels ? inv_level_sigma2[l] : 0.f;
    }
    hipLaunchKernelGGL(k_search_kf, dim3((nq + 3) / 4), dim3(M_THREADS), 0, s, g, in.at<uint8_t>(pd), in.at<float>(px), in.at<float>(py),
                       in.at<float>(pr), in.at<int32_t>(pl), nq, in.at<uint8_t>(pt), gate, d_res, d_res + nq);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

static int check_kf_args(orbm_matcher *m, int n_mp, const uint8_t *use, const float *u, const float *v, const int32_t *lvl, const uint8_t *desc,
                         const float *sf, int nlevels, const orbx_keypoint *kps_kf, const uint8_t *desc_kf, int n_kf)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n_mp < 0 || n_kf < 0 || !sf || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || (n_mp > 0 && (!use || !u || !v || !lvl || !desc)) ||
        (n_kf > 0 && (!kps_kf || !desc_kf)))
        return mfail(ORBX_E_INVALID, "bad argument");
    return ORBX_OK;
}

// Fuse's search (:889-952) and Fuse(Scw)'s (:1048-1082) for every usable MapPoint: best_idx[i] = the key-frame feature with the
// smallest distance in the window / octave window (/ chi-square gate), if that distance is <= max_dist, else -1.
static int stateless_search(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v, const float *proj_ur,
                            const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, const float *inv_level_sigma2,
                            int nlevels, const float *u_right_kf, const uint8_t *desc_kf, int n_kf, float th, int max_dist,
                            int32_t *best_idx, int *count)
{
    *count = 0;
    for (int i = 0; i < n_mp; i++) best_idx[i] = -1;
    if (n_mp == 0 || n_kf == 0) return ORBX_OK;
    if (!m->grid_ok || m->grid.n != n_kf) return mfail(ORBX_E_INVALID, "orbm_grid_build_kf(key frame) has not been called");
    KfQueries Q;
    MTRY(Q.build(n_mp, use, proj_u, proj_v, proj_ur, pred_level, mp_desc, scale_factors, nlevels, th));
    const int nq = (int)Q.src.size();
    if (nq == 0) return ORBX_OK;
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, nq, 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    MTRY(launch_search_kf(m, m->grid, Q, desc_kf, n_kf, proj_ur ? u_right_kf : nullptr, inv_level_sigma2, nlevels, m->d_out, in, s));
    std::vector<int32_t> res((size_t)2 * nq);
    MTRY(orbm_d2h(m, res.data(), m->d_out, (size_t)2 * nq * 4, s));
    MTRY(orbm_sync(m, s));
    int cnt = 0;
    for (int k = 0; k < nq; k++)
        if (res[k] >= 0 && res[(size_t)nq + k] <= max_dist) { best_idx[Q.src[k]] = res[k]; cnt++; }
    *count = cnt;
    return ORBX_OK;
}

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
extern "C" int orbm_fuse(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v, const float *proj_ur,
                         const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, const float *inv_level_sigma2,
                         int nlevels, const orbx_keypoint *kps_kf, const float *u_right_kf, const uint8_t *desc_kf, int n_kf, float th,
                         int32_t *best_idx, int *nfused)
{
    MTRY(check_kf_args(m, n_mp, use, proj_u, proj_v, pred_level, mp_desc, scale_factors, nlevels, kps_kf, desc_kf, n_kf));
    if (!best_idx || !nfused || !inv_level_sigma2 || (n_mp > 0 && !proj_ur) || (n_kf > 0 && !u_right_kf)) return mfail(ORBX_E_INVALID, "bad argument");
    return stateless_search(m, n_mp, use, proj_u, proj_v, proj_ur, pred_level, mp_desc, scale_factors, inv_level_sigma2, nlevels, u_right_kf,
                            desc_kf, n_kf, th, ORBM_TH_LOW, best_idx, nfused);
}

extern "C" int orbm_fuse_sim3(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v,
                              const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, int nlevels,
                              const orbx_keypoint *kps_kf, const uint8_t *desc_kf, int n_kf, float th, int32_t *best_idx, int *nfused)
{
    MTRY(check_kf_args(m, n_mp, use, proj_u, proj_v, pred_level, mp_desc, scale_factors, nlevels, kps_kf, desc_kf, n_kf));
    if (!best_idx || !nfused) return mfail(ORBX_E_INVALID, "bad argument");
    return stateless_search(m, n_mp, use, proj_u, proj_v, nullptr, pred_level, mp_desc, scale_factors, nullptr, nlevels, nullptr,
                            desc_kf, n_kf, th, ORBM_TH_LOW, best_idx, nfused);
}

extern "C" int orbm_search_by_projection_sim3(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v,
                                              const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, int nlevels,
                                              const orbx_keypoint *kps_kf, const uint8_t *desc_kf, int n_kf, int th,
                                              uint8_t *kf_matched, int32_t *kf_match, int *nmatches)
{
    MTRY(check_kf_args(m, n_mp, use, proj_u, proj_v, pred_level, mp_desc, scale_factors, nlevels, kps_kf, desc_kf, n_kf));
    if (!nmatches || (n_kf > 0 && (!kf_matched || !kf_match))) return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n_kf; i++) kf_match[i] = -1;
    if (n_mp == 0 || n_kf == 0) return ORBX_OK;
    if (!m->grid_ok || m->grid.n != n_kf) return mfail(ORBX_E_INVALID, "orbm_grid_build_kf(key frame) has not been called");
    AreaQueries Q;
    for (int i = 0; i < n_mp; i++) {
        if (!use[i]) continue;
        const int lv = pred_level[i];
        if (lv < 0 || lv >= nlevels) return mfail(ORBX_E_INVALID, "MapPoint %d predicted on level %d of %d", i, lv, nlevels);
        // the octave test of :380 drops candidates without any other effect, so it rides in the window query: with (lv - 1, lv) the
        // level branch of GetFeaturesInArea's Frame twin is `octave < lv - 1 || octave > lv` for every lv >= 0
        Q.add(i, proj_u[i], proj_v[i], th * scale_factors[lv], lv - 1, lv);          // :360
    }
    const int nq = Q.size();
    if (nq == 0) return ORBX_OK;
    MTRY(Q.run(m, mp_desc, desc_kf, n_kf));
    const std::vector<int32_t> &off = Q.off, &idx = Q.idx, &dist = Q.dist;
    int nm = 0;
    for (int k = 0; k < nq; k++) {                  // the sequential scan (:370-398): a match blocks its slot for every later MapPoint
        int bestDist = 256, bestIdx = -1;
        for (int c = off[k]; c < off[k + 1]; c++) {
            const int i2 = idx[c];
            if (kf_matched[i2]) continue;           // :375
            const int d = dist[c];
            if (d < bestDist) { bestDist = d; bestIdx = i2; }
        }
        if (bestDist <= ORBM_TH_LOW) { kf_matched[bestIdx] = 1; kf_match[bestIdx] = Q.src[k]; nm++; }
    }
    *nmatches = nm;
    return ORBX_OK;
}

extern "C" int orbm_search_by_sim3(orbm_matcher *m,
                                   int n_mp1, const uint8_t *use1, const float *proj_u1, const float *proj_v1, const int32_t *pred_level1,
                                   const uint8_t *mp_desc1,
                                   int n_mp2, const uint8_t *use2, const float *proj_u2, const float *proj_v2, const int32_t *pred_level2,
                                   const uint8_t *mp_desc2,
                                   const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbm_kf_grid *grid1, const float *scale_factors1,
                                   int nlevels1,
                                   const orbx_keypoint *kps2, const uint8_t *desc2, int n2, const orbm_kf_grid *grid2, const float *scale_factors2,
                                   int nlevels2, float th, int32_t *match12, int *nfound)
{
    MTRY(check_kf_args(m, n_mp1, use1, proj_u1, proj_v1, pred_level1, mp_desc1, scale_factors2, nlevels2, kps2, desc2, n2));
    MTRY(check_kf_args(m, n_mp2, use2, proj_u2, proj_v2, pred_level2, mp_desc2, scale_factors1, nlevels1, kps1, desc1, n1));
    if (!grid1 || !grid2 || !nfound || (n_mp1 > 0 && !match12)) return mfail(ORBX_E_INVALID, "bad argument");
    if (n_mp1 != n1 || n_mp2 != n2) return mfail(ORBX_E_INVALID, "one MapPoint slot per key-frame feature: n_mp1 = %d / n1 = %d, n_mp2 = %d / n2 = %d", n_mp1, n1, n_mp2, n2);
    *nfound = 0;
    for (int i = 0; i < n_mp1; i++) match12[i] = -1;
    // from here on the call leaves either both grids built (slot 1 = key frame 1) or no grid at all: an early return must not leave
    // the grid of an earlier call behind, which a caller that relabels the slot by its keypoint count would take for key frame 1's
    m->grid_ok = false; m->grid2_ok = false;
    if (n1 == 0 || n2 == 0) return ORBX_OK;
    KfQueries Q1, Q2;                                // Q1: MapPoints of key frame 1 searched in key frame 2 (:1148-1225); Q2: the reverse (:1228-1305)
    MTRY(Q1.build(n_mp1, use1, proj_u1, proj_v1, nullptr, pred_level1, mp_desc1, scale_factors2, nlevels2, th));
    MTRY(Q2.build(n_mp2, use2, proj_u2, proj_v2, nullptr, pred_level2, mp_desc2, scale_factors1, nlevels1, th));
    const int nq1 = (int)Q1.src.size(), nq2 = (int)Q2.src.size();
    if (nq1 == 0 || nq2 == 0) return ORBX_OK;       // a match needs both directions
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, 2 * std::max(nq1, nq2), std::max(n1, n2), 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    // both grids, then both searches, one synchronisation: key frame 1 -> slot `grid`, key frame 2 -> slot `grid2`
    MTRY(orbm_grid_build_into(m, 0, kps1, n1, grid1->assign_min_x, grid1->assign_min_y, grid1->inv_w, grid1->inv_h, grid1->query_min_x, grid1->query_min_y));
    MTRY(orbm_grid_build_into(m, 1, kps2, n2, grid2->assign_min_x, grid2->assign_min_y, grid2->inv_w, grid2->inv_h, grid2->query_min_x, grid2->query_min_y));
    // the grid builder's keypoint staging in d_out is consumed by its kernel before the searches run (same stream), so d_out is free
    // again: the two searches share it
    InBlock in1(m), in2(m);
    int32_t *d_r1 = m->d_out, *d_r2 = m->d_out + 2 * (size_t)nq1;
    MTRY(launch_search_kf(m, m->grid2, Q1, desc2, n2, nullptr, nullptr, nlevels2, d_r1, in1, s));
    MTRY(launch_search_kf(m, m->grid, Q2, desc1, n1, nullptr, nullptr, nlevels1, d_r2, in2, s));
    std::vector<int32_t> res((size_t)2 * (nq1 + nq2));
    MTRY(orbm_d2h(m, res.data(), m->d_out, res.size() * 4, s));
    MTRY(orbm_sync(m, s));
    m->grid_ok = true; m->grid2_ok = true;          // the handle's grid is key frame 1's now
    std::vector<int32_t> vnMatch1((size_t)n1, -1), vnMatch2((size_t)n2, -1);
    for (int k = 0; k < nq1; k++)
        if (res[k] >= 0 && res[(size_t)nq1 + k] <= ORBM_TH_HIGH) vnMatch1[Q1.src[k]] = res[k];                               // :1221
    const int32_t *r2 = res.data() + 2 * (size_t)nq1;
    for (int k = 0; k < nq2; k++)
        if (r2[k] >= 0 && r2[(size_t)nq2 + k] <= ORBM_TH_HIGH) vnMatch2[Q2.src[k]] = r2[k];                                  // :1301
    int nf = 0;
    for (int i1 = 0; i1 < n1; i1++) {               // Check agreement :1310-1323
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0 && vnMatch2[idx2] == i1) { match12[i1] = idx2; nf++; }
    }
    *nfound = nf;
    return ORBX_OK;
}
