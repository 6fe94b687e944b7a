// orbm_newpoints.hip -- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823 of WChen09/My-SLAM) and
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:209-454) for ALL neighbours of a key frame in one call (include/orbm.h):
//   orbm_search_for_triangulation   the search against one second view, with the rotation-histogram cull
//   orbm_create_new_map_points      the search against every second view, then the per-match loop (:288-434) over what the
//                                   searches found, on one snapshot of the key frames
// Both run the same search kernel on the same host preparation (FeatureVector validation and merge, view record, feature packing);
// the one-view call is the batch search with one view record whose base is 0.
//
// Why one snapshot is enough: the matcher of :217 has mbCheckOrientation == false, vbMatched2 is never set,
// and the loop writes only to mpCurrentKeyFrame and to the neighbour whose turn it is, so the search of feature idx1 against view v
// depends on no other feature and on no other view.  The one coupling, pKF1->GetMapPoint(idx1) (:699-703), removes rows and changes
// none: the caller replays it on the dense result (host/CreateNewMapPoints.h).
//
// The batch call: one upload (key frame 1 once, the views concatenated), two launches, one download:
//   k_triangulation_views   one wave per query = (view, feature of key frame 1 without a MapPoint in a node the view shares); the
//                           view's parameters come from a device array at a wave-uniform index (scalar loads) and its features
//                           are addressed through the view's offset
//   k_triangulate_queries   one lane per query: tri_lanes() (orbm_tri_body.h, k_triangulate's body) on the match the search left
//                           in device memory; a query without a match gets ORBM_TRI_NO_MATCH
// The results come back per query (match, status, point) and the host scatters them into the dense (view, idx1) outputs in query
// order, which is the visiting order of the reference (a later node's match of the same feature overwrites an earlier one's).
#include "orbm_internal.h"
#include "orbm_tri_body.h"

struct NpView {                             // what SearchForTriangulation reads of one second view, beyond its features
    float F12[9];                           // row-major
    float ex, ey;                           // epipole of camera 1 in the view's image (:664-670)
    int32_t base;                           // the view's first feature in the concatenated arrays
    float thr_epipole[ORBX_MAX_LEVELS];     // 100*pKF2->mvScaleFactors[level]  (int * float -> float, :747)
    double thr_line[ORBX_MAX_LEVELS];       // 3.84*pKF2->mvLevelSigma2[level]  (double * float -> double, :156)
};
#define NP_KEY_NONE 0xFFFFFFFFu

// SearchForTriangulation: one wave per query = a feature of key frame 1 that has no MapPoint yet, against one second view; the lanes
// walk the view's features in the same vocabulary node.  The reference accepts a candidate when `dist <= TH_LOW && dist <= bestDist`
// and both epipolar tests pass (:738-755), and bestDist only moves when a candidate is accepted: the result is the LAST candidate of
// minimal distance among those that pass the stateless tests -> minimum of (distance, -position), the position in 20 bits.
// queries[q]: x = idx1, y / z = [lo, hi) in idx2v (feature indices inside the view), w = bStereo1 | view << 1
__global__ __launch_bounds__(M_THREADS) void k_triangulation_views(const int4 *__restrict__ queries, int nq, const int32_t *__restrict__ idx2v,
                                                                  const uint8_t *__restrict__ desc1, const uint8_t *__restrict__ desc2,
                                                                  const float2 *__restrict__ xy1, const float2 *__restrict__ xy2,
                                                                  const int32_t *__restrict__ oct2, const uint8_t *__restrict__ flags2,
                                                                  const NpView *__restrict__ views, int32_t *__restrict__ match)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (M_THREADS / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int4 rec = queries[q];
    const int idx1 = rec.x, stereo1 = rec.w & 1;
    // the whole wave serves one query: through readfirstlane the view is a scalar for the compiler too, and P's fields are scalar loads
    const NpView *__restrict__ P = views + __builtin_amdgcn_readfirstlane(rec.w >> 1);
    const long long base = P->base;
    const uint4 *Q = reinterpret_cast<const uint4 *>(desc1) + 2 * (long long)idx1;
    const uint4 q0 = Q[0], q1 = Q[1];
    const float2 p1 = xy1[idx1];
    // epipolar line in image 2, l = x1' F12 (:143-145)
    const float a = __fadd_rn(__fadd_rn(__fmul_rn(p1.x, P->F12[0]), __fmul_rn(p1.y, P->F12[3])), P->F12[6]);
    const float b = __fadd_rn(__fadd_rn(__fmul_rn(p1.x, P->F12[1]), __fmul_rn(p1.y, P->F12[4])), P->F12[7]);
    const float c = __fadd_rn(__fadd_rn(__fmul_rn(p1.x, P->F12[2]), __fmul_rn(p1.y, P->F12[5])), P->F12[8]);
    const float den = __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b));
    uint32_t best = NP_KEY_NONE;
    for (int pos = rec.y + lane; pos < rec.z; pos += 64) {
        const long long i2 = base + idx2v[pos];
        const uint8_t f2 = flags2[i2];      // bit 0: eligible (no MapPoint, stereo filter passed :725-732), bit 1: bStereo2
        if (!(f2 & 1)) continue;
        const uint4 *Tj = reinterpret_cast<const uint4 *>(desc2) + 2 * i2;
        const int d = hamming256(q0, q1, Tj[0], Tj[1]);
        if (d > ORBM_TH_LOW) continue;                                           // :738
        const float2 p2 = xy2[i2];
        const int o2 = min(max(oct2[i2], 0), ORBX_MAX_LEVELS - 1);
        if (!stereo1 && !(f2 & 2)) {                                             // :743-749
            const float dx = __fsub_rn(P->ex, p2.x), dy = __fsub_rn(P->ey, p2.y);
            if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < P->thr_epipole[o2]) continue;
        }
        if (den == 0) continue;                                                  // CheckDistEpipolarLine :147-156
        const float num = __fadd_rn(__fadd_rn(__fmul_rn(a, p2.x), __fmul_rn(b, p2.y)), c);
        const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
        if (!((double)dsqr < P->thr_line[o2])) continue;
        const uint32_t key = ((uint32_t)d << 20) | (0xFFFFFu - (uint32_t)min(pos - rec.y, 0xFFFFF));
        best = min(best, key);
    }
    const uint32_t B = wave_min_u32(best);
    if (lane == 0) match[q] = B == NP_KEY_NONE ? -1 : idx2v[rec.y + (int)(0xFFFFFu - (B & 0xFFFFFu))];
}

// One lane per query: tri_lanes() (orbm_tri_body.h) on the match the search left in device memory; a query without one gets
// ORBM_TRI_NO_MATCH.
__global__ __launch_bounds__(TRI_THREADS) void k_triangulate_queries(
    const int4 *__restrict__ queries, const int32_t *__restrict__ match, int nq,
    const orbm_camera *__restrict__ cam1, const orbx_keypoint *__restrict__ kps1, const float2 *__restrict__ keys1,
    const float *__restrict__ ur1, const float *__restrict__ depth1, int n1,
    const orbm_camera *__restrict__ cams2, int nviews, const int32_t *__restrict__ off2, const orbx_keypoint *__restrict__ kps2,
    const float2 *__restrict__ keys2, const float *__restrict__ ur2, const float *__restrict__ depth2,
    uint8_t *__restrict__ status, float *__restrict__ x3d)
{
    tri_lanes(blockIdx.x * TRI_THREADS + threadIdx.x, nq,
              [&](int k, int &idx1, int &idx2, int &v) {
                  const int4 rec = queries[k];
                  idx1 = rec.x; idx2 = match[k]; v = rec.w >> 1;
                  return idx2 >= 0;
              },
              cam1, kps1, keys1, ur1, depth1, n1, cams2, nviews, off2, kps2, keys2, ur2, depth2, status, x3d);
}

// -------------------------------------------------------------------------------------------------
// host side, shared by the two entry points
// -------------------------------------------------------------------------------------------------
// nodes lo .. hi-1 of a FeatureVector: offsets monotone from a non-negative start, node ids ascending, entries off[lo] .. off[hi] of
// idx every one a feature of a key frame with nfeat features
static int np_check_csr(const char *what, const int32_t *node, const int32_t *off, const int32_t *idx, int lo, int hi, int nfeat)
{
    if (hi <= lo) return ORBX_OK;
    if (off[lo] < 0) return mfail(ORBX_E_INVALID, "%s: negative offset at node %d", what, lo);
    for (int a = lo; a < hi; a++) {
        if (off[a + 1] < off[a]) return mfail(ORBX_E_INVALID, "%s: offsets not monotone at node %d", what, a);
        if (a > lo && node[a] <= node[a - 1]) return mfail(ORBX_E_INVALID, "%s: node ids not ascending at node %d", what, a);
    }
    for (int c = off[lo]; c < off[hi]; c++)
        if (idx[c] < 0 || idx[c] >= nfeat) return mfail(ORBX_E_INVALID, "%s: feature index %d outside [0,%d)", what, idx[c], nfeat);
    return ORBX_OK;
}

// what the search derives from a second view's pose and pyramid: the epipole (:664-670) and the per-level thresholds
static NpView np_view(const float *T2w, const float *Cw, float fx2, float fy2, float cx2, float cy2, const float *F12,
                      const float *scale_factors2, const float *level_sigma2_2, int nlevels2, int base)
{
    NpView P;
    const float C2x = gemm_row(T2w, 0, Cw), C2y = gemm_row(T2w, 1, Cw), C2z = gemm_row(T2w, 2, Cw);
    const float invz = 1.0f / C2z;
    P.ex = fx2 * C2x * invz + cx2; P.ey = fy2 * C2y * invz + cy2;
    P.base = base;
    for (int k = 0; k < 9; k++) P.F12[k] = F12[k];
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) {
        P.thr_epipole[l] = l < nlevels2 ? 100 * scale_factors2[l] : 0.f;
        P.thr_line[l] = l < nlevels2 ? 3.84 * level_sigma2_2[l] : 0.0;
    }
    return P;
}

// the queries of one view, appended to qs: the features of key frame 1 in the nodes it shares with nodes [b0, b1) of the second
// FeatureVector that pass :699-709, in visiting order.  Both FeatureVectors have passed np_check_csr.
static void np_queries(std::vector<int4> &qs, int view, const uint8_t *has_mp1, const float *u_right1, const int32_t *fv1_node,
                       const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n, const int32_t *fv2_node, const int32_t *fv2_off,
                       int b0, int b1, int only_stereo)
{
    for (int a = 0, b = b0; a < fv1_n && b < b1;) {
        if (fv1_node[a] == fv2_node[b]) {
            if (fv2_off[b + 1] > fv2_off[b])
                for (int c = fv1_off[a]; c < fv1_off[a + 1]; c++) {
                    const int idx1 = fv1_idx[c];
                    if (has_mp1[idx1]) continue;
                    const int st1 = u_right1[idx1] >= 0;
                    if (only_stereo && !st1) continue;
                    qs.push_back(make_int4(idx1, fv2_off[b], fv2_off[b + 1], st1 | (view << 1)));
                }
            a++; b++;
        } else if (fv1_node[a] < fv2_node[b]) a++;
        else b++;
    }
}

// what k_triangulation_views reads of the features: positions of key frame 1; positions, octaves and flags of the second views
struct NpFeatures {
    std::vector<float> xy1, xy2;
    std::vector<int32_t> oct2;
    std::vector<uint8_t> flags2;            // bit 0: eligible (no MapPoint, stereo filter passed :725-732), bit 1: bStereo2
    NpFeatures(const orbx_keypoint *kps1, int n1, const orbx_keypoint *kps2, const float *u_right2, const uint8_t *has_mp2, int n2, int only_stereo)
        : xy1((size_t)2 * n1), xy2((size_t)2 * n2), oct2((size_t)n2), flags2((size_t)n2)
    {
        for (int i = 0; i < n1; i++) { xy1[2 * (size_t)i] = kps1[i].x; xy1[2 * (size_t)i + 1] = kps1[i].y; }
        for (int i = 0; i < n2; i++) {
            const int st2 = u_right2[i] >= 0;
            flags2[i] = (uint8_t)(((!has_mp2[i] && (!only_stereo || st2)) ? 1 : 0) | (st2 ? 2 : 0));
            xy2[2 * (size_t)i] = kps2[i].x; xy2[2 * (size_t)i + 1] = kps2[i].y; oct2[i] = kps2[i].octave;
        }
    }
};

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
// ORBmatcher::SearchForTriangulation against one second view: the batch call's search with one view record (base 0)
extern "C" int orbm_search_for_triangulation(orbm_matcher *m,
                                             const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const uint8_t *has_mp1, const float *u_right1,
                                             const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                                             const orbx_keypoint *kps2, const uint8_t *desc2, int n2, const uint8_t *has_mp2, const float *u_right2,
                                             const int32_t *fv2_node, const int32_t *fv2_off, const int32_t *fv2_idx, int fv2_n,
                                             const float *Cw, const float *T2w, float fx2, float fy2, float cx2, float cy2, const float *F12,
                                             const float *scale_factors2, const float *level_sigma2_2, int nlevels2, int only_stereo,
                                             int check_orientation, int32_t *matches12, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n1 < 0 || n2 < 0 || fv1_n < 0 || fv2_n < 0 || !matches12 || !nmatches || !Cw || !T2w || !F12 || !scale_factors2 || !level_sigma2_2 ||
        nlevels2 < 1 || nlevels2 > ORBX_MAX_LEVELS)
        return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;                             // :678
    if (n1 == 0 || n2 == 0 || fv1_n == 0 || fv2_n == 0) return ORBX_OK;
    if (!kps1 || !desc1 || !has_mp1 || !u_right1 || !kps2 || !desc2 || !has_mp2 || !u_right2 || !fv1_node || !fv1_off || !fv1_idx || !fv2_node ||
        !fv2_off || !fv2_idx)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(np_check_csr("key frame 1", fv1_node, fv1_off, fv1_idx, 0, fv1_n, n1));
    MTRY(np_check_csr("key frame 2", fv2_node, fv2_off, fv2_idx, 0, fv2_n, n2));
    const NpView view = np_view(T2w, Cw, fx2, fy2, cx2, cy2, F12, scale_factors2, level_sigma2_2, nlevels2, 0);
    std::vector<int4> qs;
    np_queries(qs, 0, has_mp1, u_right1, fv1_node, fv1_off, fv1_idx, fv1_n, fv2_node, fv2_off, 0, fv2_n, only_stereo);
    const int nq = (int)qs.size(), ni2 = fv2_off[fv2_n];
    if (nq == 0) return ORBX_OK;
    const NpFeatures F(kps1, n1, kps2, u_right2, has_mp2, n2, only_stereo);     // octaves are clamped in the kernel, not refused
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, nq, 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pq = in.add(qs.data(), (size_t)nq * 16), pv = in.add(&view, sizeof view), pi = in.add(fv2_idx, (size_t)ni2 * 4);
    const int pd1 = in.add(desc1, (size_t)n1 * 32), pd2 = in.add(desc2, (size_t)n2 * 32), p1 = in.add(F.xy1.data(), (size_t)n1 * 8);
    const int p2 = in.add(F.xy2.data(), (size_t)n2 * 8), po = in.add(F.oct2.data(), (size_t)n2 * 4), pf = in.add(F.flags2.data(), (size_t)n2);
    MTRY(in.upload(s));
    hipLaunchKernelGGL(k_triangulation_views, dim3((nq + 3) / 4), dim3(M_THREADS), 0, s, in.at<int4>(pq), nq, in.at<int32_t>(pi), in.at<uint8_t>(pd1),
                       in.at<uint8_t>(pd2), in.at<float2>(p1), in.at<float2>(p2), in.at<int32_t>(po), in.at<uint8_t>(pf), in.at<NpView>(pv), m->d_out);
    MHIPCHK(hipGetLastError());
    std::vector<int32_t> res((size_t)nq);
    MTRY(orbm_d2h(m, res.data(), m->d_out, (size_t)nq * 4, s));
    MTRY(orbm_sync(m, s));
    // matches, rotation histogram and cull (:758-810) in visiting order
    RotHist rot;                                     // tag = idx1
    int nm = 0;
    for (int k = 0; k < nq; k++) {
        if (res[k] < 0) continue;
        const int idx1 = qs[k].x, idx2 = res[k];
        matches12[idx1] = idx2;
        nm++;
        if (check_orientation) MTRY(rot.add(kps1[idx1].angle, kps2[idx2].angle, idx1));
    }
    if (check_orientation) rot.cull([&](int idx1) { matches12[idx1] = -1; nm--; });
    *nmatches = nm;
    return ORBX_OK;
}

extern "C" int orbm_create_new_map_points(orbm_matcher *m, const orbm_camera *cam1, const orbx_keypoint *kps_un1, const float *keys_xy1,
                                          const float *u_right1, const float *depth1, const uint8_t *desc1, int n1, const uint8_t *has_mp1,
                                          const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                                          const orbm_camera *cams2, const float *F12, int nviews, const int32_t *off2,
                                          const orbx_keypoint *kps_un2, const float *keys_xy2, const float *u_right2, const float *depth2,
                                          const uint8_t *desc2, const uint8_t *has_mp2, const int32_t *fv2_view_off, const int32_t *fv2_node,
                                          const int32_t *fv2_off, const int32_t *fv2_idx, int only_stereo,
                                          int32_t *matches12, uint8_t *status, float *x3d, int32_t *nmatches)
{
    if (n1 < 0 || nviews < 0 || fv1_n < 0) return mfail(ORBX_E_INVALID, "n1=%d nviews=%d fv1_n=%d", n1, nviews, fv1_n);
    if (nviews == 0 || n1 == 0) return ORBX_OK;
    if (nviews > (1 << 20) || (long long)nviews * n1 > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 (view, feature) slots");
    if (!cam1 || !kps_un1 || !keys_xy1 || !u_right1 || !depth1 || !desc1 || !has_mp1 || !cams2 || !F12 || !off2 || !fv2_view_off ||
        !matches12 || !status || !x3d || !nmatches || (fv1_n > 0 && (!fv1_node || !fv1_off || !fv1_idx)))
        return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(orbm_tri_check_views(cam1, cams2, nviews, off2));
    if (fv2_view_off[0] != 0) return mfail(ORBX_E_INVALID, "fv2_view_off[0] must be 0");
    for (int v = 0; v < nviews; v++)
        if (fv2_view_off[v + 1] < fv2_view_off[v]) return mfail(ORBX_E_INVALID, "fv2_view_off not monotone at %d", v);
    const int n2 = off2[nviews], fv2_n = fv2_view_off[nviews];
    if (n2 > 0 && (!kps_un2 || !keys_xy2 || !u_right2 || !depth2 || !desc2 || !has_mp2)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (fv2_n > 0 && (!fv2_node || !fv2_off)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (fv1_n > 0 && fv1_off[0] != 0) return mfail(ORBX_E_INVALID, "fv1_off[0] must be 0");
    if (fv2_n > 0 && fv2_off[0] != 0) return mfail(ORBX_E_INVALID, "fv2_off[0] must be 0");
    for (int a = 0; a < fv2_n; a++)
        if (fv2_off[a + 1] < fv2_off[a]) return mfail(ORBX_E_INVALID, "fv2_off not monotone at node %d", a);
    const int ni2 = fv2_n > 0 ? fv2_off[fv2_n] : 0;
    if (ni2 > 0 && !fv2_idx) return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(np_check_csr("key frame 1", fv1_node, fv1_off, fv1_idx, 0, fv1_n, n1));
    for (int v = 0; v < nviews; v++)
        MTRY(np_check_csr("second view", fv2_node, fv2_off, fv2_idx, fv2_view_off[v], fv2_view_off[v + 1], off2[v + 1] - off2[v]));
    for (int i = 0; i < n1; i++)
        if (kps_un1[i].octave < 0 || kps_un1[i].octave >= cam1->nlevels)
            return mfail(ORBX_E_INVALID, "key frame 1, feature %d: octave %d of %d levels", i, kps_un1[i].octave, cam1->nlevels);
    for (int v = 0; v < nviews; v++)
        for (int i = off2[v]; i < off2[v + 1]; i++)
            if (kps_un2[i].octave < 0 || kps_un2[i].octave >= cams2[v].nlevels)
                return mfail(ORBX_E_INVALID, "second view %d, feature %d: octave %d of %d levels", v, i - off2[v], kps_un2[i].octave, cams2[v].nlevels);

    // the outputs are written once the answer is known (a failed call leaves them as they were): every slot empty, then the pairs
    auto no_pairs = [&]() {
        const size_t slots = (size_t)nviews * n1;
        for (size_t k = 0; k < slots; k++) { matches12[k] = -1; status[k] = ORBM_TRI_NO_MATCH; }
        memset(x3d, 0, slots * 12);
        for (int v = 0; v < nviews; v++) nmatches[v] = 0;
    };

    // per view: its record and its queries
    std::vector<NpView> views((size_t)nviews);
    std::vector<int4> qs;
    for (int v = 0; v < nviews; v++) {
        const orbm_camera &c2 = cams2[v];
        const float T2w[16] = {c2.Rcw[0], c2.Rcw[1], c2.Rcw[2], c2.tcw[0], c2.Rcw[3], c2.Rcw[4], c2.Rcw[5], c2.tcw[1],
                               c2.Rcw[6], c2.Rcw[7], c2.Rcw[8], c2.tcw[2], 0.f, 0.f, 0.f, 1.f};
        views[v] = np_view(T2w, cam1->Ow, c2.fx, c2.fy, c2.cx, c2.cy, F12 + 9 * (size_t)v, c2.scale_factors, c2.level_sigma2, c2.nlevels, off2[v]);
        if (off2[v + 1] == off2[v]) continue;
        np_queries(qs, v, has_mp1, u_right1, fv1_node, fv1_off, fv1_idx, fv1_n, fv2_node, fv2_off, fv2_view_off[v], fv2_view_off[v + 1], only_stereo);
    }
    if (qs.size() > ((size_t)1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 queries");
    const int nq = (int)qs.size();
    if (nq == 0) { no_pairs(); return ORBX_OK; }
    if (!m) return orbm_no_handle();

    const NpFeatures F(kps_un1, n1, kps_un2, u_right2, has_mp2, n2, only_stereo);

    MHIPCHK(hipSetDevice(m->device));
    // d_out holds 3 * max_q ints: per query the point (3 floats), the match (1 int) and the status (1 byte), in this order
    const long long out_ints = (long long)4 * nq + (nq + 3) / 4;
    MTRY(orbm_grow(m, (out_ints + 2) / 3, 0, 0));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const int pq = in.add(qs.data(), (size_t)nq * 16), pv = in.add(views.data(), (size_t)nviews * sizeof(NpView)), pi = in.add(fv2_idx, (size_t)ni2 * 4);
    const int pc1 = in.add(cam1, sizeof(orbm_camera)), pc2 = in.add(cams2, (size_t)nviews * sizeof(orbm_camera)), po = in.add(off2, ((size_t)nviews + 1) * 4);
    const int pd1 = in.add(desc1, (size_t)n1 * 32), px1 = in.add(F.xy1.data(), (size_t)n1 * 8), pk1 = in.add(kps_un1, (size_t)n1 * sizeof(orbx_keypoint));
    const int pr1 = in.add(keys_xy1, (size_t)n1 * 8), pu1 = in.add(u_right1, (size_t)n1 * 4), pz1 = in.add(depth1, (size_t)n1 * 4);
    const int pd2 = in.add(desc2, (size_t)n2 * 32), px2 = in.add(F.xy2.data(), (size_t)n2 * 8), pk2 = in.add(kps_un2, (size_t)n2 * sizeof(orbx_keypoint));
    const int pr2 = in.add(keys_xy2, (size_t)n2 * 8), pu2 = in.add(u_right2, (size_t)n2 * 4), pz2 = in.add(depth2, (size_t)n2 * 4);
    const int pt2 = in.add(F.oct2.data(), (size_t)n2 * 4), pf2 = in.add(F.flags2.data(), (size_t)n2);
    MTRY(in.upload(s));
    float *d_x3d = reinterpret_cast<float *>(m->d_out.get());
    int32_t *d_match = m->d_out + 3 * (size_t)nq;
    uint8_t *d_status = reinterpret_cast<uint8_t *>(m->d_out + 4 * (size_t)nq);
    hipLaunchKernelGGL(k_triangulation_views, dim3((nq + 3) / 4), dim3(M_THREADS), 0, s, in.at<int4>(pq), nq, in.at<int32_t>(pi), in.at<uint8_t>(pd1),
                       in.at<uint8_t>(pd2), in.at<float2>(px1), in.at<float2>(px2), in.at<int32_t>(pt2), in.at<uint8_t>(pf2), in.at<NpView>(pv), d_match);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_triangulate_queries, dim3((nq + TRI_THREADS - 1) / TRI_THREADS), dim3(TRI_THREADS), 0, s, in.at<int4>(pq), d_match, nq,
                       in.at<orbm_camera>(pc1), in.at<orbx_keypoint>(pk1), in.at<float2>(pr1), in.at<float>(pu1), in.at<float>(pz1), n1,
                       in.at<orbm_camera>(pc2), nviews, in.at<int32_t>(po), in.at<orbx_keypoint>(pk2), in.at<float2>(pr2), in.at<float>(pu2),
                       in.at<float>(pz2), d_status, d_x3d);
    MHIPCHK(hipGetLastError());
    std::vector<float> q_x3d((size_t)3 * nq);
    std::vector<int32_t> q_match((size_t)nq);
    std::vector<uint8_t> q_status((size_t)nq);
    void *host[3] = {q_x3d.data(), q_match.data(), q_status.data()};
    const size_t parts[3] = {(size_t)nq * 12, (size_t)nq * 4, (size_t)nq};
    MTRY(orbm_d2h_split(m, host, parts, 3, m->d_out, s));
    MTRY(orbm_sync(m, s));
    no_pairs();
    for (int k = 0; k < nq; k++) {                  // visiting order (:758-760): a later query of the same slot overwrites
        if (q_match[k] < 0) continue;
        const int v = qs[k].w >> 1;
        const size_t slot = (size_t)v * n1 + qs[k].x;
        matches12[slot] = q_match[k];
        status[slot] = q_status[k];
        memcpy(x3d + 3 * slot, &q_x3d[3 * (size_t)k], 12);
        nmatches[v]++;
    }
    return ORBX_OK;
}
