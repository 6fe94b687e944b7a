/*
 * orbm.h -- C ABI of the MI355X-native ORB descriptor matcher primitives (liborbx.so).
 *
 * Drop-in boundary for the Hamming inner loops of the reference's ORB_SLAM2::ORBmatcher
 * (citations relative to WChen09/My-SLAM):
 *   include/ORBmatcher.h:44, src/ORBmatcher.cc:1647-1663   static DescriptorDistance(a, b)
 *   src/ORBmatcher.cc:201-232 (SearchByBoW), :432-471 (SearchForInitialization), :76-125, :370-398,
 *   :1397-1430, :1535-1558 (SearchByProjection), :715-756 (SearchForTriangulation), :901-949,
 *   :1060-1079 (Fuse), :1199-1219, :1279-1299 (SearchBySim3), src/Frame.cc:522-549 (stereo):
 *       every one is "best / second-best DescriptorDistance over a candidate index list".
 *   src/ORBmatcher.cc:1601-1642 ComputeThreeMaxima + the 30-bin rotation histogram (:236-246).
 * The reference has no whole-frame brute-force matcher: dense N x M matching is the
 * degenerate case "one candidate list = every train descriptor".
 *
 * The geometry / MapPoint bookkeeping around these loops stays host C++ in the caller
 * (my-slam_amd/host/ORBmatcher.h shows the adapter); the variants whose skip predicates depend on
 * earlier matches (e.g. :444-445) take the per-candidate distances from orbm_distances() and run
 * their tiny selection loop on the host, so their results stay identical.
 *
 * Descriptors are rows of 32 bytes (cv::Mat N x 32 CV_8U, contiguous).  All functions return 0 or
 * a negative orbx_status (orbx.h); text via orbm_last_error().  A matcher handle owns a HIP stream
 * and staging buffers; handles are independent, one handle is not re-entrant.
 */
#ifndef ORBM_H
#define ORBM_H

#include <stddef.h>
#include <stdint.h>
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBM_TH_HIGH 100      /* src/ORBmatcher.cc:37 */
#define ORBM_TH_LOW 50        /* src/ORBmatcher.cc:38 */
#define ORBM_HISTO_LENGTH 30  /* src/ORBmatcher.cc:39 */

typedef struct orbm_matcher orbm_matcher;

int orbm_create(orbm_matcher **out, int device, int max_queries, int max_train, int max_pairs);
void orbm_destroy(orbm_matcher *m);

/* ORBmatcher::DescriptorDistance for one pair (host popcount; one pair is not GPU work). */
int orbm_distance(const uint8_t a[32], const uint8_t b[32]);

/*
 * best / second-best over candidate lists, on the GPU.  Host buffers.
 *   cand_off[nq+1], cand_idx[cand_off[nq]] : CSR lists of train indices per query, scanned in list
 *   order; cand_off == NULL means dense (each query against train 0..nt-1).
 * Semantics of src/ORBmatcher.cc:201-226: bestDist1 = bestDist2 = 256, bestIdx = -1; strict '<'
 * updates (first candidate wins a tie; a tie with the best becomes the second best).
 */
int orbm_best2(orbm_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
               const int32_t *cand_off, const int32_t *cand_idx,
               int32_t *best_idx, int32_t *best_d, int32_t *second_d);

/* Per-candidate distances dist[cand_off[nq]] (dense: dist[nq*nt], row-major) for the search
 * variants whose skip predicates interleave with the scan. */
int orbm_distances(orbm_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                   const int32_t *cand_off, const int32_t *cand_idx, int32_t *dist);

/*
 * Device-resident, batched, dense: pair b matches d_q[b] (d_nq[b] rows) against d_t[b] (d_nt[b]
 * rows); descriptor blocks are [nbatch][cap][32] as written by orbx_extract_batch_device, counts
 * live on the device.  Outputs [nbatch][cap].  Asynchronous on hip_stream (NULL = handle stream).
 */
int orbm_best2_batch_device(orbm_matcher *m, const uint8_t *d_q, const int32_t *d_nq,
                            const uint8_t *d_t, const int32_t *d_nt, int cap, int nbatch,
                            int32_t *d_best_idx, int32_t *d_best_d, int32_t *d_second_d,
                            void *hip_stream);

/*
 * Same plus the SearchByBoW acceptance (:228-232: best <= th and best < nnratio * second) and the
 * rotation-consistency filter (:236-246, :266-284) using the keypoints' angles.  d_match12[b][i] =
 * train index or -1; d_nmatches[b] = surviving matches.  BASELINE config 3's "match against the
 * previous frame".
 */
int orbm_match_batch_device(orbm_matcher *m, const uint8_t *d_q, const orbx_keypoint *d_kq,
                            const int32_t *d_nq, const uint8_t *d_t, const orbx_keypoint *d_kt,
                            const int32_t *d_nt, int cap, int nbatch, int th, float nnratio,
                            int check_orientation, int32_t *d_match12, int32_t *d_nmatches,
                            void *hip_stream);

/*
 * ---- "next" row N1: the Frame grid behind every windowed search ----
 * src/Frame.cc:230-245 AssignFeaturesToGrid, :382-392 PosInGrid, :327-380 GetFeaturesInArea, and the
 * scan they feed in ORBmatcher::SearchByProjection (src/ORBmatcher.cc:1397-1430) / SearchForInitialization
 * (:425-457).  FRAME_GRID_COLS x FRAME_GRID_ROWS = 64 x 48 (include/Frame.h:37-38).
 *
 * orbm_grid_build   builds the 64x48 cell lists of one frame on the GPU from its undistorted keypoints
 *                   (mvKeysUn; with the shipped calibration k1 = 0 that is mvKeys, src/Frame.cc:406-410).
 *                   Bounds are mnMinX/mnMaxX/mnMinY/mnMaxY (:436-463).  The grid stays in the handle.
 * orbm_features_in_area   GetFeaturesInArea for nq windows in one call: CSR lists in the reference's
 *                   order (cell columns, cell rows, push_back order).  Returns the total count.
 * orbm_search_area_best2  the fused form: window query + best / second-best DescriptorDistance with
 *                   the strict-'<' tie rules; skip[i] != 0 drops train keypoint i (the reference's
 *                   `continue` predicates).  *_device takes device pointers and does not synchronise.
 */
/*
 * ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520), the monocular initialiser's matcher.  Frame 2's grid
 * must be in the handle (orbm_grid_build on F2.mvKeysUn).  For every level-0 keypoint of frame 1 the window
 * GetFeaturesInArea(vbPrevMatched[i1], windowSize, 0, 0) and the candidates' distances come from the GPU (one
 * orbm_features_in_area + one orbm_distances pass over all windows); the scan itself is sequential in the reference
 * (vMatchedDistance / vnMatches21 let a later keypoint steal an earlier one's match, :444, :463-467) and runs on the host
 * on those distances, as do the rotation histogram -- whose bins keep the entries of stolen matches, as the reference's
 * rotHist does -- and the cull (:489-510).  prev_matched (2 * n1 floats) is vbPrevMatched, updated in place (:513-516);
 * matches12[n1] = vnMatches12; *nmatches = the return value.
 */
int orbm_search_for_initialization(orbm_matcher *m, const orbx_keypoint *kps1, const uint8_t *desc1, int n1,
                                   const orbx_keypoint *kps2, const uint8_t *desc2, int n2,
                                   float *prev_matched, int window_size, float nnratio, int check_orientation,
                                   int32_t *matches12, int *nmatches);

/*
 * ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (src/ORBmatcher.cc:1328-1470), the
 * matcher of Tracking::TrackWithMotionModel.  The current frame's grid must be in the handle (orbm_grid_build on its mvKeysUn).
 *   last frame, per feature i:  has_point[i] = pMP && !mvbOutlier[i];  xw = pMP->GetWorldPos();  mp_desc = pMP->GetDescriptor();
 *                               mp_obs[i] = pMP->Observations();  kps_last[i] = octave of mvKeys[i], angle of mvKeysUn[i]
 *   current frame:              Tcw / Tlw = CurrentFrame.mTcw / LastFrame.mTcw (row-major 4x4 float);  bounds = mnMinX, mnMaxX,
 *                               mnMinY, mnMaxY;  scale_factors = mvScaleFactors;  u_right = mvuRight or NULL
 *   cur_obs[i2]   in/out: -1 where mvpMapPoints[i2] is NULL, else that point's Observations() (> 0 keeps its place, :1403-1405)
 *   cur_match[i2] out: the last-frame feature whose MapPoint this call put into mvpMapPoints[i2], or -1
 * The projections (cv::Mat algebra as cv::gemm's small-matrix path evaluates it: float accumulation, alpha / beta in double) run on the host, all windows and
 * all candidate distances in two GPU passes, and the scan on the host: it is sequential in the reference (an assignment
 * blocks or is overwritten by later ones; *nmatches counts assignments, the rotation cull decrements once per histogram
 * entry, exactly as :1428-1429 and :1458-1462 do).
 */
int orbm_search_by_projection_last(orbm_matcher *m, int n_last, const uint8_t *has_point, const float *xw, const uint8_t *mp_desc,
                                   const int32_t *mp_obs, const orbx_keypoint *kps_last, const float *Tcw, const float *Tlw,
                                   float fx, float fy, float cx, float cy, float mb, float mbf, const float bounds[4],
                                   const float *scale_factors, int nlevels, const orbx_keypoint *kps_cur, const uint8_t *desc_cur,
                                   const float *u_right, int n_cur, float th, int mono, int check_orientation,
                                   int32_t *cur_obs, int32_t *cur_match, int *nmatches);

/*
 * ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:45-125), the matcher of
 * Tracking::SearchLocalPoints (every frame, against the local map).  Per MapPoint: in_view = mbTrackInView && !isBad(),
 * proj_x / proj_y / proj_xr = mTrackProjX / Y / XR (proj_xr may be NULL when u_right is), pred_level = mnTrackScaleLevel,
 * view_cos = mTrackViewCos (RadiusByViewingCos :127-133), mp_desc = GetDescriptor(), mp_obs = Observations().  Frame side and
 * the cur_obs / cur_match convention as in orbm_search_by_projection_last (cur_match[i2] = MapPoint index).  Best and
 * second-best with their octaves, TH_HIGH, and the ratio test only when both sit on the same level (:115-118).
 */
int orbm_search_by_projection_map(orbm_matcher *m, int n_mp, const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                  const float *proj_xr, const int32_t *pred_level, const float *view_cos, const uint8_t *mp_desc,
                                  const int32_t *mp_obs, const float *scale_factors, int nlevels, const orbx_keypoint *kps_cur,
                                  const uint8_t *desc_cur, const float *u_right, int n_cur, float th, float nnratio,
                                  int32_t *cur_obs, int32_t *cur_match, int *nmatches);

/*
 * ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1472-1599), the matcher Tracking::Relocalization runs after PnP (src/Tracking.cc:1459, 1473: th = 10,
 * ORBdist = 100, then th = 3, ORBdist = 64).  Three entry points, because the level prediction in the middle belongs to the
 * caller's MapPoint (MapPoint::PredictScale reads the protected mfMaxDistance, src/MapPoint.cc:402-417):
 *   orbm_project_points   (host) :1498-1514 for n world points: x3Dc = Rcw x + tcw, u, v, 1 / zc, the image-bounds test
 *                         (in_image[i], :1507-1510) and dist3D = |x - Ow| -- cv::Mat algebra as cv::gemm's small-matrix path does it
 *                         (float accumulation, alpha / beta in double), cv::norm accumulating in double.  invzc and dist3d may be NULL.
 *   orbm_predict_scale    (host) MapPoint::PredictScale(dist, Frame*) for callers that own mfMaxDistance themselves.
 *   orbm_search_by_projection_kf   the search: per key-frame MapPoint i, use[i] = usable (non-NULL, !isBad(), not in sAlreadyFound,
 *                         in_image, minDistance <= dist3D <= maxDistance :1492-1521), window (proj_u, proj_v, th *
 *                         mvScaleFactors[pred_level], levels pred_level -+ 1 :1526-1528), best distance over the free slots
 *                         (cur_has_point[i2] == 0, :1541-1542), accept at <= orb_dist, rotation histogram with
 *                         kf_angle[i] = pKF->mvKeysUn[i].angle and the ComputeThreeMaxima cull (:1577-1596).  The current frame's
 *                         grid must be in the handle.  cur_has_point in/out; cur_match[i2] = i or -1; *nmatches = return value.
 * Windows and candidate distances on the GPU in two passes, the scan on the host (it is sequential in the reference: an
 * assignment blocks the slot for every later MapPoint).
 *
 * Inputs the reference leaves undefined, for this search and the other projecting ones (SearchByProjection(pKF, Scw, ..), both Fuse,
 * SearchBySim3); the reference pin ("What is pinned for the ORBmatcher") keeps them out of the comparison and
 * its UBSan copy reports exactly this line on them:
 *   - `int nScale = ceil(log(ratio)/mfLogScaleFactor)` (src/MapPoint.cc:393, :410) with a quotient that is NaN or infinite:
 *     mfMaxDistance of 0, inf or NaN behind a passing distance test, mfLogScaleFactor of 0, or a distance of 0.  The last is how a
 *     zero divisor gets there: this search has no depth test (:1502), and a point at the camera centre has zc = +-0, an infinite
 *     invzc, u = fx*0*inf = NaN, which passes both bounds tests (:1507-1510), and dist3D = 0.
 * The single-call entry points make no promise on them either: orbm_project_points keeps the reference's tests (a NaN passes them),
 * orbm_predict_scale makes the same conversion; orbm_frustum and orbm_fuse_views reject such points with a status of their own.
 */
int orbm_project_points(const float *Tcw, float fx, float fy, float cx, float cy, const float bounds[4],
                        const float *xw, int n, float *u, float *v, float *invzc, float *dist3d, uint8_t *in_image);
int orbm_predict_scale(float mf_max_distance, float current_dist, float log_scale_factor, int n_levels);
int orbm_search_by_projection_kf(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v,
                                 const int32_t *pred_level, const uint8_t *mp_desc, const float *kf_angle,
                                 const float *scale_factors, int nlevels, const orbx_keypoint *kps_cur, const uint8_t *desc_cur,
                                 int n_cur, float th, int orb_dist, int check_orientation,
                                 uint8_t *cur_has_point, int32_t *cur_match, int *nmatches);

/*
 * Frame::UndistortKeyPoints (src/Frame.cc:404-434) and Frame::ComputeImageBounds (:436-463): host code, they run once per
 * frame on ~10^3 points between orbx_extract and orbm_grid_build.  dist = mDistCoef (k1, k2, p1, p2[, k3]); ndist = 4 or 5.
 * With dist[0] == 0 both are the identity exactly as in the reference (:406-410, :455-461).  Otherwise the points go
 * through cv::undistortPoints(src, dst, K, dist, noArray(), K) of OpenCV 3.1.0, restated: normalise with K, five fixed-point
 * iterations x <- (x0 - deltaX(x)) * icdist(x) of the Brown model in double, reproject with K, store as float.
 * kps_un may alias kps.  bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY}.
 */
int orbm_undistort_keypoints(const orbx_keypoint *kps, int n, float fx, float fy, float cx, float cy,
                             const float *dist, int ndist, orbx_keypoint *kps_un);
int orbm_image_bounds(int width, int height, float fx, float fy, float cx, float cy, const float *dist, int ndist,
                      float bounds[4]);

int orbm_grid_build(orbm_matcher *m, const orbx_keypoint *kps_un, int n,
                    float min_x, float max_x, float min_y, float max_y);
int orbm_features_in_area(orbm_matcher *m, const float *x, const float *y, const float *r,
                          const int32_t *min_level, const int32_t *max_level, int nq,
                          int32_t *cand_off, int32_t *cand_idx, int cap_idx);
int orbm_search_area_best2(orbm_matcher *m, const uint8_t *qdesc, const float *x, const float *y, const float *r,
                           const int32_t *min_level, const int32_t *max_level, int nq,
                           const uint8_t *train_desc, const uint8_t *skip,
                           int32_t *best_idx, int32_t *best_d, int32_t *second_d);
int orbm_search_area_best2_device(orbm_matcher *m, const uint8_t *d_qdesc, const float *d_x, const float *d_y,
                                  const float *d_r, const int32_t *d_min_level, const int32_t *d_max_level, int nq,
                                  const uint8_t *d_train_desc, const uint8_t *d_skip,
                                  int32_t *d_best_idx, int32_t *d_best_d, int32_t *d_second_d, void *hip_stream);

/*
 * ---- "next" row N2: ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) src/ORBmatcher.cc:159-288 ----
 * The two FeatureVectors come from orbv_feature_vector (ascending node ids, CSR feature lists).  For every node both
 * frames share, every key-frame feature with a usable MapPoint (valid_kf[i] != 0: the reference's `pMP && !pMP->isBad()`)
 * scans the frame's features of that node in list order, skipping the ones an earlier key-frame feature already took
 * (`if(vpMapPointMatches[realIdxF]) continue;` :209) -- so the scan order matters and is kept.  A frame feature lives in
 * exactly one node, hence nodes are independent: one wave per node walks its key-frame features in order with the node's
 * frame features across the lanes (best / second-best :214-226, TH_LOW and ratio :228-232); the rotation histogram
 * (:236-246, :266-284) runs on the host over the match table.  A call in which a shared node has more than 4096 lane-side
 * features (the frame's here, key frame 2's usable ones in orbm_search_by_bow_kf), and every call when ORBM_BOW_HOST_SELECT=1 is
 * in the environment, takes the host selection: all node-mate distances in one GPU call, the same selection scan on the host.
 * match_f[i] = index of the key-frame feature matched to frame feature i, or -1 (the reference's vpMapPointMatches as indices);
 * *nmatches = the function's return value.  kps_kf are the key frame's mvKeysUn, kps_f the frame's mvKeys (only .angle is read).
 *
 * This call and orbm_search_by_bow_kf are the batch calls below with one candidate, and they check their arguments exactly as those
 * do: the same conditions in the same order with the same ORBX_E_INVALID texts, before anything is written and before the handle
 * is looked at, so an argument error leaves match_f / matches12 / *nmatches untouched.  A call with an empty side (n == 0 or
 * fv_n == 0), or without a usable shared node, is answered on the host (-1 / 0) and needs no handle; everything else needs one
 * (a NULL handle: as orbm_create_new_map_points, outputs untouched).  A failure after that (a HIP error) may leave the table partly
 * written.  The calls grow the handle's result buffer when they need to and nothing else: no SearchByBoW call drops the grid.
 */
int orbm_search_by_bow(orbm_matcher *m,
                       const uint8_t *desc_kf, const orbx_keypoint *kps_kf, int n_kf, const uint8_t *valid_kf,
                       const int32_t *fv_kf_node, const int32_t *fv_kf_off, const int32_t *fv_kf_idx, int fv_kf_n,
                       const uint8_t *desc_f, const orbx_keypoint *kps_f, int n_f,
                       const int32_t *fv_f_node, const int32_t *fv_f_off, const int32_t *fv_f_idx, int fv_f_n,
                       float nnratio, int check_orientation, int32_t *match_f, int *nmatches);

/*
 * ---- the LocalMapping / LoopClosing matchers (include/ORBmatcher.h:60, 66, 72, 77, 80, 83) ----
 * Same division of labour as the Tracking-thread matchers above: the cv::Mat algebra of a call runs on the host with OpenCV
 * 3.1.0's arithmetic (3x3 * 3x1 products through cv::gemm's small-matrix path: float accumulation, alpha / beta applied in
 * double; Mat / scalar as a float multiplication by (float)(1./s); Mat::dot and cv::norm accumulating in double), MapPoint::
 * PredictScale(dist, pKF) stays with the caller's MapPoint, and the windows (KeyFrame::GetFeaturesInArea, src/KeyFrame.cc:569-606),
 * the per-candidate predicates and the Hamming distances run on the GPU.  Where the reference's inner loop carries no state from
 * one MapPoint / feature to the next (Fuse x 2, SearchBySim3, SearchForTriangulation) the selection runs on the GPU as well.
 *
 * orbm_reserve       grows the handle's workspace (never shrinks it).  The reference's matcher has no size limit, so every entry
 *                    point grows the handle when its inputs are larger than the handle instead of refusing; reserving up front
 *                    keeps allocation out of the calls.  Growing max_train drops the grid in the handle.
 * orbm_grid_build_kf a KeyFrame's grid: the cells were filled by Frame::PosInGrid with Frame's float mnMinX / mnMinY and grid
 *                    element sizes (assign_*, inv_*: src/KeyFrame.cc:48-54 copies mGrid), while KeyFrame::GetFeaturesInArea
 *                    subtracts the key frame's own int mnMinX / mnMinY (query_*: include/KeyFrame.h:190-193).
 */
typedef struct {
    float assign_min_x, assign_min_y;   /* Frame::mnMinX, Frame::mnMinY */
    float inv_w, inv_h;                 /* pKF->mfGridElementWidthInv, mfGridElementHeightInv */
    float query_min_x, query_min_y;     /* (float)pKF->mnMinX, (float)pKF->mnMinY */
} orbm_kf_grid;
int orbm_reserve(orbm_matcher *m, int max_queries, int max_train, int max_pairs);
int orbm_grid_count(const orbm_matcher *m);     /* keypoints in the handle's grid; -1: none (never built, or dropped by a growth) */
int orbm_grid_build_kf(orbm_matcher *m, const orbx_keypoint *kps_un, int n, float assign_min_x, float assign_min_y,
                       float inv_w, float inv_h, float query_min_x, float query_min_y);

/* (host) Scw -> [Rcw|tcw] as a row-major 4x4 and Ow: src/ORBmatcher.cc:299-303 == :986-990. */
int orbm_sim3_decompose(const float *Scw, float *Tcw, float *Ow);
/* (host) SearchBySim3's src/ORBmatcher.cc:1119-1121: sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (row-major 3x3, 3). */
int orbm_sim3_relative(float s12, const float *R12, const float *t12, float *sR12, float *sR21, float *t21);
/*
 * (host) the projection block of :320-355, :852-885, :1008-1043 for n world points: p3Dc = Rcw*p3Dw+tcw, u, v, 1/z, dist3D =
 * |p3Dw - Ow|.  ok[i] = depth not negative && KeyFrame::IsInImage(u, v) (bounds = the key frame's mnMinX, mnMaxX, mnMinY, mnMaxY;
 * [min, max), src/KeyFrame.cc:608-611) && (normal == NULL || !(PO.dot(Pn) < 0.5*dist3D)).  Ow == NULL: -Rcw^T tcw; Fuse passes
 * pKF->GetCameraCenter().  The distance-invariance test and PredictScale are the caller's (MapPoint getters).  invz may be NULL.
 */
int orbm_project_points_kf(const float *Tcw, const float *Ow, float fx, float fy, float cx, float cy, const float bounds[4],
                           const float *xw, const float *normal, int n, float *u, float *v, float *invz, float *dist3d, uint8_t *ok);
/* (host) SearchBySim3's :1158-1179 / :1238-1259: p = sR*(R_A x + t_A) + t for the MapPoints of key frame A (pose TAw), projected
 * with pKF1's calibration into key frame B; ok[i] = depth not negative && B->IsInImage(u, v); dist3d = |p|. */
int orbm_project_points_sim3(const float *TAw, const float *sR, const float *t, float fx, float fy, float cx, float cy,
                             const float boundsB[4], const float *xw, int n, float *u, float *v, float *dist3d, uint8_t *ok);

/*
 * ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:290-403; LoopClosing.cc:376).
 * Per candidate MapPoint i: use[i] = every `continue` of :317-355 passed (not bad, not in spAlreadyFound, orbm_project_points_kf's
 * ok, minDistance <= dist <= maxDistance), proj_u / proj_v, pred_level = pMP->PredictScale(dist, pKF), mp_desc = GetDescriptor().
 * The key frame's grid must be in the handle (orbm_grid_build_kf).  kf_matched[idx] in/out = (vpMatched[idx] != NULL);
 * kf_match[idx] out = the MapPoint this call stored in vpMatched[idx], or -1; *nmatches = the return value.  Windows and candidate
 * distances on the GPU, the scan on the host: a match blocks its slot for every later MapPoint (:375, :396).
 */
int orbm_search_by_projection_sim3(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v,
                                   const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, int nlevels,
                                   const orbx_keypoint *kps_kf, const uint8_t *desc_kf, int n_kf, int th,
                                   uint8_t *kf_matched, int32_t *kf_match, int *nmatches);

/*
 * ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (src/ORBmatcher.cc:522-655; LoopClosing.cc:266).
 * valid1 / valid2 = `pMP && !pMP->isBad()` per feature; kps = mvKeysUn (angles); FeatureVectors as for orbm_search_by_bow.
 * matches12[idx1] = the feature of KF2 whose MapPoint goes into vpMatches12[idx1], or -1.  Strict `bestDist1 < TH_LOW` (:598).
 */
int orbm_search_by_bow_kf(orbm_matcher *m,
                          const uint8_t *desc1, const orbx_keypoint *kps1, int n1, const uint8_t *valid1,
                          const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                          const uint8_t *desc2, const orbx_keypoint *kps2, int n2, const uint8_t *valid2,
                          const int32_t *fv2_node, const int32_t *fv2_off, const int32_t *fv2_idx, int fv2_n,
                          float nnratio, int check_orientation, int32_t *matches12, int *nmatches);

/*
 * ---- SearchByBoW for ALL candidate key frames in one call (Tracking::Relocalization, src/Tracking.cc:1377-1398;
 * LoopClosing::ComputeSim3, src/LoopClosing.cc:253-281) ----
 * Both callers loop over their candidates with one SearchByBoW each.  The calls do not interact: each writes a table of its own
 * and reads only its own key frame and the shared side (the lost frame, or mpCurrentKF), and the skip of :209 acts inside one call
 * and one vocabulary node.  So all candidates are searched in one call: the shared side goes up once, every (candidate, shared node)
 * pair is one wave of one launch, the tables come back in one copy, and the rotation histogram runs on the host per candidate.  The
 * one-candidate calls are this with nkf == 1: for every candidate c the table and the count are bit for bit what they return.
 *
 * Checked before any device work, refused with ORBX_E_INVALID and every output untouched: negative counts, NULL buffers where the
 * count is positive (the key-frame variant needs `valid` on both sides, as orbm_search_by_bow_kf does), fv_off not monotone from 0,
 * node ids not strictly ascending, a feature index outside [0, n).  Of a side with n == 0 or fv_n == 0 nothing else is read (its
 * candidate, or with an empty shared side every candidate, has 0 matches, as in the one-candidate calls).  nkf == 0 is ORBX_OK and
 * touches nothing.  A call whose shared
 * side is empty (n == 0 or fv_n == 0), or none of whose candidates shares a usable node with it, is answered on the host (-1 / 0)
 * and needs no handle; everything else needs one (a NULL handle: as orbm_create_new_map_points).  A candidate that shares a node of
 * more than 4096 lane-side features (the frame's in the first call, its own usable ones in the second), and every candidate when
 * ORBM_BOW_HOST_SELECT=1 is in the environment, takes the host selection after the launch (distances on the GPU, the scan on the
 * host).  The call grows the handle when the tables, or the host selection's distances, exceed its result buffer, and leaves the
 * grid slots as it found them.  A failed call leaves the outputs as they were.
 */
typedef struct {
    const uint8_t *desc; const orbx_keypoint *kps; int32_t n;   /* 32-byte descriptors, keypoints (only .angle is read) */
    const uint8_t *valid;                                        /* pMP && !pMP->isBad() per feature; NULL = all valid (frame side: ignored) */
    const int32_t *fv_node, *fv_off, *fv_idx; int32_t fv_n;      /* FeatureVector as orbv_feature_vector writes it */
} orbm_bow_side;

/* Relocalization: nkf key frames against one frame.  match_f[c*frame->n + i], nmatches[c]
   == orbm_search_by_bow(kfs[c], frame) for every c. */
int orbm_search_by_bow_batch(orbm_matcher *m, const orbm_bow_side *kfs, int nkf, const orbm_bow_side *frame,
                             float nnratio, int check_orientation, int32_t *match_f, int32_t *nmatches);

/* ComputeSim3: one key frame (kf1) against nkf key frames.  matches12[c*kf1->n + idx1], nmatches[c]
   == orbm_search_by_bow_kf(kf1, kfs2[c]) for every c. */
int orbm_search_by_bow_kf_batch(orbm_matcher *m, const orbm_bow_side *kf1, const orbm_bow_side *kfs2, int nkf,
                                float nnratio, int check_orientation, int32_t *matches12, int32_t *nmatches);

/*
 * ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (src/ORBmatcher.cc:657-823; LocalMapping.cc:270).
 * has_mp = (GetMapPoint(idx) != NULL), u_right = mvuRight, kps = mvKeysUn; Cw = pKF1->GetCameraCenter(), T2w = pKF2's [R2w|t2w]
 * (row-major 4x4), the calibration, scale factors and level sigma^2 of pKF2, F12 row-major 3x3.  matches12[idx1] = idx2 or -1:
 * vMatchedPairs is the list of (i, matches12[i]) with matches12[i] >= 0 in ascending i (:812-820).  Entirely on the GPU (one wave
 * per feature of KF1): this reference never sets vbMatched2, so no feature's search depends on another's; the candidate accepted
 * is the last one of minimal distance among those that pass the epipole and epipolar-line tests (:738-755).
 * Both FeatureVectors are checked as orbm_create_new_map_points checks its own: offsets not monotone, node ids not ascending or a
 * feature index outside [0, n) are refused with ORBX_E_INVALID before anything is queued (matches12 all -1, *nmatches = 0).
 */
int orbm_search_for_triangulation(orbm_matcher *m,
                                  const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const uint8_t *has_mp1, const float *u_right1,
                                  const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                                  const orbx_keypoint *kps2, const uint8_t *desc2, int n2, const uint8_t *has_mp2, const float *u_right2,
                                  const int32_t *fv2_node, const int32_t *fv2_off, const int32_t *fv2_idx, int fv2_n,
                                  const float *Cw, const float *T2w, float fx2, float fy2, float cx2, float cy2, const float *F12,
                                  const float *scale_factors2, const float *level_sigma2_2, int nlevels2, int only_stereo,
                                  int check_orientation, int32_t *matches12, int *nmatches);

/*
 * ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:825-975; LocalMapping.cc:491, 516),
 * the search half (:889-952).  use[i] = every `continue` of :846-885 passed; proj_ur = u - bf*invz (:870); the key frame's grid in
 * the handle.  best_idx[i] = the key-frame feature the point is fused with (window, octave window, chi-square gate :914-938, best
 * distance <= TH_LOW), or -1; *nfused = their number.  What happens to a fused point (:954-970: Replace, or AddObservation +
 * AddMapPoint) is object-graph work and stays with the caller; no MapPoint's search depends on it, so the searches run on the GPU
 * as one launch.  orbm_fuse_sim3 is Fuse(KeyFrame *pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (:977-1100; LoopClosing.cc:600),
 * :1048-1082: the same without the gate.
 */
int orbm_fuse(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v, const float *proj_ur,
              const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, const float *inv_level_sigma2,
              int nlevels, const orbx_keypoint *kps_kf, const float *u_right_kf, const uint8_t *desc_kf, int n_kf, float th,
              int32_t *best_idx, int *nfused);
int orbm_fuse_sim3(orbm_matcher *m, int n_mp, const uint8_t *use, const float *proj_u, const float *proj_v,
                   const int32_t *pred_level, const uint8_t *mp_desc, const float *scale_factors, int nlevels,
                   const orbx_keypoint *kps_kf, const uint8_t *desc_kf, int n_kf, float th, int32_t *best_idx, int *nfused);

/*
 * ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1102-1326; LoopClosing.cc:324), the two
 * searches and the agreement check (:1188-1323).  One MapPoint slot per key-frame feature (n_mp1 == n1, n_mp2 == n2).
 * use1[i] = pMP && !vbAlreadyMatched1[i] && !isBad() && orbm_project_points_sim3's ok && the distance-invariance test (:1152-1183);
 * proj_u1 / proj_v1 = its projection into key frame 2, pred_level1 = PredictScale(dist3D, pKF2); use2 / proj_*2 / pred_level2 the
 * reverse.  Once the arguments are valid the call ends in one of two states: both grids are built and slot 1 of the handle holds key
 * frame 1's (orbm_grid_count() == n1), or the handle holds no grid (orbm_grid_count() == -1).  The second is the state after an
 * empty side (n1 == 0 or n2 == 0), after a side without a usable MapPoint (every use1 or every use2 zero: nothing can match both
 * ways) and after an error; the grid of an earlier call never survives it.  match12[i1] = the feature of KF2 whose MapPoint goes
 * into vpMatches12[i1], or -1; *nfound = the return value.
 */
int orbm_search_by_sim3(orbm_matcher *m,
                        int n_mp1, const uint8_t *use1, const float *proj_u1, const float *proj_v1, const int32_t *pred_level1,
                        const uint8_t *mp_desc1,
                        int n_mp2, const uint8_t *use2, const float *proj_u2, const float *proj_v2, const int32_t *pred_level2,
                        const uint8_t *mp_desc2,
                        const orbx_keypoint *kps1, const uint8_t *desc1, int n1, const orbm_kf_grid *grid1, const float *scale_factors1,
                        int nlevels1,
                        const orbx_keypoint *kps2, const uint8_t *desc2, int n2, const orbm_kf_grid *grid2, const float *scale_factors2,
                        int nlevels2, float th, int32_t *match12, int *nfound);

/*
 * ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) for a batch of MapPoints in one call ----
 * The reference calls the method once per MapPoint, in loops over all MapPoints of a key frame (src/LocalMapping.cc:141-163,
 * :444, :519-532, src/LoopClosing.cc:533, src/Tracking.cc:541, 677, 1124).  Here the batch is a CSR: point p owns the rows
 * off[p] .. off[p+1]-1 of desc (32 bytes each), given in the iteration order of its mObservations with bad key frames left out
 * (:261-267) -- the order is part of the input, ties go to the first row.  Per point, with N rows:
 *   dist[i][j] = DescriptorDistance(row i, row j), dist[i][i] = 0 (:276-285);
 *   median[i]  = element (N-1)/2 (the lower middle for even N) of row i of dist sorted ascending, own 0 included (:292-294);
 *   best[p]    = the first i with the smallest median[i] (:288-301), best_median[p] = that median; both -1 for an empty run
 *                (the reference returns with mDescriptor untouched, :256, :269).
 * mDescriptor = row best[p] of the point is the caller's to store.  best_median may be NULL.  n_points == 0 is ORBX_OK.  There is
 * no limit on N: runs of up to 256 rows are served from LDS, longer ones from global memory, spread over N / 256 workgroups.
 * Argument checks come before any device work (ORBX_E_INVALID: negative count, NULL off / best / desc, off[0] != 0, off not
 * monotone).  A batch whose runs all have N <= 2 needs no arithmetic (best = 0, or -1): it is answered on the host without a launch
 * and without touching the handle, which may then be NULL.  Every other batch needs the GPU: with a NULL handle it fails with
 * ORBX_E_HIP where there is no HIP device ("no CPU path", as orbm_create does) and with ORBX_E_INVALID where there is one.
 * The call keeps its own scratch block in the handle and grows it on demand; the grid and the other buffers of the handle are
 * not touched, whatever the batch size.
 *
 * orbm_distinctive_descriptors_device takes device pointers (d_desc 16-byte aligned) and the two facts the launch plan needs
 * from the host: total_rows = off[n_points] and max_run >= the longest run (classes above max_run are not launched, so a
 * max_run that is too small leaves their points unanswered; a larger one only costs empty launches).  d_off is trusted to be
 * monotone from 0.  Asynchronous on hip_stream (NULL = the handle's stream), nothing is synchronised -- except that the first
 * call with more points than any call before allocates scratch (not possible inside a stream capture: warm up once).
 */
int orbm_distinctive_descriptors(orbm_matcher *m, int n_points, const int32_t *off, const uint8_t *desc,
                                 int32_t *best, int32_t *best_median);
int orbm_distinctive_descriptors_device(orbm_matcher *m, int n_points, const int32_t *d_off, const uint8_t *d_desc,
                                        int total_rows, int max_run, int32_t *d_best, int32_t *d_best_median, void *hip_stream);

/*
 * ---- LocalMapping::CreateNewMapPoints, the per-match loop (src/LocalMapping.cc:288-434) for all matches in one call ----
 * For every pair of vMatchedIndices (:270) the reference checks the parallax of the two rays (:302-318), triangulates linearly
 * (:324-339) or falls back to KeyFrame::UnprojectStereo (:342-348, src/KeyFrame.cc:615-631), and applies the gates: depth signs
 * (:356-362), the chi-square reprojection tests in their mono and stereo forms (:365-415) and scale consistency (:418-433).  No
 * match reads what another writes (:436-451 is the first write), so one lane takes one match.
 *
 * orbm_camera is what the loop reads of a key frame (:219-234, :272-284, :314-316, :365, :392, :428): Rcw = GetRotation() (row-major),
 * tcw = GetTranslation(), Ow = GetCameraCenter(), the calibration, mb, mbf, mfScaleFactor and the per-level tables.  Key frame 1
 * (mpCurrentKeyFrame) has one block; the second views are `ncams2` blocks, and every match names its view, so several neighbours'
 * matches may share a call.  The reference's own caller goes one neighbour at a time: ncams2 = 1.  What the next neighbour's
 * SearchForTriangulation sees of an accepted match is only that pKF1->GetMapPoint(idx1) is no longer NULL, which removes that
 * feature's row from the search; no other feature's match, and nothing in this loop, depends on the previous neighbour
 * (orbm_create_new_map_points below runs all neighbours at once on that ground).
 * The per-feature arrays of the second views are concatenated, view v owning
 * the features off2[v] .. off2[v+1]-1; off2 has ncams2 + 1 entries, off2[0] = 0.
 *   kps_un = mvKeysUn (pt and octave are read), keys_xy = mvKeys[i].pt as 2 floats per feature (UnprojectStereo reads the raw
 *   keys, not mvKeysUn), u_right = mvuRight, depth = mvDepth
 *   matches[3*k .. 3*k+2] = idx1, idx2 (inside its view), view
 *   status[k] = the line that decided match k (orbm_tri_status); x3d[3*k ..] = the new MapPoint's position for the accepted
 *   statuses (<= ORBM_TRI_STEREO2), zeros otherwise.
 * The reference's quirks are kept: `else if(bStereo2)` (:315: the second view's stereo angle is not looked at when the first is
 * stereo), mpCurrentKeyFrame->mbf in the second view's stereo test (:408).  Arithmetic: the reference's float expressions
 * operation by operation, except the 4x4 cv::SVD of :331, whose last bits depend on OpenCV's algorithm:
 * here the right singular vector of the smallest singular value comes from a one-sided Jacobi in fp64 on the float matrix, and
 * x3D = v[0:3] / v[3] is rounded to float once; the `== 0` test of :335 is made on v[3] rounded to float.
 * ORBM_TRI_UNDEFINED: mvuRight >= 0 with mvDepth <= 0 reaching :344 / :348 -- UnprojectStereo returns an empty cv::Mat and :353
 * reads it; the match is rejected.  ORBM_TRI_BAD_INDEX is only ever written by the device-pointer form (below).
 *
 * Argument checks come before any device work (ORBX_E_INVALID: negative counts, NULL buffers, nlevels outside
 * [1, ORBX_MAX_LEVELS], off2 not monotone from 0, an index outside its key frame, a view outside [0, ncams2), a key point's
 * octave outside its camera's levels); n == 0 is ORBX_OK and touches nothing, the handle included.  Every other call needs the
 * GPU: a NULL handle fails with ORBX_E_HIP where there is no HIP device ("no CPU path") and with ORBX_E_INVALID where there is
 * one.  The call runs on the handle's stream through its staging arena (one upload, one launch, one download) and grows the
 * handle when n is larger than its workspace.
 *
 * orbm_triangulate_matches_device: the same on device pointers (the camera blocks and off2 included).  Nothing is uploaded,
 * downloaded or synchronised; asynchronous on hip_stream (NULL = the handle's stream).
 * The host cannot see the indices, so the kernel checks them: a match with an index, view or octave out of range gets
 * ORBM_TRI_BAD_INDEX and reads nothing through it.
 */
typedef enum {
    ORBM_TRI_SVD = 0,            /* accepted, x3D from the linear triangulation (:324-339) */
    ORBM_TRI_STEREO1 = 1,        /* accepted, x3D = mpCurrentKeyFrame->UnprojectStereo(idx1) (:344) */
    ORBM_TRI_STEREO2 = 2,        /* accepted, x3D = pKF2->UnprojectStereo(idx2) (:348) */
    ORBM_TRI_LOW_PARALLAX = 3,   /* :351 */
    ORBM_TRI_W_ZERO = 4,         /* :336 */
    ORBM_TRI_BEHIND1 = 5,        /* :358 */
    ORBM_TRI_BEHIND2 = 6,        /* :362 */
    ORBM_TRI_REPROJ1 = 7,        /* :377 / :388 */
    ORBM_TRI_REPROJ2 = 8,        /* :403 / :414 */
    ORBM_TRI_ZERO_DIST = 9,      /* :425 */
    ORBM_TRI_SCALE = 10,         /* :433 */
    ORBM_TRI_UNDEFINED = 11,     /* undefined in the reference: UnprojectStereo of a feature with mvDepth <= 0 */
    ORBM_TRI_BAD_INDEX = 12,     /* device-pointer form only: index, view or octave out of range */
    ORBM_TRI_NO_MATCH = 255      /* orbm_create_new_map_points only: the slot holds no pair (matches12 < 0) */
} orbm_tri_status;
typedef struct {
    float Rcw[9];                               /* GetRotation(), row-major */
    float tcw[3];                               /* GetTranslation() */
    float Ow[3];                                /* GetCameraCenter() */
    float fx, fy, cx, cy, invfx, invfy;
    float mb, mbf;
    float scale_factor;                         /* mfScaleFactor (:234; read of key frame 1 only) */
    int32_t nlevels;
    float scale_factors[ORBX_MAX_LEVELS];       /* mvScaleFactors */
    float level_sigma2[ORBX_MAX_LEVELS];        /* mvLevelSigma2 */
} orbm_camera;
int orbm_triangulate_matches(orbm_matcher *m, const orbm_camera *cam1, const orbx_keypoint *kps_un1, const float *keys_xy1,
                             const float *u_right1, const float *depth1, int n1,
                             const orbm_camera *cams2, int ncams2, const int32_t *off2, const orbx_keypoint *kps_un2,
                             const float *keys_xy2, const float *u_right2, const float *depth2,
                             const int32_t *matches, int n, uint8_t *status, float *x3d);
int orbm_triangulate_matches_device(orbm_matcher *m, const orbm_camera *d_cam1, const orbx_keypoint *d_kps_un1,
                                    const float *d_keys_xy1, const float *d_u_right1, const float *d_depth1, int n1,
                                    const orbm_camera *d_cams2, int ncams2, const int32_t *d_off2, const orbx_keypoint *d_kps_un2,
                                    const float *d_keys_xy2, const float *d_u_right2, const float *d_depth2,
                                    const int32_t *d_matches, int n, uint8_t *d_status, float *d_x3d, void *hip_stream);

/*
 * ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:209-454): every neighbour's search and triangulation in one call ----
 * The reference's loop (:239-453) makes, per neighbour, one SearchForTriangulation (:270) and one pass over its pairs (:288-434).
 * The matcher of :217 is ORBmatcher(0.6,false), so the rotation histogram never runs; vbMatched2 is never set; and before neighbour
 * k's own turn the loop has written nothing that the search reads of it (:436-451 writes to mpCurrentKeyFrame and to the neighbour
 * whose turn it is).  The result for feature idx1 of key frame 1 against neighbour k therefore depends on idx1, on neighbour k's
 * features and MapPoint slots, on F12 and on the epipole -- on no other feature and no other neighbour -- with one exception:
 * a feature that received a MapPoint from an earlier neighbour is skipped (:699-703), which removes its row and changes no other.
 * So all searches and all triangulations run here on ONE snapshot taken before the loop, and the caller's loop replays the
 * exception on the dense result: at neighbour v's turn it takes the slots (v, idx1) with matches12 >= 0 in ascending idx1 and keeps
 * those whose pKF1->GetMapPoint(idx1) is still NULL (host/CreateNewMapPoints.h does that).
 *
 * Key frame 1: its orbm_camera, kps_un1 / keys_xy1 / u_right1 / depth1 as for orbm_triangulate_matches, desc1 (32 bytes per
 * feature), has_mp1 = (GetMapPoint(idx) != NULL) and its FeatureVector as CSR (fv1_node ascending, fv1_off, fv1_idx, fv1_n nodes).
 * `nviews` second views in the caller's order: cams2[v] (the epipole, 100*mvScaleFactors, 3.84*mvLevelSigma2 and everything the
 * triangulation reads come from it), F12[9*v ..] = ComputeF12(pKF1, pKF2_v) row-major, off2[nviews+1] into the concatenated
 * kps_un2 / keys_xy2 / u_right2 / depth2 / desc2 / has_mp2, and the views' FeatureVectors concatenated: view v owns the nodes
 * fv2_view_off[v] .. fv2_view_off[v+1]-1 of fv2_node / fv2_off (fv2_off has fv2_view_off[nviews] + 1 entries and runs through
 * all views), and the entries of fv2_idx are feature indices inside their view.  only_stereo as for orbm_search_for_triangulation.
 * There is no check_orientation: the histogram cull (src/ORBmatcher.cc:764-810) depends on which features take part in the
 * search, so it does not survive taking rows out afterwards; a caller that wants it keeps the per-neighbour calls.
 *
 * Outputs, one slot per (view, feature of key frame 1), slot = v*n1 + idx1:
 *   matches12[slot] = idx2 inside view v, or -1            = orbm_search_for_triangulation(view v alone, check_orientation = 0)
 *   status[slot]    = orbm_tri_status of the pair, or ORBM_TRI_NO_MATCH where matches12 < 0
 *   x3d[3*slot ..]  = the new MapPoint's position for the accepted statuses, zeros otherwise
 *                                                          = orbm_triangulate_matches on view v's pair list
 *   nmatches[v]     = what orbm_search_for_triangulation returns in *nmatches for view v
 * The candidate taken is the last of minimal distance, positions inside a node are clamped to 20 bits, and :315's `else
 * if(bStereo2)`, :408's mpCurrentKeyFrame->mbf, the fp64 Jacobi and ORBM_TRI_UNDEFINED are orbm_triangulate_matches' (same code).
 *
 * Argument checks come before any device work (ORBX_E_INVALID: negative counts, NULL buffers, off2 / fv2_view_off / fv1_off /
 * fv2_off not monotone from 0, node ids not ascending, a feature index outside its key frame or view, nlevels outside
 * [1, ORBX_MAX_LEVELS], an octave outside its camera's levels -- of every feature, since the pairs are not known beforehand).
 * nviews == 0 or n1 == 0 is ORBX_OK and touches nothing, the handle and the outputs included.  A call in which no feature of key
 * frame 1 is left to search (no shared node, every feature has a MapPoint) is answered on the host; every other call needs the
 * GPU, and a NULL handle behaves as in orbm_triangulate_matches.  The call runs on the handle's stream through its staging arena:
 * one upload (key frame 1 once), the search launch over the queries of all views, the triangulation launch over the same queries
 * (nothing returns to the host in between), one download.  It grows the handle when it is larger than its workspace and leaves the
 * grid slots as it found them (orbm_grid_count() and window searches are unchanged by it).
 */
int orbm_create_new_map_points(orbm_matcher *m, const orbm_camera *cam1, const orbx_keypoint *kps_un1, const float *keys_xy1,
                               const float *u_right1, const float *depth1, const uint8_t *desc1, int n1, const uint8_t *has_mp1,
                               const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                               const orbm_camera *cams2, const float *F12, int nviews, const int32_t *off2,
                               const orbx_keypoint *kps_un2, const float *keys_xy2, const float *u_right2, const float *depth2,
                               const uint8_t *desc2, const uint8_t *has_mp2, const int32_t *fv2_view_off, const int32_t *fv2_node,
                               const int32_t *fv2_off, const int32_t *fv2_idx, int only_stereo,
                               int32_t *matches12, uint8_t *status, float *x3d, int32_t *nmatches);

/*
 * ---- Frame::isInFrustum for all local MapPoints of a frame, and Tracking::SearchLocalPoints in one call ----
 * Tracking::SearchLocalPoints (src/Tracking.cc:1174-1187) calls Frame::isInFrustum (src/Frame.cc:269-325) once per local
 * MapPoint: camera coordinates (:277), the depth sign (:283), the projection against the image bounds (:287-294), the distance
 * against the scale-invariance region (:297-303, MapPoint::GetMin / MaxDistanceInvariance src/MapPoint.cc:373-383), the viewing
 * angle (:306-311) and MapPoint::PredictScale (:314, src/MapPoint.cc:402-417).  No MapPoint reads what another writes, so one lane
 * takes one MapPoint.
 *
 * orbm_frame_view is what the loop reads of the frame: Rcw = mRcw (row-major), tcw = mtcw, Ow = mOw (src/Frame.cc:261-266), the
 * calibration, mbf, bounds = mnMinX, mnMaxX, mnMinY, mnMaxY, log_scale_factor = mfLogScaleFactor, nlevels = mnScaleLevels and
 * scale_factors = mvScaleFactors (read by orbm_search_local_points only).
 *   per MapPoint i:  skip[i] = (pMP->mnLastFrameSeen == mCurrentFrame.mnId || pMP->isBad()) (src/Tracking.cc:1177-1180);
 *                    xw = GetWorldPos(), normal = GetNormal() (3 floats each); mf_max / mf_min = the raw members mfMaxDistance /
 *                    mfMinDistance -- the 1.2f and 0.8f of the two getters are applied here, and PredictScale divides the raw
 *                    mfMaxDistance;  viewing_cos_limit = the second argument of isInFrustum as a float (0.5 at :1182)
 *   status[i]   = the line that decided the point (orbm_frustum_status); mbTrackInView = (status[i] == ORBM_FRUSTUM_IN_VIEW)
 *   proj_x, proj_y, proj_xr, pred_level, view_cos = mTrackProjX, mTrackProjY, mTrackProjXR, mnTrackScaleLevel, mTrackViewCos
 *                 (:318-322) of the points in view, zeros for every other point
 *   *n_to_match = the points in view (nToMatch, :1185); the caller calls IncreaseVisible() on them (:1184)
 * Arithmetic: the reference's float expressions operation by operation: Pc through cv::gemm's small-matrix
 * path, invz = 1.0f/PcZ in float, cv::norm and Mat::dot accumulated in double, viewCos = the double dot product divided by
 * (double)dist and rounded to float once, PredictScale as float division, logf, float division, ceil.  logf is the correctly
 * rounded fp32 logarithm (orbm_predict_scale keeps the host's logf; the two differ only where the quotient is within rounding
 * of an integer).  The reference's quirks are kept: PcZ == +-0 passes :283 (invz is then infinite), a NaN u or v passes both
 * bounds tests, a NaN viewCos passes :310.  ORBM_FRUSTUM_UNDEFINED: the `int nScale = ceil(...)` of src/MapPoint.cc:410 converts
 * a value that is not finite or lies outside int (mfMaxDistance <= 0, a zero or NaN distance, log_scale_factor == 0), which is
 * undefined in C++; the point is rejected.
 *
 * Argument checks come before any device work (ORBX_E_INVALID: a negative count, NULL buffers, nlevels outside
 * [1, ORBX_MAX_LEVELS], u_right without mbf in orbm_search_local_points); n == 0 is ORBX_OK and touches nothing, the handle
 * included.  Every other call needs the GPU: a NULL handle fails with ORBX_E_HIP where there is no HIP device ("no CPU path") and
 * with ORBX_E_INVALID where there is one.  orbm_frustum runs on the handle's stream through its staging arena (one upload, one
 * launch, one download) and grows the handle when n is larger than its workspace; the grid in the handle is not touched.
 *
 * orbm_frustum_device: the same on device pointers, the view block included (4-byte aligned).  Nothing is uploaded, downloaded
 * or synchronised, hence no count either; asynchronous on hip_stream (NULL = the handle's stream).
 *
 * orbm_search_local_points is src/Tracking.cc:1174-1199 in one call: the frustum test of every local MapPoint followed by
 * ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-125) on the points in view, when there is one (:1189).
 * The frustum arguments and outputs are orbm_frustum's; mp_desc, mp_obs, the frame side, th, nnratio, cur_obs, cur_match and
 * nmatches are orbm_search_by_projection_map's (scale_factors and nlevels come from the view; the current frame's grid must be
 * in the handle when n_cur > 0).  The projection does not return to the host between the two halves: the frustum kernel also
 * writes each point's window (RadiusByViewingCos :127-133 compared in double, times th when th != 1, times
 * mvScaleFactors[level]; levels [level-1, level]; an empty window for a point not in view) where the window pass reads it.  The
 * frustum outputs come back with the window counts and the candidates with their distances in a second round trip, so the call
 * synchronises twice, as orbm_search_by_projection_map does; the scan runs on the host in MapPoint order.
 */
typedef enum {
    ORBM_FRUSTUM_IN_VIEW = 0,    /* isInFrustum returned true (:324) */
    ORBM_FRUSTUM_SKIPPED = 1,    /* the caller's skip[i]: isInFrustum was not called (src/Tracking.cc:1177-1180) */
    ORBM_FRUSTUM_BEHIND = 2,     /* :283 */
    ORBM_FRUSTUM_OUT_X = 3,      /* :291 */
    ORBM_FRUSTUM_OUT_Y = 4,      /* :293 */
    ORBM_FRUSTUM_DISTANCE = 5,   /* :302 */
    ORBM_FRUSTUM_VIEW_COS = 6,   /* :310 */
    ORBM_FRUSTUM_UNDEFINED = 7   /* undefined in the reference: the int conversion of src/MapPoint.cc:410 */
} orbm_frustum_status;
typedef struct {
    float Rcw[9];                               /* mRcw, row-major */
    float tcw[3];                               /* mtcw */
    float Ow[3];                                /* mOw */
    float fx, fy, cx, cy;
    float mbf;
    float bounds[4];                            /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float log_scale_factor;                     /* mfLogScaleFactor */
    int32_t nlevels;                            /* mnScaleLevels */
    float scale_factors[ORBX_MAX_LEVELS];       /* mvScaleFactors */
} orbm_frame_view;
int orbm_frustum(orbm_matcher *m, const orbm_frame_view *view, int n, const uint8_t *skip, const float *xw, const float *normal,
                 const float *mf_max, const float *mf_min, float viewing_cos_limit, uint8_t *status, float *proj_x, float *proj_y,
                 float *proj_xr, int32_t *pred_level, float *view_cos, int *n_to_match);
int orbm_frustum_device(orbm_matcher *m, const orbm_frame_view *d_view, int n, const uint8_t *d_skip, const float *d_xw,
                        const float *d_normal, const float *d_mf_max, const float *d_mf_min, float viewing_cos_limit,
                        uint8_t *d_status, float *d_proj_x, float *d_proj_y, float *d_proj_xr, int32_t *d_pred_level,
                        float *d_view_cos, void *hip_stream);
int orbm_search_local_points(orbm_matcher *m, const orbm_frame_view *view, int n, const uint8_t *skip, const float *xw,
                             const float *normal, const float *mf_max, const float *mf_min, float viewing_cos_limit,
                             const uint8_t *mp_desc, const int32_t *mp_obs, const orbx_keypoint *kps_cur, const uint8_t *desc_cur,
                             const float *u_right, int n_cur, float th, float nnratio,
                             uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, int32_t *pred_level, float *view_cos,
                             int *n_to_match, int32_t *cur_obs, int32_t *cur_match, int *nmatches);

/*
 * ---- Optimizer::PoseOptimization for a batch of independent problems ----
 * Optimizer::PoseOptimization (src/Optimizer.cc:239-451) for B problems in one launch: the frames of a step, or the candidate
 * key frames of Tracking::Relocalization (src/Tracking.cc:1447, 1463, 1478).  Problem p owns the observations off[p]:off[p+1] of
 * obs (2 floats each), u_right, inv_sigma2 and xw (3 floats each), the camera cams[p] and the pose Tcw[16p .. 16p+16); per problem
 * the meaning of every array is that of orbp_pose_optimization (include/orbp.h) with n = off[p+1] - off[p]:
 *   u_right == NULL: every edge is monocular; otherwise u_right[i] < 0 marks a monocular edge and u_right[i] >= 0 a stereo edge
 *   Tcw        = pFrame->mTcw (row-major 4x4) on entry, the optimised pose on return
 *   outlier[i] = mvbOutlier of the observation; bytes outside the problems' ranges are not written
 *   n_good[p]  = the function's return value (nInitialCorrespondences - nBad)
 * A problem with fewer than 3 observations keeps its pose bit for bit, clears its flags and reports n_good[p] = 0 (:363-364).
 *
 * One workgroup solves one problem and restates the host path operation by operation in fp64: every per-edge
 * quantity is bit-identical to orbp_pose_optimization's, and the sums over the edges are added in a fixed tree instead of in edge
 * order, so the pose agrees with the host's to rounding (2e-6 on the fp32 output) and a flag can differ only for an edge whose
 * chi2 lies within rounding of its threshold.  The result of a problem does not depend on the batch around it, on its position in
 * the batch or on the run.  There is no limit on n.  Non-finite inputs and points at depth 0 are outside the contract.
 *
 * Argument checks come before any device work (ORBX_E_INVALID: a negative count, NULL buffers, off[0] != 0 or a decreasing off,
 * and in the host variant a stereo edge in a problem whose camera has bf == 0); n_problems == 0 is ORBX_OK and touches nothing.
 * Every other call needs the GPU: a NULL handle fails with ORBX_E_HIP where there is no HIP device ("no CPU path") and with
 * ORBX_E_INVALID where there is one.  orbm_pose_optimization_batch runs on the handle's stream through its staging arena (one
 * upload, one launch, one download) and grows the handle when the batch is larger than its workspace; the grids in the handle
 * are not touched.  For a single frame the host path orbp_pose_optimization is the faster one (README).
 *
 * orbm_pose_optimization_batch_device: the same on device pointers (4-byte aligned; off and cams included).  Nothing is
 * uploaded, downloaded, synchronised or grown; asynchronous on hip_stream (NULL = the handle's stream), capturable.
 */
typedef struct { float fx, fy, cx, cy, bf; } orbm_pose_camera;
int orbm_pose_optimization_batch(orbm_matcher *m, int n_problems, const int32_t *off, const float *obs, const float *u_right,
                                 const float *inv_sigma2, const float *xw, const orbm_pose_camera *cams, float *Tcw,
                                 uint8_t *outlier, int32_t *n_good);
int orbm_pose_optimization_batch_device(orbm_matcher *m, int n_problems, const int32_t *d_off, const float *d_obs,
                                        const float *d_u_right, const float *d_inv_sigma2, const float *d_xw,
                                        const orbm_pose_camera *d_cams, float *d_Tcw, uint8_t *d_outlier, int32_t *d_n_good,
                                        void *hip_stream);

/*
 * ---- Optimizer::OptimizeSim3 for a batch of independent problems ----
 * Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) for B problems in one launch: the loop candidates of one round of
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:287-343) whose Sim3Solver returned a Scm.  Problem p owns the pairs
 * off[p]:off[p+1] of x1c, x2c (3 floats each), obs1, obs2 (2 floats each), inv_sigma2_1 and inv_sigma2_2, the two calibrations
 * cams[8p .. 8p+8) = {fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2}, th2[p], fix_scale[p] (0 / not 0) and S12[8p .. 8p+8) (doubles, in
 * and out); per problem the meaning of every array is that of orbp_optimize_sim3 (include/orbp.h) with n = off[p+1] - off[p]:
 *   flags[i] = 1 where the reference sets vpMatches1[idx] = NULL; bytes outside the problems' ranges are not written
 *   n_in[p]  = the function's return value; 0 with S12 of the problem untouched bit for bit when fewer than 10 pairs survive the
 *              first pass (:1211-1212)
 *
 * One workgroup solves one problem with the text of the host path (csrc/orbp_sim3opt_body.h is compiled by both); the sums over
 * the pairs are added in a fixed tree instead of in edge order, so S12 agrees with the host's to the spread
 * of tests/golden/sim3opt/tolerance.json and a flag can differ only for a pair whose chi2 lies within rounding of th2.  The result
 * of a problem does not depend on the batch around it, on its position in the batch or on the run.  There is no limit on n.
 * Non-finite correspondences and points at depth 0 are outside the contract.
 *
 * Argument checks come before any device work (ORBX_E_INVALID: a negative count, NULL buffers, off[0] != 0 or a decreasing off,
 * and in the host variant a non-finite S12); n_problems == 0 is ORBX_OK and touches nothing.  Every other call needs the GPU: a
 * NULL handle fails with ORBX_E_HIP where there is no HIP device and with ORBX_E_INVALID where there is one.
 * orbm_optimize_sim3_batch runs on the handle's stream through its staging arena (one upload, one launch, one download) and grows
 * the handle when the batch is larger than its workspace; the grids in the handle are not touched.
 *
 * orbm_optimize_sim3_batch_device: the same on device pointers (4-byte aligned, d_S12 8-byte aligned).  Nothing is uploaded,
 * downloaded, synchronised or grown; asynchronous on hip_stream (NULL = the handle's stream), capturable.
 */
int orbm_optimize_sim3_batch(orbm_matcher *m, int n_problems, const int32_t *off, const float *x1c, const float *x2c, const float *obs1,
                             const float *obs2, const float *inv_sigma2_1, const float *inv_sigma2_2, const float *cams,
                             const float *th2, const int32_t *fix_scale, double *S12, uint8_t *flags, int32_t *n_in);
int orbm_optimize_sim3_batch_device(orbm_matcher *m, int n_problems, const int32_t *d_off, const float *d_x1c, const float *d_x2c,
                                    const float *d_obs1, const float *d_obs2, const float *d_inv_sigma2_1,
                                    const float *d_inv_sigma2_2, const float *d_cams, const float *d_th2, const int32_t *d_fix_scale,
                                    double *d_S12, uint8_t *d_flags, int32_t *d_n_in, void *hip_stream);

/*
 * ---- Sim3Solver: the hypotheses of all loop candidates in one call ----
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:253-343) runs up to 300 RANSAC iterations per candidate key frame, five at a time
 * (Sim3Solver::iterate, src/Sim3Solver.cc:140-207).  An iteration is a 3-point Horn solve (ComputeSim3, :226-337) and two
 * projections of all correspondences (CheckInliers, :340-364); the draws do not depend on the results, so every hypothesis of
 * every candidate can be evaluated at once.  orbm_sim3_hypotheses does that for B problems:
 *   problem p owns the correspondences off[p]:off[p+1] of x3dc1 / x3dc2 (the point in camera 1 / 2, 3 floats each) and of
 *   max_err1 / max_err2 (mvnMaxError1/2 as floats: orbp_sim3_get_problem), the calibrations and mbFixScale in cams[p], and
 *   the hypotheses hyp_off[p]:hyp_off[p+1]; hypothesis h samples the correspondences triples[3h .. 3h+3) of its problem
 *   (indices relative to off[p]: what orbp_sim3_draw records);
 *   n_inliers[h] = mnInliersi, sRt[13h .. 13h+13) = ms12i, mR12i (row-major), mt12i;
 *   masks: hypothesis h of problem p owns the W = ceil(n_p / 32) words from mask_off[p] + (h - hyp_off[p]) * W; bit i of them is
 *   mvbInliersi[i], bits >= n_p are zero.  mask_off[0] = 0 and mask_off[p+1] = mask_off[p] + (hyp_off[p+1] - hyp_off[p]) * W.
 * The outputs are the inputs of orbp_sim3_attach_results (include/orbp.h), after which Sim3Solver::iterate replays them.
 *
 * One wave evaluates one hypothesis with the text of the host solver (csrc/orbm_sim3_body.h: IEEE operations only, its own
 * atan2 / sin / cos), so every output equals orbp_sim3_hypothesis' byte for byte.  The result of a hypothesis depends on its
 * problem and its triple alone, not on the batch, its position or the run.  There is no limit on n.  A triple whose points are
 * collinear or coincident within rounding is outside the value contract: its flags are still 0/1, its count is its mask's
 * popcount and nothing outside its slots is written.  Points at depth 0 and non-finite inputs are outside the contract.
 *
 * Argument checks come before any device work (ORBX_E_INVALID: a negative count, NULL buffers, off / hyp_off / mask_off not
 * starting at 0, a decreasing off or hyp_off, a mask_off that is not the layout above, a triple index outside its problem);
 * n_problems == 0 or no hypothesis at all is ORBX_OK and touches nothing.  Every other call needs the GPU: a NULL handle fails
 * with ORBX_E_HIP where there is no HIP device ("no CPU path") and with ORBX_E_INVALID where there is one.  The call runs on the
 * handle's stream through its staging arena (one upload, one launch, one download) and grows the handle when the batch is larger
 * than its workspace; the grids in the handle are not touched.
 *
 * orbm_sim3_hypotheses_device: the same on device pointers (4-byte aligned, mask_off 8-byte aligned).  total_hypotheses =
 * hyp_off[n_problems] (the launch size: the host cannot read it).  The index arrays are not checked (a triple index outside its
 * problem is clamped into it).  Nothing is uploaded, downloaded, synchronised or grown; asynchronous on hip_stream (NULL = the
 * handle's stream), capturable.
 */
typedef struct { float K1[4], K2[4]; int32_t fix_scale; } orbm_sim3_camera;     /* {fx, fy, cx, cy} of key frame 1 / 2, mbFixScale */
int orbm_sim3_hypotheses(orbm_matcher *m, int n_problems, const int32_t *off, const float *x3dc1, const float *x3dc2,
                         const float *max_err1, const float *max_err2, const orbm_sim3_camera *cams, const int32_t *hyp_off,
                         const int32_t *triples, const int64_t *mask_off, int32_t *n_inliers, float *sRt, uint32_t *masks);
int orbm_sim3_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_x3dc1,
                                const float *d_x3dc2, const float *d_max_err1, const float *d_max_err2,
                                const orbm_sim3_camera *d_cams, const int32_t *d_hyp_off, const int32_t *d_triples,
                                const int64_t *d_mask_off, int32_t *d_n_inliers, float *d_sRt, uint32_t *d_masks, void *hip_stream);

/*
 * ---- PnPsolver: the EPnP hypotheses of all Relocalization candidates in one call ----
 * Tracking::Relocalization (src/Tracking.cc:1348-1509) runs PnPsolver::iterate(5, ...) per candidate key frame (:1405-1418); with
 * the reference's `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` (src/PnPsolver.cc:182) the first call runs
 * all mRansacMaxIts iterations unless a refined pose comes back earlier.  An iteration is an EPnP solve on the drawn set
 * (compute_pose, :458-508) and a projection of all correspondences (CheckInliers, :312-344); the draws do not depend on the results,
 * so every hypothesis of every candidate can be evaluated at once.  orbm_pnp_hypotheses does that for B problems:
 *   problem p owns the correspondences off[p]:off[p+1] of p2d (mvP2D, 2 floats each), p3d (mvP3Dw, 3 floats) and max_err
 *   (mvMaxError = sigma2 * th2 as the float CheckInliers compares with: orbp_pnp_get_problem), cams[p] = the calibration and
 *   mRansacMinSet, and the hypotheses hyp_off[p]:hyp_off[p+1]; hypothesis h samples the correspondences
 *   samples[8h .. 8h + set_size) of its problem (indices relative to off[p]: what orbp_pnp_draw records); the stride is 8 ints
 *   (ORBM_PNP_MAX_SET) whatever set_size is, the entries from set_size on are -1 and are not read;
 *   n_inliers[h] = mnInliersi, Rt[12h .. 12h+12) = mRi (row-major), then mti, as the doubles the host solver holds;
 *   masks: as for orbm_sim3_hypotheses above (W = ceil(n_p / 32) words per hypothesis from mask_off[p] on, bit i = mvbInliersi[i]).
 * The outputs are the inputs of orbp_pnp_attach_results (include/orbp.h), after which PnPsolver::iterate replays them; Refine stays
 * on the host.
 *
 * One wave evaluates one hypothesis with the text of the host solver (csrc/orbp_epnp_body.h: IEEE + - * / sqrt only, every sum in
 * the host's order), so every output equals orbp_pnp_hypothesis' byte for byte.  The result of a hypothesis depends on its problem
 * and its sample alone.  There is no limit on n; set_size is 4 to 8 (a solver with a larger mRansacMinSet stays on the host).  A
 * sample with coincident, collinear or otherwise degenerate points is outside the value contract: its flags are still 0/1, its
 * count is its mask's popcount and nothing outside its slots is written.  Non-finite inputs are outside the contract.
 *
 * Argument checks come before any device work (ORBX_E_INVALID: a negative count, NULL buffers, off / hyp_off / mask_off not
 * starting at 0, a decreasing off or hyp_off, a mask_off that is not the layout above, a set_size outside [4, 8] on a problem with
 * hypotheses, a sample index outside its problem or repeated within its sample); n_problems == 0 or no hypothesis at all is
 * ORBX_OK and touches nothing.  NULL handle, stream, staging arena and growth as for orbm_sim3_hypotheses; the grids in the
 * handle are not touched.
 *
 * orbm_pnp_hypotheses_device: the same on device pointers (4-byte aligned; Rt and mask_off 8-byte aligned).  total_hypotheses =
 * hyp_off[n_problems].  The index arrays are not checked (a sample index outside its problem is clamped into it, a set_size
 * outside [4, 8] into that range).  Nothing is uploaded, downloaded, synchronised or grown; asynchronous on hip_stream (NULL = the
 * handle's stream), capturable.
 */
#define ORBM_PNP_MAX_SET 8
typedef struct { float fx, fy, cx, cy; int32_t set_size; } orbm_pnp_camera;
int orbm_pnp_hypotheses(orbm_matcher *m, int n_problems, const int32_t *off, const float *p2d, const float *p3d, const float *max_err,
                        const orbm_pnp_camera *cams, const int32_t *hyp_off, const int32_t *samples, const int64_t *mask_off,
                        int32_t *n_inliers, double *Rt, uint32_t *masks);
int orbm_pnp_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_p2d,
                               const float *d_p3d, const float *d_max_err, const orbm_pnp_camera *d_cams, const int32_t *d_hyp_off,
                               const int32_t *d_samples, const int64_t *d_mask_off, int32_t *d_n_inliers, double *d_Rt, uint32_t *d_masks,
                               void *hip_stream);

/*
 * ---- Initializer: the H / F hypotheses of Tracking::MonocularInitialization and the CheckRT passes, one call each ----
 * Initializer::Initialize (src/Initializer.cc:44-121) draws all its index sets first (:77-97), then evaluates mMaxIterations
 * homographies (FindHomography, :148-171) and as many fundamental matrices (FindFundamental, :199-222): each is one small SVD on
 * the 8 drawn matches and a pass over all matches.  orbm_init_hypotheses does that for B problems (one per camera or session):
 *   problem p owns the matches off[p]:off[p+1] of uv (4 floats each: kp1.pt.x, kp1.pt.y, kp2.pt.x, kp2.pt.y of mvMatches12[i]) and
 *   pn (the same four after Normalize, :132-133), params[p] = T1, T2 (row-major 3 x 3) and sigma, and the hypotheses
 *   hyp_off[p]:hyp_off[p+1]; hypothesis h runs model models[h] (0: ComputeH21 + CheckHomography, 1: ComputeF21 +
 *   CheckFundamental) on the matches sets[8h .. 8h+8) of its problem (indices relative to off[p]: what orbp_init_draw records);
 *   score_M[10h] = currentScore, score_M[10h+1 .. 10h+10) = H21i / F21i (row-major), n_inliers[h] = the number of set flags;
 *   masks: W = ceil(n_p / 32) words per hypothesis from mask_off[p] on, bit i = vbCurrentInliers[i] (as orbm_sim3_hypotheses).
 * The outputs are the inputs of orbp_init_attach_results (include/orbp.h), after which the two walks are a replay.
 *
 * One wave evaluates one hypothesis with the text of the host solver (csrc/orbp_init_body.h: IEEE + - * / sqrt only, every sum in
 * the host's order; the score is added in match order, term 1 then term 2, never by a tree), so every output equals
 * orbp_init_hypothesis' byte for byte.  The result of a hypothesis depends on its problem, its set and its model alone.  A set
 * with collinear, repeated or otherwise degenerate points is outside the value contract: its flags are still 0/1, its count is its
 * mask's popcount and nothing outside its slots is written.  Non-finite inputs are outside the contract.
 *
 * Argument checks come before any device work (ORBX_E_INVALID: a negative count, NULL buffers, off / hyp_off / mask_off not
 * starting at 0, a decreasing off or hyp_off, a mask_off that is not the layout above, a model other than 0 / 1, a set index outside
 * its problem); n_problems == 0 or no hypothesis at all is ORBX_OK and touches nothing.  NULL handle, stream, staging arena and
 * growth as for orbm_sim3_hypotheses; the grids in the handle are not touched.
 *
 * orbm_init_hypotheses_device: the same on device pointers (4-byte aligned, mask_off 8-byte aligned).  total_hypotheses =
 * hyp_off[n_problems].  The index arrays are not checked (a set index outside its problem is clamped into it, a model other than 0
 * runs as 1).  Nothing is uploaded, downloaded, synchronised or grown; asynchronous on hip_stream (NULL = the handle's stream).
 *
 * orbm_init_check_rt: CheckRT (:798-907) of n_motions candidate motions (Rt: 12 floats each, R row-major then t; 4 from
 * ReconstructF, 8 from ReconstructH) on the n matches uv of ONE problem, one lane per (motion, match): for pair g = motion * n +
 * match, status[g] names the line that decided it (orbm_init_rt_status), cos_parallax[g] is cosParallax (0 before it is computed),
 * p3d[3g .. 3g+3) is p3dC1 when the status is one of the two GOOD and 0 otherwise.  K = {fx, fy, cx, cy}, th2 = 4 * mSigma2.
 * inliers[n] (0/1) = vbMatchesInliers.  Counting nGood, sorting vCosParallax and the acceptance rules stay on the host
 * (orbp_init_attach_check_rt).  Byte for byte orbp_init_check_rt_matches.  The _device form takes device pointers (K stays a host
 * pointer: it is passed by value) and neither copies nor synchronises.
 */
#define ORBM_INIT_MAX_MOTIONS 8
typedef struct { float T1[9], T2[9], sigma; } orbm_init_params;
typedef enum {
    ORBM_INIT_RT_GOOD = 0,              /* :888-893: counted, vP3D written, vbGood set */
    ORBM_INIT_RT_GOOD_LOW_PARALLAX = 1, /* the same with cosParallax >= 0.99998: vbGood stays false (:892) */
    ORBM_INIT_RT_NOT_INLIER = 2,        /* :832 */
    ORBM_INIT_RT_NOT_FINITE = 3,        /* :841 */
    ORBM_INIT_RT_BEHIND1 = 4,           /* :857 */
    ORBM_INIT_RT_BEHIND2 = 5,           /* :863 */
    ORBM_INIT_RT_REPROJ1 = 6,           /* :874 */
    ORBM_INIT_RT_REPROJ2 = 7            /* :885 */
} orbm_init_rt_status;
int orbm_init_hypotheses(orbm_matcher *m, int n_problems, const int32_t *off, const float *uv, const float *pn,
                         const orbm_init_params *params, const int32_t *hyp_off, const int32_t *sets, const int32_t *models,
                         const int64_t *mask_off, float *score_M, int32_t *n_inliers, uint32_t *masks);
int orbm_init_hypotheses_device(orbm_matcher *m, int n_problems, int total_hypotheses, const int32_t *d_off, const float *d_uv,
                                const float *d_pn, const orbm_init_params *d_params, const int32_t *d_hyp_off, const int32_t *d_sets,
                                const int32_t *d_models, const int64_t *d_mask_off, float *d_score_M, int32_t *d_n_inliers,
                                uint32_t *d_masks, void *hip_stream);
int orbm_init_check_rt(orbm_matcher *m, int n, const float *uv, const uint8_t *inliers, const float *K, float th2, int n_motions,
                       const float *Rt, uint8_t *status, float *cos_parallax, float *p3d);
int orbm_init_check_rt_device(orbm_matcher *m, int n, const float *d_uv, const uint8_t *d_inliers, const float *K, float th2,
                              int n_motions, const float *d_Rt, uint8_t *d_status, float *d_cos_parallax, float *d_p3d, void *hip_stream);

/*
 * ---- ORBmatcher::Fuse for ALL target key frames of LocalMapping::SearchInNeighbors in one call ----
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc:456-536) calls Fuse(pKFi, vpMapPointMatches) once per target key frame
 * (:487-492) and once more with every MapPoint of those key frames against mpCurrentKeyFrame (:516).  orbm_fuse_views runs
 * src/ORBmatcher.cc:852-952 for every (view, MapPoint) slot on ONE snapshot: projection, gates, PredictScale, the window, the octave
 * window, the chi-square gate and the Hamming selection, without returning to the host in between.  What happens to a fused
 * point (:954-970) is object-graph work and stays with the caller, who replays it in the reference's order; of everything the
 * search reads, only a MapPoint's descriptor can change between two key frames of the loop (MapPoint::Replace ends with
 * ComputeDistinctiveDescriptors on the survivor, src/MapPoint.cc:177-215), and only the Hamming selection (:940-949) reads it, so
 * the caller re-selects on the host for the slots whose live descriptor differs from the snapshot's (host/ORBmatcher.h, DESIGN.md
 * section 17).
 *
 * orbm_fuse_view is what the loop reads of a key frame beyond its features: Rcw / tcw / Ow = GetRotation(), GetTranslation(),
 * GetCameraCenter(), the calibration, mbf, bounds = (float) mnMinX, mnMaxX, mnMinY, mnMaxY, log_scale_factor = mfLogScaleFactor,
 * nlevels = mnScaleLevels, scale_factors = mvScaleFactors, inv_level_sigma2 = mvInvLevelSigma2 (entries past nlevels are not
 * read) and grid as for orbm_grid_build_kf.  The views' features are concatenated: view v owns off[v] .. off[v+1]-1 of kps_un
 * (mvKeysUn), u_right (mvuRight) and desc_kf (32 bytes each).
 *   per slot (v, i), slot = v*n_mp + i:  skip = !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF_v) (:846-850)
 *   per MapPoint i:  xw = GetWorldPos(), normal = GetNormal(), mf_max / mf_min = the raw mfMaxDistance / mfMinDistance (the 1.2f
 *                    and 0.8f of the two getters are applied here, PredictScale divides the raw mfMaxDistance), mp_desc =
 *                    GetDescriptor()
 *   status[slot]     the line that decided the slot (orbm_fuse_status)
 *   best_idx[slot]   ORBM_FUSE_MATCH: the feature inside view v the point is fused with (bestIdx at :952); -1 otherwise
 *   best_dist[slot]  the smallest distance among the candidates that survived the octave window and the gate, also when it is
 *                    above TH_LOW; 256 when there is none (and for a slot that was not searched)
 *   proj_u, proj_v, proj_ur, pred_level = u, v, ur, nPredictedLevel of the slots that reached :887 (MATCH and NO_MATCH), zeros
 *                    for every other slot
 *   nfused[v]        the slots of view v with ORBM_FUSE_MATCH
 * The first candidate in the reference's order (cell column, cell row, push_back order) wins a tie.
 *
 * Arithmetic: :852-890 operation by operation under the conventions of DESIGN.md section 2, without contraction: Rcw*p+tcw through
 * cv::gemm's small-matrix path, invz = 1/z a float division, x = Pc0*invz and then u = fx*x+cx (the order of :860-864, not
 * isInFrustum's), ur = u - bf*invz, cv::norm and Mat::dot accumulated in double, PO.dot(Pn) compared with 0.5*dist3D in double,
 * PredictScale as float division, correctly rounded logf, float division, ceil (orbm_frustum's, same code), radius =
 * th*scale_factors[level].  The reference's quirks are kept: z == +-0 passes :856 and fails :867, a NaN u or v fails
 * KeyFrame::IsInImage ([min, max) on both axes; unlike isInFrustum), a NaN normal passes :884.  ORBM_FUSE_UNDEFINED as
 * ORBM_FRUSTUM_UNDEFINED.  A key point whose octave lies outside its view's levels causes no out-of-range read: it is clamped
 * into [0, ORBX_MAX_LEVELS) where mvInvLevelSigma2 is indexed, as orbm_fuse does (the octave window has dropped every such key
 * point but octave -1 next to level 0, which is gated with level 0's sigma).
 *
 * Argument checks come before any device work (ORBX_E_INVALID: negative counts, NULL buffers where the count is positive, off
 * not monotone from 0, nlevels outside [1, ORBX_MAX_LEVELS], grid cell sizes that are not positive; ORBX_E_CAPACITY: nviews *
 * n_mp > 2^28 or more than 65535 views).  nviews == 0 or n_mp == 0 is ORBX_OK and touches nothing, the handle and the outputs
 * included.  A call with every skip set, or with every view empty, is answered on the host (the same arithmetic) and needs no
 * handle; every other call needs the GPU, and a NULL handle behaves as in orbm_create_new_map_points.  A failed call leaves
 * every output as it was.  The call runs on the handle's stream through its staging arena: one upload, the grid launch (one
 * workgroup per view) and the search launch with nothing returning to the host in between, one download, one synchronisation.
 * It grows the handle as needed and keeps the views' grids in storage of its own: the two grid slots of the handle are left as
 * found (orbm_grid_count() and a following windowed search are unchanged by it).  The result for a view does not depend on the
 * views around it, on its position in the batch or on the run.
 */
typedef enum {
    ORBM_FUSE_MATCH = 0,       /* reached :952 with bestDist <= TH_LOW; best_idx >= 0 */
    ORBM_FUSE_SKIPPED = 1,     /* the caller's skip: :846-850 */
    ORBM_FUSE_BEHIND = 2,      /* :856 */
    ORBM_FUSE_OUT_IMAGE = 3,   /* :867, KeyFrame::IsInImage: [min, max) on both axes; a NaN u or v FAILS here (unlike isInFrustum) */
    ORBM_FUSE_DISTANCE = 4,    /* :878 */
    ORBM_FUSE_VIEW_ANGLE = 5,  /* :884: PO.dot(Pn) (double) < 0.5 * dist3D (double); NaN passes */
    ORBM_FUSE_UNDEFINED = 6,   /* the int conversion in PredictScale, as ORBM_FRUSTUM_UNDEFINED */
    ORBM_FUSE_NO_MATCH = 7     /* searched: empty window (:894), every member dropped by :911 / :925 / :936, or bestDist > TH_LOW */
} orbm_fuse_status;
typedef struct {
    float Rcw[9], tcw[3], Ow[3];                /* GetRotation() (row-major), GetTranslation(), GetCameraCenter() */
    float fx, fy, cx, cy, mbf;
    float bounds[4];                            /* (float) mnMinX, mnMaxX, mnMinY, mnMaxY */
    float log_scale_factor;                     /* mfLogScaleFactor */
    int32_t nlevels;                            /* mnScaleLevels */
    float scale_factors[ORBX_MAX_LEVELS];       /* mvScaleFactors */
    float inv_level_sigma2[ORBX_MAX_LEVELS];    /* mvInvLevelSigma2 */
    orbm_kf_grid grid;                          /* as for orbm_grid_build_kf */
} orbm_fuse_view;
int orbm_fuse_views(orbm_matcher *m, const orbm_fuse_view *views, int nviews, const int32_t *off,
                    const orbx_keypoint *kps_un, const float *u_right, const uint8_t *desc_kf,
                    int n_mp, const uint8_t *skip,
                    const float *xw, const float *normal, const float *mf_max, const float *mf_min,
                    const uint8_t *mp_desc, float th,
                    uint8_t *status, int32_t *best_idx, int32_t *best_dist,
                    float *proj_u, float *proj_v, float *proj_ur, int32_t *pred_level,
                    int32_t *nfused);

/*
 * ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778), LocalMapping::Run's call at src/LocalMapping.cc:82 ----
 * The problem, outputs, `stop`, `stats` and return codes of orbp_local_bundle_adjustment (include/orbp.h), whose argument checks run
 * first and need no handle; so does a `stop` set at entry, which launches nothing.  Everything else needs the GPU, and a NULL handle
 * behaves as in orbm_create_new_map_points.  The kernels run the text of the host path (csrc/orbp_lba_body.h): every per-edge
 * quantity is the host's bit for bit; the sums over edges (fixed trees instead of edge order), the device's sin / cos and the inside
 * of the dense solve are not, so the results agree with the host's within the bar of tests/golden/lba/tolerance.json and the flags
 * and counts are identical away from the decision boundaries.
 *
 * The call runs on the handle's stream: one upload through the staging arena, one download of the results at the end, and between
 * them a Levenberg loop driven by the host over plain kernel launches in stream order.  After each trial the host reads back one
 * 64-byte block (the trial's robust chi2, computeScale's sum, the solve's ok flag) and takes g2o's decisions in the body's own code;
 * that is also where `stop` is read.  At most 15 iterations x 10 trials.  No cooperative launch, no grid-wide barrier, no spin-wait,
 * no communication between workgroups other than kernel boundaries, no floating-point atomics; every kernel loop is bounded by the
 * problem's counts.  The result is a function of the problem alone: byte-equal on a second run and on a handle that solved another
 * problem in between.  The workspace is a block of the handle's own (grown by the rule of csrc/dev_buf.h); the grid slots and every
 * other buffer of the handle are left as found.  The three results leave the device in one copy into the staging arena and reach
 * the caller's arrays after the last synchronisation, so a failed call leaves every output as it was; only when the arena has no
 * room left in this call do the copies land in the arrays directly, and a failure after that may leave them partly written.
 *
 * ORBX_E_CAPACITY beyond ORBM_LBA_MAX_LOCAL local key frames: the reduced system is factored by one workgroup, whose time grows
 * with the cube of 6 n_local and which a call may run 150 times (DESIGN.md section 22 has the time at the cap); and beyond 2^28
 * entries of the n_local x n_points table.  The host path has neither limit.
 */
#define ORBM_LBA_MAX_LOCAL 128
struct orbp_lba_problem;
struct orbp_lba_stats;
int orbm_local_bundle_adjustment(orbm_matcher *m, const struct orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase,
                                 const volatile uint8_t *stop, struct orbp_lba_stats *stats);
/*
 * The same call, measured (tools/bench_lba.py): events on the handle's stream after each group of launches.  split_ms[g] is the
 * device time of group g summed over the call and split_count[g] the number of times it ran (both ORBM_LBA_SPLIT_N long).  A
 * group's time runs from the end of the group before it, or from the host's return from the synchronisation before it, to its own
 * end, so the time until the host has enqueued it counts into it.  Results and stats are those of orbm_local_bundle_adjustment,
 * bit for bit.  ORBX_E_INVALID on a NULL split_ms or split_count.
 */
enum {
    ORBM_LBA_SPLIT_UPLOAD = 0,          /* the one staged upload */
    ORBM_LBA_SPLIT_SETUP = 1,           /* table memset, k_lba_init; k_lba_activate and its memsets (twice) */
    ORBM_LBA_SPLIT_ERRORS = 2,          /* k_lba_errors */
    ORBM_LBA_SPLIT_LINEARIZE = 3,       /* k_lba_linearize */
    ORBM_LBA_SPLIT_REDUCE_POINTS = 4,   /* k_lba_reduce_points */
    ORBM_LBA_SPLIT_REDUCE_KFS = 5,      /* k_lba_reduce_kfs */
    ORBM_LBA_SPLIT_DINV = 6,            /* k_lba_dinv */
    ORBM_LBA_SPLIT_SCHUR = 7,           /* k_lba_schur */
    ORBM_LBA_SPLIT_SOLVE = 8,           /* k_lba_solve */
    ORBM_LBA_SPLIT_UPDATE = 9,          /* k_lba_update */
    ORBM_LBA_SPLIT_READ_BACK = 10,      /* k_lba_reduce_out and the 64-byte copy the host then waits for */
    ORBM_LBA_SPLIT_FLAG_OUTPUT = 11,    /* k_lba_flag (both passes), k_lba_output */
    ORBM_LBA_SPLIT_DOWNLOAD = 12,       /* the one copy of the results */
    ORBM_LBA_SPLIT_N = 13
};
int orbm_local_bundle_adjustment_split(orbm_matcher *m, const struct orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase,
                                       const volatile uint8_t *stop, struct orbp_lba_stats *stats, double *split_ms,
                                       int32_t *split_count);

/*
 * ---- A dense symmetric positive definite solve in fp64 over many workgroups (csrc/orbm_spd.hip) ----
 * A x = b for the symmetric positive definite n x n A (row-major; its lower triangle is read), by a blocked Cholesky
 * factorisation: panels of 48 columns, each a diagonal-block launch of one workgroup, a panel solve over row tiles and a
 * trailing update over the tiles of the lower triangle, then both substitutions panel by panel: 5 ceil(n / 48) - 2 launches in
 * stream order.  No cooperative launch, no grid-wide barrier, no spin-wait, nothing between workgroups but kernel boundaries,
 * no atomic; every loop is bounded by n; x is a function of (A, b) alone.  This is the host-array entry, for tests and
 * measurements: it uploads into the optimizer workspace of the handle, runs the device routine that
 * orbm_bundle_adjustment runs on its reduced system, and downloads.  *ok = 1, or 0 where a pivot was not positive or not finite:
 * x is then all zeros and the call still returns ORBX_OK (the later launches of the solve see the device flag and return at
 * once; nothing traps and nothing is read back between the panels).
 * ORBX_E_INVALID on a NULL argument or n < 1, ORBX_E_CAPACITY beyond ORBM_SPD_MAX_N.  tests/test_spd_gpu.py runs the solve up to
 * and at ORBM_SPD_MAX_N: against Higham's backward error bound, and on systems whose exact solution it must return byte for byte.
 */
#define ORBM_SPD_MAX_N 3072
int orbm_spd_solve_f64(orbm_matcher *m, const double *A, const double *b, int n, double *x, int *ok);

/*
 * ---- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:41-237) on the GPU ----
 * The problem, arguments, semantics and return codes of orbp_bundle_adjustment (include/orbp.h), whose argument checks run
 * first and need no handle.  It is the driver of orbm_local_bundle_adjustment over the same launches, with the call's robust
 * kernel, one optimize(n_iterations), and the solve above in place of the one-workgroup k_lba_solve: per iteration k_lba_errors /
 * k_lba_linearize, k_lba_reduce_points, k_lba_reduce_kfs; per trial k_lba_dinv, k_lba_schur, the solve, k_lba_update,
 * k_lba_errors, k_lba_reduce_out and its 64-byte read-back, where `stop` is read; at the end k_lba_output.  One upload, one
 * download.  Results agree with the host path's within the bar of tests/golden/ba/tolerance.json, counts are identical away from
 * the decision boundaries, and a second run gives the same bytes.
 *
 * ORBX_E_CAPACITY, decided from the counts before any allocation or launch: beyond ORBM_BA_MAX_KFS local key frames (the dense
 * reduced system is then 75 MB) or beyond ORBM_BA_MAX_TABLE entries of the n_local x n_points table of edge indices.  Larger
 * maps need a sparse reduced system, which is not built here.
 * orbm_bundle_adjustment_split is the same call measured as orbm_local_bundle_adjustment_split measures: the groups are the
 * ORBM_LBA_SPLIT_* above, ORBM_LBA_SPLIT_SOLVE holding every launch of the many-workgroup solve.
 */
#define ORBM_BA_MAX_KFS 512
#define ORBM_BA_MAX_TABLE (1 << 26)
struct orbp_ba_stats;
int orbm_bundle_adjustment(orbm_matcher *m, const struct orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local, float *xw,
                           const volatile uint8_t *stop, struct orbp_ba_stats *stats);
int orbm_bundle_adjustment_split(orbm_matcher *m, const struct orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local,
                                 float *xw, const volatile uint8_t *stop, struct orbp_ba_stats *stats, double *split_ms,
                                 int32_t *split_count);

/*
 * ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044) on the GPU ----
 * The problem, arguments, semantics and return codes of orbp_optimize_essential_graph (include/orbp.h), whose argument checks
 * run first and need no handle.  Host and kernels run one text (csrc/orbp_eg_body.h); the host drives lm_optimize as
 * orbm_bundle_adjustment does.  Once a call k_eg_measure (the edges' measurements); per iteration k_eg_linearize (the 29 error
 * evaluations of an edge's numeric Jacobian over 29 threads), k_eg_diag and k_eg_offdiag (one wave per vertex / per vertex pair
 * sums its blocks in edge order into the dense 7N x 7N H0: no atomics, every sum in a fixed order); per trial k_eg_stage
 * (H0 + lambda I and b into the work matrix), the many-workgroup solve of orbm_spd_solve_f64, k_eg_update, k_eg_errors,
 * k_eg_reduce_out and its 64-byte read-back; at the end k_eg_output and k_eg_points.  One upload, one download.  Results agree
 * with the host path's within the bar of tests/golden/eg/tolerance.json and a second run gives the same bytes (DESIGN.md
 * section 24).
 *
 * ORBX_E_CAPACITY, decided from the counts before any allocation or launch: beyond ORBM_EG_MAX_KFS key frames, which keeps the
 * 7 x 438 = 3066 unknowns inside ORBM_SPD_MAX_N, the range the solve has been tested and measured in (tests/test_spd_gpu.py at
 * n = 3066 and 3072; tests/test_eg_gpu.py holds this call to the oracle at 438 key frames).  The host path has no cap.
 * orbm_optimize_essential_graph_split is the same call with split_ms[g] = the device time of group g summed over the call and
 * split_count[g] the number of times it ran (both ORBM_EG_SPLIT_N long), measured as orbm_local_bundle_adjustment_split measures.
 */
#define ORBM_EG_MAX_KFS 438
enum {
    ORBM_EG_SPLIT_UPLOAD = 0,           /* the one staged upload, the memsets, k_eg_measure */
    ORBM_EG_SPLIT_LINEARIZE = 1,        /* k_eg_linearize */
    ORBM_EG_SPLIT_ASSEMBLE = 2,         /* k_eg_diag, k_eg_offdiag */
    ORBM_EG_SPLIT_STAGE = 3,            /* k_eg_stage */
    ORBM_EG_SPLIT_SOLVE = 4,            /* every launch of the many-workgroup solve */
    ORBM_EG_SPLIT_UPDATE_ERRORS = 5,    /* k_eg_update, k_eg_errors */
    ORBM_EG_SPLIT_READ_BACK = 6,        /* k_eg_reduce_out and the 64-byte copy the host then waits for */
    ORBM_EG_SPLIT_OUTPUT = 7,           /* k_eg_output, k_eg_points, the one copy of the results */
    ORBM_EG_SPLIT_N = 8
};
struct orbp_eg_problem;
struct orbp_eg_stats;
int orbm_optimize_essential_graph(orbm_matcher *m, const struct orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw,
                                  double *Scw_out, struct orbp_eg_stats *stats);
int orbm_optimize_essential_graph_split(orbm_matcher *m, const struct orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw,
                                        double *Scw_out, struct orbp_eg_stats *stats, double *split_ms, int32_t *split_count);

/* Host helpers: ComputeThreeMaxima (ind[3], -1 = none) and the histogram cull over match12.
 * orbm_rot_filter returns the number of matches left in match12 (>= 0), or ORBX_E_INVALID (negative) when the rotation
 * difference of a match falls off the histogram -- a NaN angle, or angles far outside [0, 360); the reference asserts
 * there.  match12 is then partly filtered and must not be used. */
int orbm_three_maxima(const int32_t *hist_sizes, int L, int32_t ind[3]);
int orbm_rot_filter(const float *angle_q, const float *angle_t, int32_t *match12, int nq);

const char *orbm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
