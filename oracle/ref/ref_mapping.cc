/*
 * ref_mapping.cc -- driver that runs the reference's own src/MapPoint.cc (compiled unmodified and in place behind the stand-in Map /
 * KeyFrame / Frame of mapping_standin.h) and, on real MapPoint objects from it, the reference's own Frame::isInFrustum,
 * KeyFrame::UnprojectStereo / ComputeSceneMedianDepth and LocalMapping::CreateNewMapPoints / ComputeF12 / SkewSymmetricMatrix, sliced
 * out of the reference at build time (oracle/_ref/*.inc), for tests/test_reference_pin_mapping_*.py.
 *
 *   ref_mapping REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable: it keeps the reference's code out of the test process.  Request and response are
 * the record files of ref_solver_io.h; tests/ref_mapping.py is the other end.  One program, three modes (record `mode`):
 *
 * mode 1, MapPoint::ComputeDistinctiveDescriptors for a batch of MapPoints
 *     off int32 [n+1], desc uint8 [total, 32]   point p is observed by off[p+1]-off[p] key frames, in this order, with these descriptors
 *     kfbad uint8 [total]                       KeyFrame::isBad() of each of them
 *     mpbad uint8 [n], init uint8 [n, 32]       the point's own mbBad, and its mDescriptor before the call
 *   -> desc uint8 [n, 32]                       mDescriptor after the call
 *   mObservations is a std::map<KeyFrame*, size_t>, iterated in pointer order: a point's key frames are the elements of ONE array, so
 *   pointer order is the request's order.  float Distances[N][N] (src/MapPoint.cc:275) lives on the stack: every point runs on a thread
 *   whose stack is sized from its N.
 *
 * mode 2, Frame::isInFrustum for the points of one frame
 *     view uint8 [sizeof orbm_frame_view], limit float32, xw / normal float32 [n, 3], mfmax / mfmin float32 [n]
 *   -> flag uint8 [n] (the returned bool), projx, projy, projxr, viewcos float32 [n], level int32 [n]: mTrackProjX, mTrackProjY,
 *      mTrackProjXR, mTrackViewCos, mnTrackScaleLevel of the points in view, zero elsewhere (the reference leaves them unset there)
 *   The raw members mfMaxDistance, mfMinDistance and mNormalVector are set through a probe subclass; GetMin / GetMaxDistanceInvariance
 *   and PredictScale(float, Frame*) are the reference's.
 *
 * mode 3, LocalMapping::CreateNewMapPoints with the pairs given
 *     mono int32                                mbMonocular
 *     cam1 uint8 [sizeof orbm_camera], kps1 uint8 [n1, 28], xy1 float32 [n1, 2], ur1 / dep1 float32 [n1]      the current key frame
 *     cams2 uint8 [nv, sizeof orbm_camera], off2 int32 [nv+1], kps2, xy2, ur2, dep2                            the neighbours, concatenated
 *     scene float32 [nv, 3], scnidx int32 [nv]  one MapPoint each neighbour already holds (ComputeSceneMedianDepth reads it), and its slot
 *     pairs int32 [n, 3]                        idx1, idx2 inside its view, view
 *   -> acc uint8 [n]  1: a MapPoint was made of the pair, 0: not, 2: the loop asked UnprojectStereo for a feature without depth (the
 *                     reference goes on with an empty matrix there; the driver leaves the call)
 *      path uint8 [n]                           1 / 2: the run called UnprojectStereo of the current key frame / of the neighbour, 0: of neither
 *      x3d float32 [n, 3]                       the new point's position (bits), zero elsewhere
 *      gate uint8 [nv], F12 float32 [nv, 9]     whether the neighbour passed :251-263, and the F12 the matcher was then handed
 *   The loop runs once per pair: the stand-in ORBmatcher::SearchForTriangulation hands that pair back for its view and nothing for
 *   the others, and the key frames' MapPoint slots are reset in between.  What the loop did is read where it calls the driver:
 *   SearchForTriangulation (a neighbour that passed the gates, with its F12) and Map::AddMapPoint (:448), by which time the new point
 *   holds its position and its two observations (the call-log trick of kfdb_standin.h).  CheckNewKeyFrames() returns false.
 *
 * mode 4, the whole loop (only in oracle/_ref/ref_newpoints, built with -DREF_REAL_MATCHER: the reference's src/ORBmatcher.cc is linked
 * unmodified and SearchForTriangulation, DescriptorDistance and the constructor are its own; that build has no mode 3)
 *     mode 3's records without pairs and scnidx, and desc1 / desc2 uint8 [n, 32], has1 / has2 uint8 [n] (the feature holds a MapPoint
 *     already: a real MapPoint, at `scene` for a neighbour's), the FeatureVectors fv1n / fv1o / fv1i and fv2v / fv2n / fv2o / fv2i as
 *     orbm_create_new_map_points takes them
 *   -> acc int32 [k, 3], x3d float32 [k, 3]     per new MapPoint in the order of Map::AddMapPoint: view, idx1, idx2 and the position
 *   The neighbours that pass :251-263 and their F12 are mode 3's record of the same key frames, asked without pairs.  A request on
 *   which the loop asks UnprojectStereo for a feature without depth is refused.
 */
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ORBmatcher.h"             // the reference's; with it the reference's MapPoint.h.  KeyFrame.h, Frame.h, Map.h are skipped
#include "ref_solver_io.h"

namespace ORB_SLAM2 {

#ifdef REF_LIBM_MATH
float cos(float x) { return ::cosf(x); }
float atan2(float y, float x) { return ::atan2f(y, x); }
float log(float x) { return ::logf(x); }
#else
float cos(float x) { return (float)::cosl((long double)x); }
float atan2(float y, float x) { return (float)::atan2l((long double)y, (long double)x); }
float log(float x) { return (float)::logl((long double)x); }
#endif

float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

/* stand-in LocalMapping: the members the three slices touch (include/LocalMapping.h:78-81, :104-110) */
class LocalMapping {
public:
    void CreateNewMapPoints();
    cv::Mat ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2);
    cv::Mat SkewSymmetricMatrix(const cv::Mat &v);
    bool CheckNewKeyFrames() { return false; }

    bool mbMonocular;
    Map *mpMap;
    KeyFrame *mpCurrentKeyFrame;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
};

#include "frame_frustum.inc"
#define UnprojectStereo UnprojectStereo_ref
#include "keyframe_stereo.inc"
#undef UnprojectStereo
#include "localmapping_newpoints.inc"
#ifndef REF_REAL_MATCHER
#include "matcher_distance.inc"
#endif

class ProbePoint : public MapPoint {
public:
    ProbePoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : MapPoint(Pos, pRefKF, pMap) {}
    void SetRaw(float mfMax, float mfMin, const float *normal)
    {
        mfMaxDistance = mfMax;
        mfMinDistance = mfMin;
        mNormalVector = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) mNormalVector.at<float>(k) = normal[k];
    }
    void SetBad(bool bad) { mbBad = bad; }
    void SetDescriptor(const cv::Mat &d) { mDescriptor = d.clone(); }
};

/* mode 3's record of one loop run */
struct NoDepth {};
static KeyFrame *g_kfs = 0;
static int g_nviews = 0;
static int g_pair[3];
static int g_accepted = 0;
static float g_x3d[3];
static std::vector<unsigned char> g_gate;
static std::vector<float> g_F12;

static int g_unprojected = 0;

void ref_mapping_unproject(KeyFrame *pKF, int i)
{
    g_unprojected = pKF == g_kfs ? 1 : 2;
    if (!(pKF->mvDepth[i] > 0)) throw NoDepth();
}

static bool g_loop = false;                      /* mode 4: every new point is appended to the log */
static std::vector<int32_t> g_log_pairs;
static std::vector<float> g_log_x3d;

void ref_mapping_new_point(MapPoint *pMP)
{
    std::map<KeyFrame *, size_t> obs = pMP->GetObservations();
    if (g_loop) {
        if (obs.size() != 2 || !obs.count(g_kfs)) refio::refuse("a new MapPoint does not hold two observations, one of the current key frame");
        for (std::map<KeyFrame *, size_t>::iterator it = obs.begin(); it != obs.end(); ++it)
            if (it->first != g_kfs) {
                g_log_pairs.push_back((int32_t)(it->first - g_kfs) - 1);
                g_log_pairs.push_back((int32_t)obs[g_kfs]);
                g_log_pairs.push_back((int32_t)it->second);
            }
        cv::Mat Q = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) g_log_x3d.push_back(Q.at<float>(k));
        return;
    }
    KeyFrame *kf2 = g_kfs + 1 + g_pair[2];
    if (obs.size() != 2 || !obs.count(g_kfs) || !obs.count(kf2) || (int)obs[g_kfs] != g_pair[0] || (int)obs[kf2] != g_pair[1])
        refio::refuse("a new MapPoint does not hold the pair it was made of");
    cv::Mat P = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) g_x3d[k] = P.at<float>(k);
    g_accepted++;
}

#ifdef REF_REAL_MATCHER
/* src/ORBmatcher.cc is linked whole; CreateNewMapPoints reaches none of these (mapping_standin.h) */
std::set<MapPoint *> KeyFrame::GetMapPoints() { refio::refuse("KeyFrame::GetMapPoints is not part of this driver"); }
bool KeyFrame::IsInImage(const float &, const float &) const { refio::refuse("KeyFrame::IsInImage is not part of this driver"); }
std::vector<size_t> KeyFrame::GetFeaturesInArea(const float &, const float &, const float &) const { refio::refuse("KeyFrame::GetFeaturesInArea is not part of this driver"); }
std::vector<size_t> Frame::GetFeaturesInArea(const float &, const float &, const float &, const int, const int) const { refio::refuse("Frame::GetFeaturesInArea is not part of this driver"); }
#else
ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

/* stand-in: hands back the pair of the current run for its view */
int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, std::vector<pair<size_t, size_t> > &vMatchedPairs, const bool)
{
    int view = (int)(pKF2 - g_kfs) - 1;
    if (pKF1 != g_kfs || view < 0 || view >= g_nviews) refio::refuse("SearchForTriangulation on an unknown key frame");
    g_gate[view] = 1;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) g_F12[view * 9 + r * 3 + c] = F12.at<float>(r, c);
    vMatchedPairs.clear();
    if (g_pair[2] == view) vMatchedPairs.push_back(make_pair((size_t)g_pair[0], (size_t)g_pair[1]));
    return (int)vMatchedPairs.size();
}
#endif

}  // namespace ORB_SLAM2

using namespace ORB_SLAM2;

/* the layouts of include/orbm.h: orbm_frame_view, orbm_camera, orbx_keypoint */
struct View {
    float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, mbf, bounds[4], log_scale_factor;
    int32_t nlevels;
    float scale_factors[16];
};
struct Camera {
    float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factor;
    int32_t nlevels;
    float scale_factors[16], level_sigma2[16];
};
struct Kp {
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

static cv::Mat mat_of(int rows, int cols, const float *v)
{
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.at<float>(r, c) = v[r * cols + c];
    return m;
}

/* ---- mode 1 */

struct DdJob {
    ProbePoint *p;
};
static void *dd_thread(void *arg)
{
    ((DdJob *)arg)->p->ComputeDistinctiveDescriptors();
    return 0;
}

static void run_distinctive(const refio::Request &rq, refio::Response &rs)
{
    const refio::Record &off_r = rq.get("off", refio::I32, 1, -1);
    const int n = off_r.cols - 1;
    const int32_t *off = off_r.as<int32_t>(refio::I32);
    if (n < 0 || off[0] != 0) refio::refuse("bad off");
    const int total = off[n];
    const unsigned char *desc = rq.get("desc", refio::U8, total, 32).as<unsigned char>(refio::U8);
    const unsigned char *kfbad = rq.get("kfbad", refio::U8, 1, total).as<unsigned char>(refio::U8);
    const unsigned char *mpbad = rq.get("mpbad", refio::U8, 1, n).as<unsigned char>(refio::U8);
    const unsigned char *init = rq.get("init", refio::U8, n, 32).as<unsigned char>(refio::U8);
    std::vector<unsigned char> out((size_t)n * 32 + 1);
    Map map;
    float zero[3] = {0, 0, 0};
    for (int p = 0; p < n; p++) {
        const int cnt = off[p + 1] - off[p];
        if (cnt < 0) refio::refuse("bad off");
        KeyFrame *kfs = new KeyFrame[cnt + 1];              /* one array: pointer order is the request's order */
        for (int j = 0; j < cnt; j++) {
            kfs[j].mnId = j;
            kfs[j].N = 1;
            kfs[j].mvuRight.assign(1, -1.0f);
            kfs[j].mvpMapPoints.assign(1, (MapPoint *)0);
            kfs[j].mbBad = kfbad[off[p] + j] != 0;
            kfs[j].mDescriptors.create(1, 32, CV_8UC1);
            std::memcpy(kfs[j].mDescriptors.ptr(0), desc + (size_t)(off[p] + j) * 32, 32);
        }
        ProbePoint *mp = new ProbePoint(mat_of(3, 1, zero), &kfs[cnt], &map);
        for (int j = 0; j < cnt; j++) mp->AddObservation(&kfs[j], 0);
        cv::Mat d0(1, 32, CV_8UC1);
        std::memcpy(d0.ptr(0), init + (size_t)p * 32, 32);
        mp->SetDescriptor(d0);
        mp->SetBad(mpbad[p] != 0);
        DdJob job = {mp};
        pthread_attr_t attr;
        pthread_t th;
        pthread_attr_init(&attr);
        pthread_attr_setstacksize(&attr, (size_t)cnt * cnt * sizeof(float) + (size_t)cnt * 64 + (8u << 20));
        if (pthread_create(&th, &attr, dd_thread, &job) != 0) refio::refuse("cannot start the thread of a point");
        pthread_join(th, 0);
        pthread_attr_destroy(&attr);
        cv::Mat d = mp->GetDescriptor();
        if (d.rows != 1 || d.cols != 32) refio::refuse("mDescriptor is not one row of 32 bytes");
        std::memcpy(out.data() + (size_t)p * 32, d.ptr(0), 32);
        delete mp;
        delete[] kfs;
    }
    rs.put("desc", refio::U8, n, 32, out.data());
}

/* ---- mode 2 */

static void run_frustum(const refio::Request &rq, refio::Response &rs)
{
    const View *V = (const View *)rq.get("view", refio::U8, 1, (int)sizeof(View)).as<unsigned char>(refio::U8);
    const float limit = *rq.get("limit", refio::F32, 1, 1).as<float>(refio::F32);
    const refio::Record &xw_r = rq.get("xw", refio::F32, -1, 3);
    const int n = xw_r.rows;
    const float *xw = xw_r.as<float>(refio::F32);
    const float *normal = rq.get("normal", refio::F32, n, 3).as<float>(refio::F32);
    const float *mfmax = rq.get("mfmax", refio::F32, 1, n).as<float>(refio::F32);
    const float *mfmin = rq.get("mfmin", refio::F32, 1, n).as<float>(refio::F32);
    if (V->nlevels < 1 || V->nlevels > 16) refio::refuse("bad nlevels");

    Frame F;
    Frame::fx = V->fx;
    Frame::fy = V->fy;
    Frame::cx = V->cx;
    Frame::cy = V->cy;
    Frame::mnMinX = V->bounds[0];
    Frame::mnMaxX = V->bounds[1];
    Frame::mnMinY = V->bounds[2];
    Frame::mnMaxY = V->bounds[3];
    F.mbf = V->mbf;
    F.mnScaleLevels = V->nlevels;
    F.mfLogScaleFactor = V->log_scale_factor;
    F.mvScaleFactors.assign(V->scale_factors, V->scale_factors + V->nlevels);
    F.mRcw = mat_of(3, 3, V->Rcw);
    F.mtcw = mat_of(3, 1, V->tcw);
    F.mOw = mat_of(3, 1, V->Ow);

    Map map;
    KeyFrame kf;
    std::vector<unsigned char> flag(n + 1);
    std::vector<float> px(n + 1), py(n + 1), pr(n + 1), vc(n + 1);
    std::vector<int32_t> lv(n + 1);
    for (int i = 0; i < n; i++) {
        ProbePoint mp(mat_of(3, 1, xw + 3 * i), &kf, &map);
        mp.SetRaw(mfmax[i], mfmin[i], normal + 3 * i);
        const bool in = F.isInFrustum(&mp, limit);
        if (in != mp.mbTrackInView) refio::refuse("isInFrustum's result and mbTrackInView disagree");
        flag[i] = in ? 1 : 0;
        if (in) {
            px[i] = mp.mTrackProjX;
            py[i] = mp.mTrackProjY;
            pr[i] = mp.mTrackProjXR;
            vc[i] = mp.mTrackViewCos;
            lv[i] = mp.mnTrackScaleLevel;
        }
    }
    rs.put("flag", refio::U8, 1, n, flag.data());
    rs.put("projx", refio::F32, 1, n, px.data());
    rs.put("projy", refio::F32, 1, n, py.data());
    rs.put("projxr", refio::F32, 1, n, pr.data());
    rs.put("viewcos", refio::F32, 1, n, vc.data());
    rs.put("level", refio::I32, 1, n, lv.data());
}

/* ---- mode 3 */

static void fill_keyframe(KeyFrame &kf, int id, const Camera &C, const Kp *kps, const float *xy, const float *ur, const float *dep, int n)
{
    if (C.nlevels < 1 || C.nlevels > 16) refio::refuse("bad nlevels");
    kf.mnId = kf.mnFrameId = id;
    kf.fx = C.fx;
    kf.fy = C.fy;
    kf.cx = C.cx;
    kf.cy = C.cy;
    kf.invfx = C.invfx;
    kf.invfy = C.invfy;
    kf.mbf = C.mbf;
    kf.mb = C.mb;
    kf.N = n;
    kf.mnScaleLevels = C.nlevels;
    kf.mfScaleFactor = C.scale_factor;
    kf.mfLogScaleFactor = ORB_SLAM2::log(C.scale_factor);
    kf.mvScaleFactors.assign(C.scale_factors, C.scale_factors + C.nlevels);
    kf.mvLevelSigma2.assign(C.level_sigma2, C.level_sigma2 + C.nlevels);
    kf.mvInvLevelSigma2.resize(C.nlevels);
    for (int l = 0; l < C.nlevels; l++) kf.mvInvLevelSigma2[l] = 1.0f / C.level_sigma2[l];
    const float K[9] = {C.fx, 0, C.cx, 0, C.fy, C.cy, 0, 0, 1};
    kf.mK = mat_of(3, 3, K);
    float T[16] = {0}, W[16] = {0};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            T[r * 4 + c] = C.Rcw[r * 3 + c];
            W[r * 4 + c] = C.Rcw[c * 3 + r];
        }
        T[r * 4 + 3] = C.tcw[r];
        W[r * 4 + 3] = C.Ow[r];
    }
    T[15] = W[15] = 1;
    kf.Tcw = mat_of(4, 4, T);
    kf.Twc = mat_of(4, 4, W);
    kf.Ow = mat_of(3, 1, C.Ow);
    kf.mvKeys.resize(n);
    kf.mvKeysUn.resize(n);
    for (int i = 0; i < n; i++) {
        if (kps[i].octave < 0 || kps[i].octave >= C.nlevels) refio::refuse("an octave outside the pyramid");
        kf.mvKeysUn[i] = cv::KeyPoint(kps[i].x, kps[i].y, kps[i].size, kps[i].angle, kps[i].response, kps[i].octave, kps[i].class_id);
        kf.mvKeys[i] = kf.mvKeysUn[i];
        kf.mvKeys[i].pt.x = xy[2 * i];
        kf.mvKeys[i].pt.y = xy[2 * i + 1];
    }
    kf.mvuRight.assign(ur, ur + n);
    kf.mvDepth.assign(dep, dep + n);
    kf.mDescriptors.create(n > 0 ? n : 1, 32, CV_8UC1);
    for (int i = 0; i < kf.mDescriptors.rows; i++) std::memset(kf.mDescriptors.ptr(i), 0, 32);
    kf.mvpMapPoints.assign(n, (MapPoint *)0);
}

#ifndef REF_REAL_MATCHER
static void run_newpoints(const refio::Request &rq, refio::Response &rs)
{
    const int mono = *rq.get("mono", refio::I32, 1, 1).as<int32_t>(refio::I32);
    const Camera *C1 = (const Camera *)rq.get("cam1", refio::U8, 1, (int)sizeof(Camera)).as<unsigned char>(refio::U8);
    const refio::Record &k1 = rq.get("kps1", refio::U8, -1, (int)sizeof(Kp));
    const int n1 = k1.rows;
    const refio::Record &c2 = rq.get("cams2", refio::U8, -1, (int)sizeof(Camera));
    const int nv = c2.rows;
    const Camera *C2 = (const Camera *)c2.as<unsigned char>(refio::U8);
    const int32_t *off2 = rq.get("off2", refio::I32, 1, nv + 1).as<int32_t>(refio::I32);
    const int n2 = off2[nv];
    const Kp *kps2 = (const Kp *)rq.get("kps2", refio::U8, n2, (int)sizeof(Kp)).as<unsigned char>(refio::U8);
    const float *xy2 = rq.get("xy2", refio::F32, n2, 2).as<float>(refio::F32);
    const float *ur2 = rq.get("ur2", refio::F32, 1, n2).as<float>(refio::F32);
    const float *dep2 = rq.get("dep2", refio::F32, 1, n2).as<float>(refio::F32);
    const float *scene = rq.get("scene", refio::F32, nv, 3).as<float>(refio::F32);
    const int32_t *scnidx = rq.get("scnidx", refio::I32, 1, nv).as<int32_t>(refio::I32);
    const refio::Record &pr = rq.get("pairs", refio::I32, -1, 3);
    const int n = pr.rows;
    const int32_t *pairs = pr.as<int32_t>(refio::I32);

    g_kfs = new KeyFrame[nv + 1];                           /* one array: the current key frame, then the neighbours */
    g_nviews = nv;
    fill_keyframe(g_kfs[0], 0, *C1, (const Kp *)k1.as<unsigned char>(refio::U8), rq.get("xy1", refio::F32, n1, 2).as<float>(refio::F32),
                  rq.get("ur1", refio::F32, 1, n1).as<float>(refio::F32), rq.get("dep1", refio::F32, 1, n1).as<float>(refio::F32), n1);
    Map map;
    std::vector<MapPoint *> scene_points(nv);
    for (int v = 0; v < nv; v++) {
        if (off2[v] < 0 || off2[v + 1] < off2[v]) refio::refuse("bad off2");
        const int nf = off2[v + 1] - off2[v];
        fill_keyframe(g_kfs[1 + v], 1 + v, C2[v], kps2 + off2[v], xy2 + 2 * off2[v], ur2 + off2[v], dep2 + off2[v], nf);
        if (scnidx[v] < 0 || scnidx[v] >= nf) refio::refuse("a scene point outside its key frame");
        scene_points[v] = new MapPoint(mat_of(3, 1, scene + 3 * v), &g_kfs[1 + v], &map);
        g_kfs[0].mvpNeighbours.push_back(&g_kfs[1 + v]);
    }

    LocalMapping lm;
    lm.mbMonocular = mono != 0;
    lm.mpMap = &map;
    lm.mpCurrentKeyFrame = &g_kfs[0];
    g_gate.assign(nv + 1, 0);
    g_F12.assign((size_t)nv * 9 + 1, 0.0f);
    std::vector<unsigned char> acc(n + 1), path(n + 1);
    std::vector<float> x3d((size_t)n * 3 + 1);
    for (int i = 0; i <= n; i++) {                          /* the last run has no pair: the gates and F12 of a call without matches */
        const int none[3] = {-1, -1, -1};
        std::memcpy(g_pair, i < n ? pairs + 3 * i : none, sizeof g_pair);
        if (i < n) {
            const int v = g_pair[2];
            if (v < 0 || v >= nv || g_pair[0] < 0 || g_pair[0] >= n1 || g_pair[1] < 0 || g_pair[1] >= off2[v + 1] - off2[v]) refio::refuse("a pair outside its key frames");
        }
        g_kfs[0].mvpMapPoints.assign(n1, (MapPoint *)0);
        for (int v = 0; v < nv; v++) {
            g_kfs[1 + v].mvpMapPoints.assign(off2[v + 1] - off2[v], (MapPoint *)0);
            g_kfs[1 + v].mvpMapPoints[scnidx[v]] = scene_points[v];
        }
        g_accepted = g_unprojected = 0;
        g_x3d[0] = g_x3d[1] = g_x3d[2] = 0;
        bool no_depth = false;
        try {
            lm.CreateNewMapPoints();
        } catch (const NoDepth &) {
            no_depth = true;
        }
        if (i == n) break;
        if (g_accepted > 1 || (no_depth && g_accepted)) refio::refuse("one pair made more than one MapPoint");
        acc[i] = no_depth ? 2 : g_accepted;
        path[i] = g_unprojected;
        std::memcpy(&x3d[3 * i], g_x3d, sizeof g_x3d);
    }
    rs.put("acc", refio::U8, 1, n, acc.data());
    rs.put("path", refio::U8, 1, n, path.data());
    rs.put("x3d", refio::F32, n, 3, x3d.data());
    rs.put("gate", refio::U8, 1, nv, g_gate.data());
    rs.put("F12", refio::F32, nv, 9, g_F12.data());
}

#endif

#ifdef REF_REAL_MATCHER
/* ---- mode 4: the whole loop, with the reference's own ORBmatcher::SearchForTriangulation */

static void fill_features(KeyFrame &kf, const unsigned char *desc, const unsigned char *has, int n, const int32_t *node, const int32_t *off,
                          const int32_t *idx, int nnodes, const float *pos, Map *map, std::vector<MapPoint *> &keep)
{
    for (int i = 0; i < n; i++) {
        std::memcpy(kf.mDescriptors.ptr(i), desc + (size_t)i * 32, 32);
        if (has[i]) {
            kf.mvpMapPoints[i] = new MapPoint(mat_of(3, 1, pos), &kf, map);
            keep.push_back(kf.mvpMapPoints[i]);
        }
    }
    for (int k = 0; k < nnodes; k++)
        for (int j = off[k]; j < off[k + 1]; j++) {
            if (idx[j] < 0 || idx[j] >= n) refio::refuse("a FeatureVector index outside its key frame");
            kf.mFeatVec.addFeature((DBoW2::NodeId)node[k], (unsigned int)idx[j]);
        }
}

static void run_loop(const refio::Request &rq, refio::Response &rs)
{
    const int mono = *rq.get("mono", refio::I32, 1, 1).as<int32_t>(refio::I32);
    const Camera *C1 = (const Camera *)rq.get("cam1", refio::U8, 1, (int)sizeof(Camera)).as<unsigned char>(refio::U8);
    const refio::Record &k1 = rq.get("kps1", refio::U8, -1, (int)sizeof(Kp));
    const int n1 = k1.rows;
    const refio::Record &c2 = rq.get("cams2", refio::U8, -1, (int)sizeof(Camera));
    const int nv = c2.rows;
    const Camera *C2 = (const Camera *)c2.as<unsigned char>(refio::U8);
    const int32_t *off2 = rq.get("off2", refio::I32, 1, nv + 1).as<int32_t>(refio::I32);
    const int n2 = off2[nv];
    const Kp *kps2 = (const Kp *)rq.get("kps2", refio::U8, n2, (int)sizeof(Kp)).as<unsigned char>(refio::U8);
    const float *xy2 = rq.get("xy2", refio::F32, n2, 2).as<float>(refio::F32);
    const float *ur2 = rq.get("ur2", refio::F32, 1, n2).as<float>(refio::F32);
    const float *dep2 = rq.get("dep2", refio::F32, 1, n2).as<float>(refio::F32);
    const float *scene = rq.get("scene", refio::F32, nv, 3).as<float>(refio::F32);
    const unsigned char *desc1 = rq.get("desc1", refio::U8, n1, 32).as<unsigned char>(refio::U8);
    const unsigned char *desc2 = rq.get("desc2", refio::U8, n2, 32).as<unsigned char>(refio::U8);
    const unsigned char *has1 = rq.get("has1", refio::U8, 1, n1).as<unsigned char>(refio::U8);
    const unsigned char *has2 = rq.get("has2", refio::U8, 1, n2).as<unsigned char>(refio::U8);
    const refio::Record &f1n = rq.get("fv1n", refio::I32, 1, -1);
    const int32_t *fv1o = rq.get("fv1o", refio::I32, 1, f1n.cols + 1).as<int32_t>(refio::I32);
    const int32_t *fv1i = rq.get("fv1i", refio::I32, 1, fv1o[f1n.cols]).as<int32_t>(refio::I32);
    const int32_t *fvv = rq.get("fv2v", refio::I32, 1, nv + 1).as<int32_t>(refio::I32);
    const int32_t *fv2n = rq.get("fv2n", refio::I32, 1, fvv[nv]).as<int32_t>(refio::I32);
    const int32_t *fv2o = rq.get("fv2o", refio::I32, 1, fvv[nv] + 1).as<int32_t>(refio::I32);
    const int32_t *fv2i = rq.get("fv2i", refio::I32, 1, fv2o[fvv[nv]]).as<int32_t>(refio::I32);

    g_kfs = new KeyFrame[nv + 1];
    g_nviews = nv;
    Map map;
    std::vector<MapPoint *> keep;
    const float origin[3] = {0, 0, 0};
    fill_keyframe(g_kfs[0], 0, *C1, (const Kp *)k1.as<unsigned char>(refio::U8), rq.get("xy1", refio::F32, n1, 2).as<float>(refio::F32),
                  rq.get("ur1", refio::F32, 1, n1).as<float>(refio::F32), rq.get("dep1", refio::F32, 1, n1).as<float>(refio::F32), n1);
    fill_features(g_kfs[0], desc1, has1, n1, f1n.as<int32_t>(refio::I32), fv1o, fv1i, f1n.cols, origin, &map, keep);
    for (int v = 0; v < nv; v++) {
        const int nf = off2[v + 1] - off2[v];
        fill_keyframe(g_kfs[1 + v], 1 + v, C2[v], kps2 + off2[v], xy2 + 2 * off2[v], ur2 + off2[v], dep2 + off2[v], nf);
        fill_features(g_kfs[1 + v], desc2 + (size_t)off2[v] * 32, has2 + off2[v], nf, fv2n + fvv[v], fv2o + fvv[v], fv2i, fvv[v + 1] - fvv[v],
                      scene + 3 * v, &map, keep);
        bool any = false;
        for (int i = 0; i < nf; i++) any = any || has2[off2[v] + i];
        if (mono && !any) refio::refuse("a neighbour without MapPoints has no median depth");
        g_kfs[0].mvpNeighbours.push_back(&g_kfs[1 + v]);
    }
    LocalMapping lm;
    lm.mbMonocular = mono != 0;
    lm.mpMap = &map;
    lm.mpCurrentKeyFrame = &g_kfs[0];
    g_loop = true;
    try {
        lm.CreateNewMapPoints();
    } catch (const NoDepth &) {
        refio::refuse("the loop asked UnprojectStereo for a feature without depth: the request is outside the reference's defined behaviour");
    }
    /* the gates and F12 of the same key frames are what mode 3 of ref_mapping records for a request without pairs */
    const int k = (int)g_log_pairs.size() / 3;
    g_log_pairs.push_back(0);
    g_log_x3d.push_back(0);
    rs.put("acc", refio::I32, k, 3, g_log_pairs.data());
    rs.put("x3d", refio::F32, k, 3, g_log_x3d.data());
}
#endif

int main(int argc, char **argv)
{
    refio::g_name = "ref_mapping";
    if (argc != 3) refio::refuse("usage: ref_mapping REQUEST RESPONSE");
    refio::Request rq(argv[1]);
    refio::Response rs(argv[2]);
    const int mode = *rq.get("mode", refio::I32, 1, 1).as<int32_t>(refio::I32);
    if (mode == 1) run_distinctive(rq, rs);
    else if (mode == 2) run_frustum(rq, rs);
#ifndef REF_REAL_MATCHER
    else if (mode == 3) run_newpoints(rq, rs);
#else
    else if (mode == 4) run_loop(rq, rs);
#endif
    else refio::refuse("unknown mode");
    rs.close();
    return 0;
}
