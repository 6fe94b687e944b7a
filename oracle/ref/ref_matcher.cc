/*
 * ref_matcher.cc -- driver of the reference's own src/ORBmatcher.cc (compiled unmodified and in place behind matcher_standin.h):
 *     ref_matcher REQUEST RESPONSE
 * TEST INFRASTRUCTURE ONLY.  tests/ref_matcher.py is the other end.  Request and response are record files (ref_solver_io.h).
 *
 * One request holds one call.  "kind" names the function (the K_* list below); the other records are the arrays that the function of
 * the same name in tests/oracle_lib.py takes, flat, under the tags the loaders below read:
 *     a MapPoint list, suffix s     use<s> xw<s> nrm<s> mind<s> maxd<s> mfmax<s> mpdesc<s> mpobs<s>
 *     a Frame / KeyFrame, suffix s  kx<s> ky<s> ka<s> ko<s> desc<s> ur<s> bnd<s> (mnMinX, mnMaxX, mnMinY, mnMaxY) grid<s> (the six numbers
 *                                   of oracle_lib.KeyFrameGrid) sf<s> sg2<s> isg2<s> fvn<s> fvo<s> fvi<s> (FeatureVector: nodes, offsets,
 *                                   indices) T<s> (4 x 4) val<s> / has<s> (per-feature flags)
 *     scalars                       fpar (floats), ipar (ints), in the order each handler states
 * A usable flag of 0 stands for the object predicate at the head of the loop body: the driver makes that MapPoint bad (or leaves the
 * slot NULL where the reference tests the pointer), so the reference's own `continue` is taken.
 *
 * What a request cannot say is refused (exit status 2), never answered: a key-frame window origin that differs from the image bounds
 * (the reference has one mnMinX for both, include/KeyFrame.h:185), scale tables of other than the stated levels.
 *
 * The grid.  Frame's static bounds and cell sizes are set from the request (mfGridElementWidthInv as src/Frame.cc:100-101 computes
 * it: static_cast<float>(FRAME_GRID_COLS)/static_cast<float>(mnMaxX-mnMinX)), the cells are filled by the reference's own
 * Frame::AssignFeaturesToGrid, and a key frame's mGrid is the copy src/KeyFrame.cc:46-52 makes of it.
 *
 * Response: "ret" (the return value), the function's tables (each handler states them) and "log", the call log of the stand-ins as
 * rows of (call, MapPoint id, argument).
 */
#include <memory>

#include "ORBmatcher.h"
#include "ref_solver_io.h"

/* the reference's own text, sliced at build time (oracle/ref/Makefile); four members under another name, see matcher_standin.h */
namespace ORB_SLAM2 {
#define GetFeaturesInArea GetFeaturesInArea_ref
#define IsInImage IsInImage_ref
#define PredictScale PredictScale_ref
#include "frame_grid.inc"
#include "keyframe_area.inc"
#include "mappoint_scale.inc"
#undef GetFeaturesInArea
#undef IsInImage
#undef PredictScale

float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
}

using namespace ORB_SLAM2;
using refio::F32;
using refio::I32;
using refio::U8;

enum { K_PROJ_MAP = 0, K_PROJ_LAST, K_PROJ_KF, K_PROJ_SIM3, K_BOW, K_BOW_KF, K_INIT, K_TRIANG, K_FUSE, K_FUSE_SIM3, K_SIM3 };

static const refio::Request *g_req;
static const float kNoGrid[6] = {0, 0, 1, 1, 0, 0}, kNoBounds[4] = {0, 1, 0, 1};      /* of a key frame whose grid the call does not read */
static std::vector<std::unique_ptr<MapPoint> > g_pool;

static std::string tag(const char *name, const char *s) { return std::string(name) + s; }
static const float *f32(const std::string &t, int rows, int cols) { return g_req->get(t.c_str(), F32, rows, cols).as<float>(F32); }
static const int32_t *i32(const std::string &t, int rows, int cols) { return g_req->get(t.c_str(), I32, rows, cols).as<int32_t>(I32); }
static const unsigned char *u8(const std::string &t, int rows, int cols) { return g_req->get(t.c_str(), U8, rows, cols).as<unsigned char>(U8); }
static int count(const std::string &t) { return (int)g_req->get(t.c_str()).count(); }

static cv::Mat mat(const float *p, int r, int c)
{
    cv::Mat m(r, c, CV_32F);
    for (int y = 0; y < r; y++)
        for (int x = 0; x < c; x++) m.at<float>(y, x) = p[y * c + x];
    return m;
}

static cv::Mat bytes(const unsigned char *p, int r, int c)
{
    cv::Mat m(std::max(r, 1), c, CV_8U);
    for (int y = 0; y < r; y++) std::memcpy(m.ptr(y), p + (size_t)y * c, c);
    return m;
}

static MapPoint *new_point(int id)
{
    g_pool.push_back(std::unique_ptr<MapPoint>(new MapPoint(id)));
    return g_pool.back().get();
}

/* the MapPoint list of suffix s; `projected`: with world position and the fields of the projection block */
static std::vector<MapPoint *> points(const char *s, bool projected, bool with_normal)
{
    const int n = count(tag("mpdesc", s)) / 32;
    const unsigned char *d = u8(tag("mpdesc", s), n, 32);
    const int32_t *obs = g_req->has(tag("mpobs", s).c_str()) ? i32(tag("mpobs", s), 1, n) : 0;
    std::vector<MapPoint *> v(n);
    for (int i = 0; i < n; i++) {
        MapPoint *p = v[i] = new_point(i);
        p->mDescriptor = bytes(d + (size_t)i * 32, 1, 32);
        p->nObs = obs ? obs[i] : 1;
    }
    if (projected) {
        const float *xw = f32(tag("xw", s), n, 3);
        for (int i = 0; i < n; i++) v[i]->mWorldPos = mat(xw + 3 * i, 3, 1);
        if (g_req->has(tag("mfmax", s).c_str())) {
            const float *mn = f32(tag("mind", s), 1, n), *mx = f32(tag("maxd", s), 1, n), *mf = f32(tag("mfmax", s), 1, n);
            for (int i = 0; i < n; i++) {
                v[i]->mfMinDistanceInvariance = mn[i];
                v[i]->mfMaxDistanceInvariance = mx[i];
                v[i]->mfMaxDistance = mf[i];
            }
        }
        if (with_normal) {
            const float *nr = f32(tag("nrm", s), n, 3);
            for (int i = 0; i < n; i++) v[i]->mNormalVector = mat(nr + 3 * i, 3, 1);
        }
    }
    return v;
}

static std::vector<cv::KeyPoint> keys(const char *s)
{
    const int n = count(tag("kx", s));
    const float *x = f32(tag("kx", s), 1, n), *y = f32(tag("ky", s), 1, n), *a = f32(tag("ka", s), 1, n);
    const int32_t *o = i32(tag("ko", s), 1, n);
    std::vector<cv::KeyPoint> k(n);
    for (int i = 0; i < n; i++) k[i] = cv::KeyPoint(x[i], y[i], 31.0f, a[i], 0.0f, o[i], -1);
    return k;
}

static std::vector<float> floats(const std::string &t)
{
    const int n = count(t);
    const float *p = f32(t, 1, n);
    return std::vector<float>(p, p + n);
}

static DBoW2::FeatureVector featvec(const char *s)
{
    const int nn = count(tag("fvn", s));
    const int32_t *node = i32(tag("fvn", s), 1, nn), *off = i32(tag("fvo", s), 1, nn + 1);
    const int32_t *idx = i32(tag("fvi", s), 1, -1);
    DBoW2::FeatureVector fv;
    for (int k = 0; k < nn; k++)
        for (int j = off[k]; j < off[k + 1]; j++) fv.addFeature((DBoW2::NodeId)node[k], (unsigned int)idx[j]);
    return fv;
}

/* a Frame of suffix s with its grid; bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).  `inv` (optional) gives the cell sizes themselves. */
static void fill_frame(Frame &F, const char *s, const float bounds[4], const float *inv)
{
    F.mvKeysUn = keys(s);
    F.mvKeys = F.mvKeysUn;
    F.N = (int)F.mvKeysUn.size();
    F.mDescriptors = bytes(u8(tag("desc", s), F.N, 32), F.N, 32);
    F.mvuRight = g_req->has(tag("ur", s).c_str()) ? floats(tag("ur", s)) : std::vector<float>(F.N, -1.0f);
    if ((int)F.mvuRight.size() != F.N) refio::refuse("ur has another length than the key points");
    F.mvpMapPoints.assign(F.N, (MapPoint *)0);
    F.mvbOutlier.assign(F.N, false);
    Frame::mnMinX = bounds[0];
    Frame::mnMaxX = bounds[1];
    Frame::mnMinY = bounds[2];
    Frame::mnMaxY = bounds[3];
    Frame::mfGridElementWidthInv = inv ? inv[0] : static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(Frame::mnMaxX - Frame::mnMinX);
    Frame::mfGridElementHeightInv = inv ? inv[1] : static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(Frame::mnMaxY - Frame::mnMinY);
    F.AssignFeaturesToGrid();
}

static void frame_scales(Frame &F, const char *s, float logsf)
{
    F.mvScaleFactors = floats(tag("sf", s));
    F.mnScaleLevels = (int)F.mvScaleFactors.size();
    F.mfLogScaleFactor = logsf;
}

/* a KeyFrame of suffix s: grid<s> = (assign_min_x, assign_min_y, inv_w, inv_h, query_min_x, query_min_y), bnd<s> its int bounds */
static KeyFrame *key_frame(const char *s, const float K[4], float bf, float logsf, bool with_grid)
{
    static std::vector<std::unique_ptr<KeyFrame> > pool;
    const int n = count(tag("kx", s));
    std::vector<float> sf = floats(tag("sf", s));
    float grid[6] = {0, 0, 1, 1, 0, 0}, bounds[4] = {0, 1, 0, 1};
    if (with_grid) {
        std::memcpy(grid, f32(tag("grid", s), 1, 6), sizeof grid);
        std::memcpy(bounds, f32(tag("bnd", s), 1, 4), sizeof bounds);
        for (int k = 0; k < 4; k++)
            if (bounds[k] != (float)(int)bounds[k]) refio::refuse("a key frame's bounds are ints (include/KeyFrame.h:185-188)");
        if (grid[4] != bounds[0] || grid[5] != bounds[2]) refio::refuse("a key frame has one mnMinX / mnMinY for IsInImage and GetFeaturesInArea");
    }
    KeyFrame *kf = new KeyFrame(n, K[0], K[1], K[2], K[3], bf, grid, bounds, (int)sf.size(), logsf);
    pool.push_back(std::unique_ptr<KeyFrame>(kf));
    kf->mvScaleFactors = sf;
    kf->mvKeysUn = keys(s);
    kf->mDescriptors = bytes(u8(tag("desc", s), n, 32), n, 32);
    kf->mvuRight = g_req->has(tag("ur", s).c_str()) ? floats(tag("ur", s)) : std::vector<float>(n, -1.0f);
    if ((int)kf->mvuRight.size() != n) refio::refuse("ur has another length than the key points");
    if (with_grid) {
        Frame F;                                            /* the frame that became the key frame */
        const float fb[4] = {grid[0], 0, grid[1], 0};
        fill_frame(F, s, fb, grid + 2);
        kf->mGrid.resize(kf->mnGridCols);                   /* src/KeyFrame.cc:46-52 */
        for (int i = 0; i < kf->mnGridCols; i++) {
            kf->mGrid[i].resize(kf->mnGridRows);
            for (int j = 0; j < kf->mnGridRows; j++) kf->mGrid[i][j] = F.mGrid[i][j];
        }
    }
    return kf;
}

static void set_pose(KeyFrame *kf, const float *T, const float *Ow)
{
    cv::Mat Tcw = mat(T, 4, 4);
    kf->Rcw = Tcw.rowRange(0, 3).colRange(0, 3).clone();
    kf->tcw = Tcw.rowRange(0, 3).col(3).clone();
    if (Ow) kf->Ow = mat(Ow, 3, 1);
}

static void put_ints(refio::Response &out, const char *t, const std::vector<int32_t> &v)
{
    int32_t none = 0;
    out.put(t, I32, 1, (int)v.size(), v.empty() ? &none : v.data());
}

/* what the slots of a frame hold after the call: the request MapPoint's id or -1, and its Observations() or -1 for a NULL slot */
static void put_slots(refio::Response &out, const std::vector<MapPoint *> &slots)
{
    std::vector<int32_t> id(slots.size(), -1), obs(slots.size(), -1);
    for (size_t i = 0; i < slots.size(); i++)
        if (slots[i]) {
            id[i] = slots[i]->id;
            obs[i] = slots[i]->nObs;
        }
    put_ints(out, "slot", id);
    put_ints(out, "slotobs", obs);
}

/* holders of ids < 0 for the slots of a frame that are taken before the call: obs[i] >= 0 is the holder's Observations() */
static void take_slots(std::vector<MapPoint *> &slots, const int32_t *obs)
{
    for (size_t i = 0; i < slots.size(); i++)
        if (obs[i] >= 0) {
            slots[i] = new_point(-2 - (int)i);
            slots[i]->nObs = obs[i];
        }
}

int main(int argc, char **argv)
{
    refio::g_name = "ref_matcher";
    if (argc != 3) refio::refuse("usage: ref_matcher REQUEST RESPONSE");
    refio::Request req(argv[1]);
    g_req = &req;
    refio::Response out(argv[2]);
    const int kind = i32("kind", 1, 1)[0];
    const int32_t *ip = req.has("ipar") ? req.get("ipar").as<int32_t>(I32) : 0;
    const float *fp = req.has("fpar") ? req.get("fpar").as<float>(F32) : 0;
    const int nip = ip ? count("ipar") : 0, nfp = fp ? count("fpar") : 0;
    auto need = [&](int ni, int nf) { if (nip != ni || nfp != nf) refio::refuse("ipar / fpar have another length than this kind takes"); };
    int ret = 0;

    switch (kind) {
    case K_PROJ_MAP: {          /* SearchByProjection(F, vpMapPoints, th); fpar = th, nnratio.  -> slot, slotobs of the frame */
        need(0, 2);
        std::vector<MapPoint *> mp = points("", false, false);
        const int n = (int)mp.size();
        const unsigned char *in_view = u8("use", 1, n);
        const float *px = f32("px", 1, n), *py = f32("py", 1, n), *vc = f32("vc", 1, n);
        const float *pxr = req.has("pxr") ? f32("pxr", 1, n) : 0;
        const int32_t *lv = i32("lv", 1, n);
        for (int i = 0; i < n; i++) {
            mp[i]->mbTrackInView = in_view[i] != 0;
            mp[i]->mTrackProjX = px[i];
            mp[i]->mTrackProjY = py[i];
            mp[i]->mTrackProjXR = pxr ? pxr[i] : 0.0f;
            mp[i]->mnTrackScaleLevel = lv[i];
            mp[i]->mTrackViewCos = vc[i];
        }
        Frame F;
        fill_frame(F, "c", f32("bndc", 1, 4), 0);
        frame_scales(F, "c", 0.0f);
        take_slots(F.mvpMapPoints, i32("curobs", 1, F.N));
        ORBmatcher m(fp[1], true);
        ret = m.SearchByProjection(F, mp, fp[0]);
        put_slots(out, F.mvpMapPoints);
        break;
    }
    case K_PROJ_LAST: {         /* SearchByProjection(CurrentFrame, LastFrame, th, bMono); fpar = K[4], mb, mbf, th; ipar = mono, check_ori */
        need(2, 7);
        std::vector<MapPoint *> mp = points("", true, false);
        const int n = (int)mp.size();
        const unsigned char *has = u8("use", 1, n);
        Frame Cur, Last;
        fill_frame(Cur, "c", f32("bndc", 1, 4), 0);
        frame_scales(Cur, "c", 0.0f);
        take_slots(Cur.mvpMapPoints, i32("curobs", 1, Cur.N));
        Frame::fx = fp[0]; Frame::fy = fp[1]; Frame::cx = fp[2]; Frame::cy = fp[3];
        Cur.mb = fp[4];
        Cur.mbf = fp[5];
        Cur.mTcw = mat(f32("Tc", 4, 4), 4, 4);
        Last.mvKeysUn = keys("l");
        Last.mvKeys = Last.mvKeysUn;
        Last.N = (int)Last.mvKeysUn.size();
        if (Last.N != n) refio::refuse("one MapPoint entry per feature of the last frame");
        Last.mvpMapPoints.assign(n, (MapPoint *)0);
        for (int i = 0; i < n; i++)
            if (has[i]) Last.mvpMapPoints[i] = mp[i];
        Last.mvbOutlier.assign(n, false);
        Last.mTcw = mat(f32("Tl", 4, 4), 4, 4);
        ORBmatcher m(0.9f, ip[1] != 0);
        ret = m.SearchByProjection(Cur, Last, fp[6], ip[0] != 0);
        put_slots(out, Cur.mvpMapPoints);
        break;
    }
    case K_PROJ_KF: {           /* SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist); fpar = K[4], logsf, th; ipar = ORBdist, check_ori */
        need(2, 6);
        std::vector<MapPoint *> mp = points("", true, false);
        const int n = (int)mp.size();
        const unsigned char *use = u8("use", 1, n);
        const float *ang = f32("kfang", 1, n);
        Frame Cur;
        fill_frame(Cur, "c", f32("bndc", 1, 4), 0);
        frame_scales(Cur, "c", fp[4]);
        const unsigned char *taken = u8("curhas", 1, Cur.N);
        std::vector<int32_t> obs(Cur.N);
        for (int i = 0; i < Cur.N; i++) obs[i] = taken[i] ? 1 : -1;
        take_slots(Cur.mvpMapPoints, obs.data());
        Frame::fx = fp[0]; Frame::fy = fp[1]; Frame::cx = fp[2]; Frame::cy = fp[3];
        Cur.mTcw = mat(f32("Tc", 4, 4), 4, 4);
        /* the key frame holds the MapPoints; the unusable ones alternate between the three predicates of :1492-1494 */
        KeyFrame kf(n, fp[0], fp[1], fp[2], fp[3], 0.0f, kNoGrid, kNoBounds, Cur.mnScaleLevels, fp[4]);
        kf.mvKeysUn.resize(n);
        std::set<MapPoint *> found;
        for (int i = 0; i < n; i++) {
            kf.mvKeysUn[i].angle = ang[i];
            if (use[i]) kf.mvpMapPoints[i] = mp[i];
            else if (i % 3 == 1) { kf.mvpMapPoints[i] = mp[i]; mp[i]->mbBad = true; }
            else if (i % 3 == 2) { kf.mvpMapPoints[i] = mp[i]; found.insert(mp[i]); }
        }
        ORBmatcher m(0.9f, ip[1] != 0);
        ret = m.SearchByProjection(Cur, &kf, found, fp[5], ip[0]);
        put_slots(out, Cur.mvpMapPoints);
        break;
    }
    case K_PROJ_SIM3:           /* SearchByProjection(pKF, Scw, vpPoints, vpMatched, th); fpar = K[4], logsf; ipar = th.  -> slot */
    case K_FUSE_SIM3: {         /* Fuse(pKF, Scw, vpPoints, th, vpReplacePoint); fpar = K[4], logsf, th.  -> slot, replace */
        if (kind == K_PROJ_SIM3) need(1, 5); else need(0, 6);
        std::vector<MapPoint *> mp = points("", true, true);
        const int n = (int)mp.size();
        const unsigned char *use = u8("use", 1, n);
        KeyFrame *kf = key_frame("k", fp, 0.0f, fp[4], true);
        cv::Mat Scw = mat(f32("Scw", 4, 4), 4, 4);
        ORBmatcher m(0.75f, true);
        if (kind == K_PROJ_SIM3) {
            const unsigned char *matched = u8("matched", 1, kf->N);
            std::vector<MapPoint *> vpMatched(kf->N, (MapPoint *)0);
            for (int i = 0; i < kf->N; i++)
                if (matched[i]) vpMatched[i] = new_point(-2 - i);
            for (int i = 0; i < n; i++)                     /* :317: bad, or already found */
                if (!use[i]) {
                    if (i % 2) mp[i]->mbBad = true;
                    else vpMatched.push_back(mp[i]);       /* spAlreadyFound is built from all of vpMatched; the search reads slots < N only */
                }
            ret = m.SearchByProjection(kf, Scw, mp, vpMatched, ip[0]);
            vpMatched.resize(kf->N);
            put_slots(out, vpMatched);
        } else {
            for (int i = 0; i < n; i++)
                if (!use[i]) mp[i]->mbBad = true;
            if (req.has("kfmp")) {                          /* MapPoints the key frame holds before the call: ids into the list, -1 none */
                const int32_t *held = i32("kfmp", 1, kf->N);
                for (int i = 0; i < kf->N; i++)
                    if (held[i] <= -2) { kf->mvpMapPoints[i] = new_point(held[i]); kf->mvpMapPoints[i]->mObservations[kf] = i; }
                    else if (held[i] >= 0) { kf->mvpMapPoints[i] = mp[held[i]]; mp[held[i]]->mObservations[kf] = i; }
            }
            std::vector<MapPoint *> vpReplacePoint(n, (MapPoint *)0);
            ret = m.Fuse(kf, Scw, mp, fp[5], vpReplacePoint);
            put_slots(out, kf->mvpMapPoints);
            std::vector<int32_t> rep(n, -1);
            for (int i = 0; i < n; i++)
                if (vpReplacePoint[i]) rep[i] = vpReplacePoint[i]->id;
            put_ints(out, "replace", rep);
        }
        break;
    }
    case K_FUSE: {              /* Fuse(pKF, vpMapPoints, th); fpar = K[4], bf, logsf, th.  -> slot, slotobs, bad */
        need(0, 7);
        std::vector<MapPoint *> mp = points("", true, true);
        const int n = (int)mp.size();
        const unsigned char *use = u8("use", 1, n);
        KeyFrame *kf = key_frame("k", fp, fp[4], fp[5], true);
        kf->mvInvLevelSigma2 = floats("isg2k");
        if ((int)kf->mvInvLevelSigma2.size() != kf->mnScaleLevels) refio::refuse("isg2k has another length than sfk");
        set_pose(kf, f32("Tk", 4, 4), f32("Ow", 1, 3));
        std::vector<MapPoint *> list(mp);
        for (int i = 0; i < n; i++)                         /* :846-850: NULL, bad, or in the key frame already */
            if (!use[i]) {
                if (i % 3 == 1) list[i] = 0;
                else if (i % 3 == 2) mp[i]->mObservations[kf] = 0;
                else mp[i]->mbBad = true;
            }
        if (req.has("kfmp")) {
            const int32_t *held = i32("kfmp", 1, kf->N), *hobs = i32("kfobs", 1, kf->N);
            for (int i = 0; i < kf->N; i++)
                if (held[i] <= -2) {
                    MapPoint *h = kf->mvpMapPoints[i] = new_point(held[i]);
                    h->mObservations[kf] = i;
                    h->nObs = hobs[i];
                }
        }
        ORBmatcher m(0.6f, true);
        ret = m.Fuse(kf, list, fp[6]);
        put_slots(out, kf->mvpMapPoints);
        std::vector<int32_t> bad(n);
        for (int i = 0; i < n; i++) bad[i] = mp[i]->mbBad;
        put_ints(out, "bad", bad);
        break;
    }
    case K_BOW: {               /* SearchByBoW(pKF, F, vpMapPointMatches); fpar = nnratio; ipar = check_ori.  -> slot (of the frame) */
        need(1, 1);
        const int nk = count("kak");
        KeyFrame kf(nk, 1, 1, 0, 0, 0, kNoGrid, kNoBounds, 1, 0.0f);
        const float *ak = f32("kak", 1, nk);
        kf.mvKeysUn.resize(nk);
        for (int i = 0; i < nk; i++) kf.mvKeysUn[i].angle = ak[i];
        kf.mDescriptors = bytes(u8("desck", nk, 32), nk, 32);
        kf.mFeatVec = featvec("k");
        const unsigned char *valid = req.has("valk") ? u8("valk", 1, nk) : 0;
        for (int i = 0; i < nk; i++) {
            if (valid && !valid[i] && i % 2) continue;     /* NULL */
            kf.mvpMapPoints[i] = new_point(i);
            if (valid && !valid[i]) kf.mvpMapPoints[i]->mbBad = true;
        }
        Frame F;
        F.N = count("kaf");
        const float *af = f32("kaf", 1, F.N);
        F.mvKeys.resize(F.N);
        for (int i = 0; i < F.N; i++) F.mvKeys[i].angle = af[i];
        F.mDescriptors = bytes(u8("descf", F.N, 32), F.N, 32);
        F.mFeatVec = featvec("f");
        std::vector<MapPoint *> matches;
        ORBmatcher m(fp[0], ip[0] != 0);
        ret = m.SearchByBoW(&kf, F, matches);
        put_slots(out, matches);
        break;
    }
    case K_BOW_KF: {            /* SearchByBoW(pKF1, pKF2, vpMatches12); fpar = nnratio; ipar = check_ori.  -> slot (vpMatches12 as KF2 features) */
        need(1, 1);
        KeyFrame *kf[2];
        const char *sfx[2] = {"1", "2"};
        for (int s = 0; s < 2; s++) {
            const int n = count(tag("ka", sfx[s]));
            kf[s] = new KeyFrame(n, 1, 1, 0, 0, 0, kNoGrid, kNoBounds, 1, 0.0f);
            const float *a = f32(tag("ka", sfx[s]), 1, n);
            const unsigned char *valid = u8(tag("val", sfx[s]), 1, n);
            kf[s]->mvKeysUn.resize(n);
            for (int i = 0; i < n; i++) {
                kf[s]->mvKeysUn[i].angle = a[i];
                if (!valid[i] && i % 2) continue;
                kf[s]->mvpMapPoints[i] = new_point(i);
                if (!valid[i]) kf[s]->mvpMapPoints[i]->mbBad = true;
            }
            kf[s]->mDescriptors = bytes(u8(tag("desc", sfx[s]), n, 32), n, 32);
            kf[s]->mFeatVec = featvec(sfx[s]);
        }
        std::vector<MapPoint *> matches;
        ORBmatcher m(fp[0], ip[0] != 0);
        ret = m.SearchByBoW(kf[0], kf[1], matches);
        put_slots(out, matches);
        delete kf[0];
        delete kf[1];
        break;
    }
    case K_INIT: {              /* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize); fpar = nnratio; ipar = window, check_ori */
        need(2, 1);
        Frame F1, F2;
        fill_frame(F2, "2", f32("bnd2", 1, 4), 0);
        F1.mvKeysUn = keys("1");
        F1.N = (int)F1.mvKeysUn.size();
        F1.mDescriptors = bytes(u8("desc1", F1.N, 32), F1.N, 32);
        const float *prev = f32("prev", F1.N, 2);
        std::vector<cv::Point2f> vbPrevMatched(F1.N);
        for (int i = 0; i < F1.N; i++) vbPrevMatched[i] = cv::Point2f(prev[2 * i], prev[2 * i + 1]);
        std::vector<int> m12;
        ORBmatcher m(fp[0], ip[1] != 0);
        ret = m.SearchForInitialization(F1, F2, vbPrevMatched, m12, ip[0]);
        put_ints(out, "m12", std::vector<int32_t>(m12.begin(), m12.end()));
        std::vector<float> p(2 * (size_t)F1.N + 1);
        for (int i = 0; i < F1.N; i++) { p[2 * i] = vbPrevMatched[i].x; p[2 * i + 1] = vbPrevMatched[i].y; }
        out.put("prev", F32, F1.N, 2, p.data());
        break;
    }
    case K_TRIANG: {            /* SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo); fpar = K2[4]; ipar = only_stereo, check_ori */
        need(2, 4);
        KeyFrame *kf[2];
        const char *sfx[2] = {"1", "2"};
        for (int s = 0; s < 2; s++) {
            if (s == 0 && !req.has("sf1")) {                /* key frame 1's tables are not read */
                const int n = count("kx1");
                kf[0] = new KeyFrame(n, fp[0], fp[1], fp[2], fp[3], 0, kNoGrid, kNoBounds, 1, 0.0f);
                kf[0]->mvKeysUn = keys("1");
                kf[0]->mDescriptors = bytes(u8("desc1", n, 32), n, 32);
                kf[0]->mvuRight = floats("ur1");
            } else {
                kf[s] = key_frame(sfx[s], fp, 0.0f, 0.0f, false);
            }
            const unsigned char *has = u8(tag("has", sfx[s]), 1, kf[s]->N);
            for (int i = 0; i < kf[s]->N; i++)
                if (has[i]) kf[s]->mvpMapPoints[i] = new_point(i);
            kf[s]->mFeatVec = featvec(sfx[s]);
        }
        kf[0]->Ow = mat(f32("Cw", 1, 3), 3, 1);
        set_pose(kf[1], f32("T2", 4, 4), 0);
        kf[1]->mvLevelSigma2 = floats("sg22");
        if (kf[1]->mvLevelSigma2.size() != kf[1]->mvScaleFactors.size()) refio::refuse("sg22 has another length than sf2");
        cv::Mat F12 = mat(f32("F12", 3, 3), 3, 3);
        std::vector<std::pair<size_t, size_t> > pairs;
        ORBmatcher m(0.6f, ip[1] != 0);
        ret = m.SearchForTriangulation(kf[0], kf[1], F12, pairs, ip[0] != 0);
        std::vector<int32_t> flat;
        for (size_t k = 0; k < pairs.size(); k++) { flat.push_back((int32_t)pairs[k].first); flat.push_back((int32_t)pairs[k].second); }
        int32_t none = 0;
        out.put("pairs", I32, (int)pairs.size(), 2, flat.empty() ? &none : flat.data());
        if (!req.has("sf1")) delete kf[0];
        break;
    }
    case K_SIM3: {              /* SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th); fpar = K[4], s12, th, logsf1, logsf2.  -> slot = vpMatches12 as KF2 features */
        need(0, 8);
        KeyFrame *kf[2];
        const char *sfx[2] = {"1", "2"};
        for (int s = 0; s < 2; s++) {
            kf[s] = key_frame(sfx[s], fp, 0.0f, fp[6 + s], true);
            set_pose(kf[s], f32(tag("T", sfx[s]), 4, 4), 0);
            std::vector<MapPoint *> mp = points(sfx[s], true, false);
            if ((int)mp.size() != kf[s]->N) refio::refuse("one MapPoint entry per key-frame feature");
            const unsigned char *use = u8(tag("use", sfx[s]), 1, kf[s]->N);
            for (int i = 0; i < kf[s]->N; i++) {            /* :1152-1156: NULL, or bad */
                if (use[i]) kf[s]->mvpMapPoints[i] = mp[i];
                else if (i % 2) { kf[s]->mvpMapPoints[i] = mp[i]; mp[i]->mbBad = true; }
            }
        }
        std::vector<MapPoint *> vpMatches12(kf[0]->N, (MapPoint *)0);
        const float s12 = fp[4];
        cv::Mat R12 = mat(f32("R12", 3, 3), 3, 3), t12 = mat(f32("t12", 1, 3), 3, 1);
        ORBmatcher m(0.75f, true);
        ret = m.SearchBySim3(kf[0], kf[1], vpMatches12, s12, R12, t12, fp[5]);
        put_slots(out, vpMatches12);
        break;
    }
    default:
        refio::refuse("unknown kind");
    }

    out.i32("ret", ret);
    std::vector<int32_t> &log = ref_matcher_log();
    int32_t none = 0;
    out.put("log", I32, (int)(log.size() / 3), 3, log.empty() ? &none : log.data());
    out.close();
    return 0;
}
