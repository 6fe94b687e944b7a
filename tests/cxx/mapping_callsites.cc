// mapping_callsites.cc -- a repo-authored caller that uses the SAME CALL EXPRESSIONS as the reference's LocalMapping and LoopClosing
// threads on the drop-in class of my-slam_amd/host/ORBmatcher.h and checks every result against direct C-ABI calls on independently
// marshalled arrays (tests/test_kf_matchers.py ties those to the oracle):
//   src/LocalMapping.cc:217,270  ORBmatcher matcher(0.6,false); matcher.SearchForTriangulation(mpCurrentKeyFrame,pKF2,F12,vMatchedIndices,false)
//   src/LocalMapping.cc:485,491  ORBmatcher matcher; matcher.Fuse(pKFi,vpMapPointMatches)
//   src/LocalMapping.cc:516      matcher.Fuse(mpCurrentKeyFrame,vpFuseCandidates)
//   src/LoopClosing.cc:240,266   ORBmatcher matcher(0.75,true); matcher.SearchByBoW(mpCurrentKF,pKF,vvpMapPointMatches[i])
//   src/LoopClosing.cc:324       matcher.SearchBySim3(mpCurrentKF,pKF,vpMapPointMatches,s,R,t,7.5)
//   src/LoopClosing.cc:376       matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints,10)
//   src/LoopClosing.cc:590,600   ORBmatcher matcher(0.8); matcher.Fuse(pKF,cvScw,mvpLoopMapPoints,4,vpReplacePoints)
// For the two Fuse variants the object graph after the call (key-frame slots, bad flags, observation counts, replacement links) is
// compared with a model that replays src/ORBmatcher.cc:952-971 / :1082-1096 on the C ABI's match table.
// The last block drives this thread's pooled handle through Fuse(X), an empty SearchBySim3 and Fuse(KF1) (row Fuse(KF,after-empty-Sim3)).
// The Frame / KeyFrame / MapPoint classes are the minimal ones of tests/cxx/slam_shims/ (an ORB-SLAM2 tree brings its own).
// usage: mapping_callsites frames.u8 layer.u8 W H vocabulary.txt      (frames.u8 = two W x H frames, layer.u8 = depth layer per pixel)
// prints one line per call site: <name> <result> <1 if equal to the C ABI>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "orbv.h"

using namespace std;
using namespace ORB_SLAM2;

static vector<unsigned char> read_file(const char *path, size_t n)
{
    vector<unsigned char> b(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(b.data(), 1, n, f) != n) { fprintf(stderr, "cannot read %zu bytes from %s\n", n, path); exit(2); }
    fclose(f);
    return b;
}
static cv::Mat eye4()
{
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.f : 0.f;
    return T;
}
static void compute_bow(orbv_vocabulary *voc, const cv::Mat &desc, int n, DBoW2::FeatureVector &fv)
{
    vector<int32_t> word(n), node(n), nid(n + 1), off(n + 2), idx(n);
    vector<double> w(n);
    if (orbv_transform_features(voc, desc.ptr<unsigned char>(), n, 2, word.data(), node.data(), w.data()) != 0) { fprintf(stderr, "transform: %s\n", orbv_last_error()); exit(3); }
    const int nn = orbv_feature_vector(node.data(), w.data(), n, nid.data(), off.data(), idx.data(), n + 1);
    if (nn < 0) { fprintf(stderr, "feature_vector: %s\n", orbv_last_error()); exit(3); }
    fv.clear();
    for (int i = 0; i < nn; i++)
        for (int k = off[i]; k < off[i + 1]; k++) fv[(DBoW2::NodeId)nid[i]].push_back((unsigned int)idx[k]);
}
static void flatten(const DBoW2::FeatureVector &fv, vector<int32_t> &node, vector<int32_t> &off, vector<int32_t> &idx)
{
    node.clear(); off.assign(1, 0); idx.clear();
    for (auto &e : fv) { node.push_back((int32_t)e.first); for (unsigned v : e.second) idx.push_back((int32_t)v); off.push_back((int32_t)idx.size()); }
}
#define CK(x) do { if ((x) != 0) { fprintf(stderr, "%s failed: %s\n", #x, orbm_last_error()); exit(4); } } while (0)

// one key frame of the scene with its MapPoints and the flat arrays a direct C-ABI call needs
struct Side {
    KeyFrame *kf = nullptr;
    vector<MapPoint *> mps;          // one slot per feature at construction time
    float T[16];
    orbm_kf_grid grid;
    float bounds[4];
};
struct Flat {                        // the MapPoints of a list as arrays (what the adapter gathers)
    vector<float> xw, normal, minInv, maxInv, mfMax;
    vector<unsigned char> desc;
    void from(const vector<MapPoint *> &pts)
    {
        const int n = (int)pts.size();
        xw.assign((size_t)3 * n, 0.f); normal.assign((size_t)3 * n, 0.f); minInv.assign(n, 0.f); maxInv.assign(n, 0.f); mfMax.assign(n, 0.f);
        desc.assign((size_t)32 * n, 0);
        for (int i = 0; i < n; i++) {
            MapPoint *p = pts[i];
            if (!p) continue;
            const cv::Mat X = p->GetWorldPos(), N = p->GetNormal();
            for (int k = 0; k < 3; k++) { xw[(size_t)3 * i + k] = X.at<float>(k); normal[(size_t)3 * i + k] = N.at<float>(k); }
            minInv[i] = p->GetMinDistanceInvariance(); maxInv[i] = p->GetMaxDistanceInvariance(); mfMax[i] = p->MaxDistance();
            memcpy(&desc[(size_t)32 * i], p->GetDescriptor().ptr<unsigned char>(), 32);
        }
    }
};

// a light model of the object graph for replaying Fuse's bookkeeping (src/ORBmatcher.cc:952-971; MapPoint::Replace, AddObservation)
struct Model {
    struct MP { bool bad; int obs; map<int, int> in; MapPoint *replaced; };      // in: key frame (0 / 1 / 2) -> slot
    map<MapPoint *, MP> mp;
    vector<MapPoint *> slot[3];
    vector<float> uright[3];
    void add_obs(MapPoint *p, int kf, int idx) { MP &m = mp[p]; if (m.in.count(kf)) return; m.in[kf] = idx; m.obs += uright[kf][idx] >= 0 ? 2 : 1; }
    void replace(MapPoint *a, MapPoint *b)      // a->Replace(b)
    {
        if (a == b) return;
        map<int, int> obs = mp[a].in;
        mp[a].in.clear(); mp[a].bad = true; mp[a].replaced = b;
        for (auto &o : obs) {
            if (!mp[b].in.count(o.first)) { slot[o.first][o.second] = b; add_obs(b, o.first, o.second); }
            else slot[o.first][o.second] = nullptr;
        }
    }
};

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    if (argc < 6) { fprintf(stderr, "usage: %s frames.u8 layer.u8 W H vocabulary.txt\n", argv[0]); return 2; }
    const int W = atoi(argv[3]), H = atoi(argv[4]);
    vector<unsigned char> raw = read_file(argv[1], (size_t)2 * W * H), layer = read_file(argv[2], (size_t)W * H);
    orbv_vocabulary *voc = nullptr;
    if (orbv_load_text(&voc, argv[5], 0) != 0) { fprintf(stderr, "vocabulary: %s\n", orbv_last_error()); return 3; }
    const int nFeatures = 2000, nLevels = 8;
    ORBextractor *extractor = new ORBextractor(nFeatures, 1.2f, nLevels, 20, 7);
    if (!extractor->Valid()) { fprintf(stderr, "extractor: %s\n", extractor->LastError().c_str()); return 3; }
    const float fx = 718.856f, fy = 718.856f, cx = 607.1928f, cy = 185.2157f, base = 0.5f, bf = fx * base;
    const float shifts[3] = {2.f, 4.f, 6.f};
    Frame::mnMinX = 0.f; Frame::mnMaxX = (float)W; Frame::mnMinY = 0.f; Frame::mnMaxY = (float)H;
    Frame::mfGridElementWidthInv = 64.f / (Frame::mnMaxX - Frame::mnMinX); Frame::mfGridElementHeightInv = 48.f / (Frame::mnMaxY - Frame::mnMinY);

    orbm_matcher *ref = nullptr;                      // the direct C-ABI side of every comparison
    CK(orbm_create(&ref, 0, 8192, 8192, 1 << 22));
    int nfail = 0;
    auto report = [&](const char *name, int nm, bool same) { printf("%s %d %d\n", name, nm, same ? 1 : 0); nfail += !same; };

    // ---- the two key frames: frame 0 at the origin, frame 1 a baseline further along +x; MapPoints = back-projected keypoints ----
    Side sd[3];                                       // [2]: the mirrored key frame X of the last block
    vector<float> logSf(1);
    for (int s = 0; s < 2; s++) {
        cv::Mat im(H, W, CV_8UC1, raw.data() + (size_t)s * W * H, W);
        Frame F(im, extractor, fx, fy, cx, cy, bf);
        const int N = F.N;
        cv::Mat Tcw = eye4();
        Tcw.at<float>(0, 3) = s == 0 ? 0.f : -base;
        vector<MapPoint *> mps(N, static_cast<MapPoint *>(NULL));
        vector<float> uRight(N, -1.f);
        for (int i = 0; i < N; i++) {
            const cv::KeyPoint &kp = F.mvKeysUn[i];
            const int px = min(max((int)lrintf(kp.pt.x), 0), W - 1), py = min(max((int)lrintf(kp.pt.y), 0), H - 1);
            const float Z = fx * base / shifts[layer[(size_t)py * W + px] % 3];
            if ((i * 7 + s) % 5 < 2) uRight[i] = kp.pt.x - bf / Z;                                  // stereo observations
            if ((i * 3 + s) % 5 < 2) continue;                                                     // features without a MapPoint
            cv::Mat x3D(3, 1, CV_32F);
            const float xc = (kp.pt.x - cx) * Z / fx, yc = (kp.pt.y - cy) * Z / fy;
            x3D.at<float>(0) = xc - Tcw.at<float>(0, 3); x3D.at<float>(1) = yc; x3D.at<float>(2) = Z;
            const float dist = sqrtf(xc * xc + yc * yc + Z * Z);
            const float mfMax = dist * F.mvScaleFactors[kp.octave], mfMin = mfMax / F.mvScaleFactors[nLevels - 1];
            mps[i] = new MapPoint(x3D, F.mDescriptors.row(i), i % 3, mfMin, mfMax);
            mps[i]->SetNormal(xc / dist, yc / dist, Z / dist);
            if (i % 23 == 7) mps[i]->SetNormal(-xc / dist, -yc / dist, -Z / dist);                 // seen from behind
            if (i % 29 == 11) mps[i]->SetBadFlag();
        }
        DBoW2::FeatureVector fv;
        compute_bow(voc, F.mDescriptors, N, fv);
        sd[s].kf = new KeyFrame(10 + s, F.mvKeysUn, uRight, F.mDescriptors, fv, mps, fx, fy, cx, cy, bf, Frame::mfGridElementWidthInv,
                                Frame::mfGridElementHeightInv, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY, F.mvScaleFactors, F.mvLevelSigma2,
                                F.mvInvLevelSigma2, F.mfLogScaleFactor);
        sd[s].kf->SetPose(Tcw);
        cv::Mat Ow(3, 1, CV_32F);
        Ow.at<float>(0) = -Tcw.at<float>(0, 3); Ow.at<float>(1) = 0.f; Ow.at<float>(2) = 0.f;      // R = I
        sd[s].kf->SetCameraCenter(Ow);
        for (int i = 0; i < N; i++)
            if (mps[i]) mps[i]->AddObservation(sd[s].kf, i);
        sd[s].mps = mps;
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) sd[s].T[4 * r + c] = Tcw.at<float>(r, c);
        sd[s].grid = {Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv, (float)sd[s].kf->mnMinX, (float)sd[s].kf->mnMinY};
        sd[s].bounds[0] = (float)sd[s].kf->mnMinX; sd[s].bounds[1] = (float)sd[s].kf->mnMaxX; sd[s].bounds[2] = (float)sd[s].kf->mnMinY; sd[s].bounds[3] = (float)sd[s].kf->mnMaxY;
        logSf[0] = F.mfLogScaleFactor;
    }
    KeyFrame *mpCurrentKeyFrame = sd[0].kf, *pKF2 = sd[1].kf;
    const int N1 = mpCurrentKeyFrame->N, N2 = pKF2->N;
    auto kpp = [](const KeyFrame *k) { return (const orbx_keypoint *)k->mvKeysUn.data(); };
    auto dsc = [](const KeyFrame *k) { return k->mDescriptors.ptr<unsigned char>(); };
    vector<int32_t> n1v, o1v, i1v, n2v, o2v, i2v;
    flatten(mpCurrentKeyFrame->mFeatVec, n1v, o1v, i1v); flatten(pKF2->mFeatVec, n2v, o2v, i2v);

    // ================= LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:217-270) =================
    {
        ORBmatcher matcher(0.6,false);
        // F12 of the true motion (LocalMapping::ComputeF12): K^-T [t12]x R12 K^-1 with R12 = I, t12 = (base, 0, 0)
        cv::Mat F12(3, 3, CV_32F);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) F12.at<float>(r, c) = 0.f;
        F12.at<float>(1, 2) = -base / fy; F12.at<float>(2, 1) = base / fy;
        // Search matches that fullfil epipolar constraint
        vector<pair<size_t,size_t> > vMatchedIndices;
        int nm = matcher.SearchForTriangulation(mpCurrentKeyFrame,pKF2,F12,vMatchedIndices,false);
        vector<uint8_t> h1(N1), h2(N2);
        for (int i = 0; i < N1; i++) h1[i] = mpCurrentKeyFrame->GetMapPoint(i) != NULL;
        for (int i = 0; i < N2; i++) h2[i] = pKF2->GetMapPoint(i) != NULL;
        float Cw[3] = {0.f, 0.f, 0.f}, F[9];
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) F[3 * r + c] = F12.at<float>(r, c);
        vector<int32_t> m12(N1, -1);
        int rn = 0;
        CK(orbm_search_for_triangulation(ref, kpp(mpCurrentKeyFrame), dsc(mpCurrentKeyFrame), N1, h1.data(), mpCurrentKeyFrame->mvuRight.data(), n1v.data(),
                                         o1v.data(), i1v.data(), (int)n1v.size(), kpp(pKF2), dsc(pKF2), N2, h2.data(), pKF2->mvuRight.data(), n2v.data(),
                                         o2v.data(), i2v.data(), (int)n2v.size(), Cw, sd[1].T, fx, fy, cx, cy, F, pKF2->mvScaleFactors.data(),
                                         pKF2->mvLevelSigma2.data(), nLevels, 0, 0, m12.data(), &rn));
        bool same = rn == nm;
        size_t k = 0;
        for (int i = 0; same && i < N1; i++)
            if (m12[i] >= 0) { same = k < vMatchedIndices.size() && vMatchedIndices[k].first == (size_t)i && vMatchedIndices[k].second == (size_t)m12[i]; k++; }
        same = same && k == vMatchedIndices.size();
        report("SearchForTriangulation", nm, same);
    }

    // ================= LoopClosing::ComputeSim3 (src/LoopClosing.cc:240-376) =================
    KeyFrame *mpCurrentKF = mpCurrentKeyFrame, *pKF = pKF2;
    vector<MapPoint *> vpMapPointMatches;
    {
        ORBmatcher matcher(0.75,true);
        vector<vector<MapPoint*> > vvpMapPointMatches(1);
        const int i = 0;
        int nmatches = matcher.SearchByBoW(mpCurrentKF,pKF,vvpMapPointMatches[i]);
        vector<uint8_t> v1(N1), v2(N2);
        for (int k = 0; k < N1; k++) v1[k] = sd[0].mps[k] && !sd[0].mps[k]->isBad();
        for (int k = 0; k < N2; k++) v2[k] = sd[1].mps[k] && !sd[1].mps[k]->isBad();
        vector<int32_t> m12(N1, -1);
        int rn = 0;
        CK(orbm_search_by_bow_kf(ref, dsc(mpCurrentKF), kpp(mpCurrentKF), N1, v1.data(), n1v.data(), o1v.data(), i1v.data(), (int)n1v.size(), dsc(pKF), kpp(pKF), N2,
                                 v2.data(), n2v.data(), o2v.data(), i2v.data(), (int)n2v.size(), 0.75f, 1, m12.data(), &rn));
        bool same = rn == nmatches && (int)vvpMapPointMatches[i].size() == N1;
        for (int k = 0; same && k < N1; k++) same = vvpMapPointMatches[i][k] == (m12[k] >= 0 ? sd[1].mps[m12[k]] : static_cast<MapPoint *>(NULL));
        report("SearchByBoW(KF,KF)", nmatches, same);

        // the Sim3 solver's inliers: every third BoW match (src/LoopClosing.cc:312-317)
        vpMapPointMatches = vector<MapPoint*>(vvpMapPointMatches[i].size(), static_cast<MapPoint*>(NULL));
        for (size_t j = 0; j < vvpMapPointMatches[i].size(); j += 3) vpMapPointMatches[j] = vvpMapPointMatches[i][j];
        vector<MapPoint *> before = vpMapPointMatches;
        cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.at<float>(r, c) = r == c ? 1.f : 0.f;
        t.at<float>(0) = base; t.at<float>(1) = 0.f; t.at<float>(2) = 0.f;                          // x1 = s R x2 + t
        const float s = 1.0f;
        int nfound = matcher.SearchBySim3(mpCurrentKF,pKF,vpMapPointMatches,s,R,t,7.5);
        // the same through the C ABI
        float R12[9], t12[3] = {base, 0.f, 0.f}, sR12[9], sR21[9], t21[3];
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R12[3 * r + c] = r == c ? 1.f : 0.f;
        CK(orbm_sim3_relative(s, R12, t12, sR12, sR21, t21));
        vector<uint8_t> already1(N1, 0), already2(N2, 0);
        for (int k = 0; k < N1; k++)
            if (before[k]) { already1[k] = 1; int idx2 = before[k]->GetIndexInKeyFrame(pKF); if (idx2 >= 0 && idx2 < N2) already2[idx2] = 1; }
        Flat f1, f2;
        f1.from(sd[0].mps); f2.from(sd[1].mps);
        auto oneSide = [&](const vector<MapPoint *> &mps, const vector<uint8_t> &already, const Flat &f, const float *TAw, const float *sR, const float *tt,
                           const float *boundsB, vector<uint8_t> &use, vector<float> &u, vector<float> &v, vector<int32_t> &lv) {
            const int n = (int)mps.size();
            vector<float> d3(n);
            vector<uint8_t> okv(n);
            use.assign(n, 0); u.assign(n, 0.f); v.assign(n, 0.f); lv.assign(n, 0);
            CK(orbm_project_points_sim3(TAw, sR, tt, fx, fy, cx, cy, boundsB, f.xw.data(), n, u.data(), v.data(), d3.data(), okv.data()));
            for (int k = 0; k < n; k++) {
                if (!mps[k] || already[k] || mps[k]->isBad() || !okv[k] || d3[k] < f.minInv[k] || d3[k] > f.maxInv[k]) continue;
                use[k] = 1;
                lv[k] = orbm_predict_scale(f.mfMax[k], d3[k], logSf[0], nLevels);
            }
        };
        vector<uint8_t> use1, use2;
        vector<float> u1, v1f, u2, v2f;
        vector<int32_t> lv1, lv2, rm12(N1, -1);
        oneSide(sd[0].mps, already1, f1, sd[0].T, sR21, t21, sd[1].bounds, use1, u1, v1f, lv1);
        oneSide(sd[1].mps, already2, f2, sd[1].T, sR12, t12, sd[0].bounds, use2, u2, v2f, lv2);
        int rf = 0;
        CK(orbm_search_by_sim3(ref, N1, use1.data(), u1.data(), v1f.data(), lv1.data(), f1.desc.data(), N2, use2.data(), u2.data(), v2f.data(), lv2.data(),
                               f2.desc.data(), kpp(mpCurrentKF), dsc(mpCurrentKF), N1, &sd[0].grid, mpCurrentKF->mvScaleFactors.data(), nLevels, kpp(pKF), dsc(pKF),
                               N2, &sd[1].grid, pKF->mvScaleFactors.data(), nLevels, 7.5f, rm12.data(), &rf));
        same = rf == nfound;
        for (int k = 0; same && k < N1; k++) same = vpMapPointMatches[k] == (rm12[k] >= 0 ? sd[1].mps[rm12[k]] : before[k]);
        report("SearchBySim3", nfound, same);
    }
    {
        ORBmatcher matcher(0.75,true);
        // mScw = the Sim3 of the current key frame predicted from the loop side: the true pose of key frame 2 with a scale of 1.02
        cv::Mat mScw = eye4();
        const float sc = 1.02f;
        for (int r = 0; r < 3; r++) mScw.at<float>(r, r) = sc;
        mScw.at<float>(0, 3) = sc * -base;
        vector<MapPoint *> mvpLoopMapPoints;
        for (int k = 0; k < N1; k++) if (sd[0].mps[k]) mvpLoopMapPoints.push_back(sd[0].mps[k]);
        vector<MapPoint *> mvpCurrentMatchedPoints(N2, static_cast<MapPoint *>(NULL));
        for (int k = 0; k < N2; k += 7) if (sd[1].mps[k]) mvpCurrentMatchedPoints[k] = sd[1].mps[k];
        for (int k = 3; k < N2; k += 50) mvpCurrentMatchedPoints[k] = mvpLoopMapPoints[(size_t)k % mvpLoopMapPoints.size()];   // loop points found already
        vector<MapPoint *> before = mvpCurrentMatchedPoints;
        int nm = matcher.SearchByProjection(pKF2, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints,10);
        float Sc[16], T[16], Ow[3];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Sc[4 * r + c] = mScw.at<float>(r, c);
        CK(orbm_sim3_decompose(Sc, T, Ow));
        const int n = (int)mvpLoopMapPoints.size();
        Flat f;
        f.from(mvpLoopMapPoints);
        set<MapPoint *> found(before.begin(), before.end());
        found.erase(static_cast<MapPoint *>(NULL));
        vector<float> u(n), v(n), d3(n);
        vector<uint8_t> okv(n), use(n, 0), taken(N2);
        vector<int32_t> lv(n, 0), km(N2, -1);
        CK(orbm_project_points_kf(T, Ow, fx, fy, cx, cy, sd[1].bounds, f.xw.data(), f.normal.data(), n, u.data(), v.data(), nullptr, d3.data(), okv.data()));
        for (int k = 0; k < n; k++) {
            MapPoint *p = mvpLoopMapPoints[k];
            if (p->isBad() || found.count(p) || !okv[k] || d3[k] < f.minInv[k] || d3[k] > f.maxInv[k]) continue;
            use[k] = 1;
            lv[k] = orbm_predict_scale(f.mfMax[k], d3[k], logSf[0], nLevels);
        }
        for (int k = 0; k < N2; k++) taken[k] = before[k] != NULL;
        CK(orbm_grid_build_kf(ref, kpp(pKF2), N2, sd[1].grid.assign_min_x, sd[1].grid.assign_min_y, sd[1].grid.inv_w, sd[1].grid.inv_h, sd[1].grid.query_min_x,
                              sd[1].grid.query_min_y));
        int rn = 0;
        CK(orbm_search_by_projection_sim3(ref, n, use.data(), u.data(), v.data(), lv.data(), f.desc.data(), pKF2->mvScaleFactors.data(), nLevels, kpp(pKF2), dsc(pKF2),
                                          N2, 10, taken.data(), km.data(), &rn));
        bool same = rn == nm;
        for (int k = 0; same && k < N2; k++) same = mvpCurrentMatchedPoints[k] == (km[k] >= 0 ? mvpLoopMapPoints[km[k]] : before[k]);
        report("SearchByProjection(KF,Scw)", nm, same);
    }

    // the model of the object graph, for the three Fuse calls below
    Model M;
    for (int s = 0; s < 2; s++) {
        M.slot[s] = sd[s].mps; M.uright[s] = sd[s].kf->mvuRight;
        for (int i = 0; i < (int)sd[s].mps.size(); i++)
            if (sd[s].mps[i]) { Model::MP m; m.bad = sd[s].mps[i]->isBad(); m.obs = sd[s].mps[i]->Observations(); m.in[s] = i; m.replaced = nullptr; M.mp[sd[s].mps[i]] = m; }
    }
    auto graph_equals_model = [&]() {
        bool same = true;
        for (int s = 0; s < 3 && same; s++)
            for (int i = 0; i < (int)M.slot[s].size() && same; i++) same = sd[s].kf->GetMapPoint(i) == M.slot[s][i];
        for (auto &e : M.mp) {
            if (!same) break;
            same = e.first->isBad() == e.second.bad && e.first->Observations() == e.second.obs && e.first->GetReplaced() == e.second.replaced &&
                   e.first->IsInKeyFrame(sd[0].kf) == (e.second.in.count(0) != 0) && e.first->IsInKeyFrame(sd[1].kf) == (e.second.in.count(1) != 0) &&
                   (!sd[2].kf || e.first->IsInKeyFrame(sd[2].kf) == (e.second.in.count(2) != 0));
        }
        return same;
    };

    // ================= LoopClosing::SearchAndFuse (src/LoopClosing.cc:588-615) =================
    {
        ORBmatcher matcher(0.8);
        KeyFrame *pKFf = pKF2;
        cv::Mat cvScw = eye4();
        const float sc = 0.99f;
        for (int r = 0; r < 3; r++) cvScw.at<float>(r, r) = sc;
        cvScw.at<float>(0, 3) = sc * -base;
        vector<MapPoint *> mvpLoopMapPoints;
        for (int k = 0; k < N1; k += 2) if (sd[0].mps[k]) mvpLoopMapPoints.push_back(sd[0].mps[k]);
        const int n = (int)mvpLoopMapPoints.size();
        // the C ABI's match table on the state before the call
        float Sc[16], T[16], Ow[3];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Sc[4 * r + c] = cvScw.at<float>(r, c);
        CK(orbm_sim3_decompose(Sc, T, Ow));
        Flat f;
        f.from(mvpLoopMapPoints);
        const set<MapPoint *> inKF = pKFf->GetMapPoints();
        vector<float> u(n), v(n), d3(n);
        vector<uint8_t> okv(n), use(n, 0);
        vector<int32_t> lv(n, 0), best(n, -1);
        CK(orbm_project_points_kf(T, Ow, fx, fy, cx, cy, sd[1].bounds, f.xw.data(), f.normal.data(), n, u.data(), v.data(), nullptr, d3.data(), okv.data()));
        for (int k = 0; k < n; k++) {
            MapPoint *p = mvpLoopMapPoints[k];
            if (p->isBad() || inKF.count(p) || !okv[k] || d3[k] < f.minInv[k] || d3[k] > f.maxInv[k]) continue;
            use[k] = 1;
            lv[k] = orbm_predict_scale(f.mfMax[k], d3[k], logSf[0], nLevels);
        }
        int cnt = 0;
        CK(orbm_grid_build_kf(ref, kpp(pKFf), N2, sd[1].grid.assign_min_x, sd[1].grid.assign_min_y, sd[1].grid.inv_w, sd[1].grid.inv_h, sd[1].grid.query_min_x,
                              sd[1].grid.query_min_y));
        CK(orbm_fuse_sim3(ref, n, use.data(), u.data(), v.data(), lv.data(), f.desc.data(), pKFf->mvScaleFactors.data(), nLevels, kpp(pKFf), dsc(pKFf), N2, 4.f,
                          best.data(), &cnt));
        // the model replays :1082-1096
        vector<MapPoint *> wantReplace(n, static_cast<MapPoint *>(NULL));
        int wantFused = 0;
        for (int k = 0; k < n; k++) {
            if (best[k] < 0) continue;
            MapPoint *in = M.slot[1][best[k]];
            if (in) { if (!M.mp[in].bad) wantReplace[k] = in; }
            else { M.add_obs(mvpLoopMapPoints[k], 1, best[k]); M.slot[1][best[k]] = mvpLoopMapPoints[k]; }
            wantFused++;
        }
        vector<MapPoint*> vpReplacePoints(mvpLoopMapPoints.size(),static_cast<MapPoint*>(NULL));
        int nFused = matcher.Fuse(pKFf,cvScw,mvpLoopMapPoints,4,vpReplacePoints);
        bool same = nFused == wantFused && vpReplacePoints == wantReplace && graph_equals_model();
        report("Fuse(KF,Scw)", nFused, same);
    }

    // ================= LocalMapping::SearchInNeighbors (src/LocalMapping.cc:485-516) =================
    // the points fused into key frame b (sd[b]) by a fresh ORBmatcher on this thread's pooled handle, against orbm_fuse on a grid built
    // for the call in `ref` and the model's replay of :842-850 / :952-971
    auto fuse_into = [&](int b, const vector<MapPoint *> &vpMapPointMatches, int *nFusedOut) {
        ORBmatcher matcher;
        KeyFrame *pKFi = sd[b].kf;
        const int n = (int)vpMapPointMatches.size(), nB = sd[b].kf->N;
        Flat f;
        f.from(vpMapPointMatches);
        float Ow[3] = {-sd[b].T[3], 0.f, 0.f};
        vector<float> u(n), v(n), iz(n), d3(n), ur(n);
        vector<uint8_t> okv(n), use(n, 0);
        vector<int32_t> lv(n, 0), best(n, -1);
        CK(orbm_project_points_kf(sd[b].T, Ow, fx, fy, cx, cy, sd[b].bounds, f.xw.data(), f.normal.data(), n, u.data(), v.data(), iz.data(), d3.data(), okv.data()));
        for (int k = 0; k < n; k++) {
            MapPoint *p = vpMapPointMatches[k];
            ur[k] = u[k] - bf * iz[k];
            if (!p || p->isBad() || p->IsInKeyFrame(pKFi) || !okv[k] || d3[k] < f.minInv[k] || d3[k] > f.maxInv[k]) continue;
            use[k] = 1;
            lv[k] = orbm_predict_scale(f.mfMax[k], d3[k], logSf[0], nLevels);
        }
        int cnt = 0;
        CK(orbm_grid_build_kf(ref, kpp(pKFi), nB, sd[b].grid.assign_min_x, sd[b].grid.assign_min_y, sd[b].grid.inv_w, sd[b].grid.inv_h, sd[b].grid.query_min_x,
                              sd[b].grid.query_min_y));
        CK(orbm_fuse(ref, n, use.data(), u.data(), v.data(), ur.data(), lv.data(), f.desc.data(), pKFi->mvScaleFactors.data(), pKFi->mvInvLevelSigma2.data(), nLevels,
                     kpp(pKFi), pKFi->mvuRight.data(), dsc(pKFi), nB, 3.0f, best.data(), &cnt));
        int wantFused = 0;
        for (int k = 0; k < n; k++) {                          // the model replays :842-850 and :952-971
            MapPoint *p = vpMapPointMatches[k];
            if (!p) continue;
            if (M.mp[p].bad || M.mp[p].in.count(b)) continue;
            if (best[k] < 0) continue;
            MapPoint *in = M.slot[b][best[k]];
            if (in) {
                if (!M.mp[in].bad) { if (M.mp[in].obs > M.mp[p].obs) M.replace(p, in); else M.replace(in, p); }
            } else { M.add_obs(p, b, best[k]); M.slot[b][best[k]] = p; }
            wantFused++;
        }
        int nFused = matcher.Fuse(pKFi,vpMapPointMatches);
        *nFusedOut = nFused;
        return nFused == wantFused && graph_equals_model();
    };
    for (int dir = 0; dir < 2; dir++) {
        const int a = dir, b = 1 - dir;                       // points of key frame a fused into key frame b
        vector<MapPoint*> vpMapPointMatches = sd[a].kf->GetMapPointMatches();
        if (dir == 1) {                                        // vpFuseCandidates: no NULLs, no bad points (:497-512)
            vector<MapPoint *> c;
            for (MapPoint *p : vpMapPointMatches) if (p && !p->isBad()) c.push_back(p);
            vpMapPointMatches = c;
        }
        int nFused = 0;
        const bool same = fuse_into(b, vpMapPointMatches, &nFused);
        report(dir == 0 ? "Fuse(KF,points)" : "Fuse(KF,candidates)", nFused, same);
    }

    // ================= one thread's handle through Fuse(X), an empty SearchBySim3 and Fuse(KF1) =================
    // X = key frame 1 mirrored (x -> W-1-x): the same N, the same descriptors, other cells.  Fuse(X, ...) leaves X's grid in the pooled
    // handle; SearchBySim3 with every slot of vpMatches12 taken has nothing to search (nq1 == 0) and must not leave that grid behind
    // labelled as key frame 1's, or the next Fuse(KF1, ...) on this thread searches X's cells.  The points: fresh MapPoints at key
    // frame 1's points (another key frame's triangulation of them), so that they are neither in key frame 1 nor in X.
    {
        KeyFrame *pKF1 = mpCurrentKeyFrame;
        vector<cv::KeyPoint> mirrored = pKF1->mvKeysUn;
        for (cv::KeyPoint &kp : mirrored) kp.pt.x = (float)(W - 1) - kp.pt.x;
        sd[2] = sd[0];
        sd[2].kf = new KeyFrame(20, mirrored, pKF1->mvuRight, pKF1->mDescriptors, pKF1->mFeatVec, vector<MapPoint *>(N1, static_cast<MapPoint *>(NULL)), fx, fy,
                                cx, cy, bf, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX,
                                Frame::mnMaxY, pKF1->mvScaleFactors, pKF1->mvLevelSigma2, pKF1->mvInvLevelSigma2, pKF1->mfLogScaleFactor);
        cv::Mat Tcw = eye4();
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = sd[0].T[4 * r + c];
        sd[2].kf->SetPose(Tcw);
        sd[2].kf->SetCameraCenter(pKF1->GetCameraCenter());
        sd[2].mps = sd[2].kf->GetMapPointMatches();
        M.slot[2] = sd[2].mps; M.uright[2] = sd[2].kf->mvuRight;
        vector<MapPoint *> points;
        for (MapPoint *p : pKF1->GetMapPointMatches()) {
            if (!p || p->isBad()) continue;
            MapPoint *q = new MapPoint(p->GetWorldPos(), p->GetDescriptor(), 1, p->MaxDistance() / pKF1->mvScaleFactors[nLevels - 1], p->MaxDistance());
            const cv::Mat N = p->GetNormal();
            q->SetNormal(N.at<float>(0), N.at<float>(1), N.at<float>(2));
            Model::MP m; m.bad = false; m.obs = 1; m.replaced = nullptr; M.mp[q] = m;
            points.push_back(q);
        }
        int nX = 0, nFused = 0;
        bool same = fuse_into(2, points, &nX);
        {
            ORBmatcher matcher(0.75,true);
            vector<MapPoint *> vpMatches12(N1, static_cast<MapPoint *>(NULL));
            vector<MapPoint *> kf2 = pKF2->GetMapPointMatches();
            for (int k = 0, j = 0; k < N1; k++, j++) {             // every slot taken: vbAlreadyMatched1 is all true
                while (!kf2[j % N2]) j++;
                vpMatches12[k] = kf2[j % N2];
            }
            const vector<MapPoint *> before = vpMatches12;
            cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.at<float>(r, c) = r == c ? 1.f : 0.f;
            t.at<float>(0) = base; t.at<float>(1) = 0.f; t.at<float>(2) = 0.f;
            const int nfound = matcher.SearchBySim3(pKF1,pKF2,vpMatches12,1.0f,R,t,7.5);
            same = same && nfound == 0 && vpMatches12 == before;
        }
        same = fuse_into(0, points, &nFused) && same;
        report("Fuse(KF,after-empty-Sim3)", nFused, same);
    }

    orbm_destroy(ref);
    orbv_destroy(voc);
    return nfail ? 1 : 0;
}
