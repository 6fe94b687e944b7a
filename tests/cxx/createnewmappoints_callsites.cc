// createnewmappoints_callsites.cc -- the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:239-453) written
// twice, as INTEGRATION.md 3h shows it before and after: once with one SearchForTriangulation and one TriangulateMatches call per
// neighbour, once with NewMapPointsBatch (my-slam_amd/host/CreateNewMapPoints.h: one GPU call before the loop, results read at
// each neighbour's turn).  Both run on equal copies of an object graph that tests/test_createnewmappoints_cxx.py writes into the
// case file; afterwards the two graphs must be equal: the new MapPoints in creation order, their positions bit for bit, both
// observations of each, and GetMapPoint of every slot of every key frame.  One run lets CheckNewKeyFrames() turn true before the
// third neighbour.  A neighbour list that names a key frame twice must be refused.
//   createnewmappoints_callsites compile-only      (no GPU: the call expressions compile and link)
//   createnewmappoints_callsites <case file>
// The per-neighbour search is ORB_SLAM2::ORBmatcher::SearchForTriangulation's body (my-slam_amd/host/ORBmatcher.h) on the C ABI:
// that header needs the Tracking thread's Frame and MapPoint as well, which the shims of this test do not carry.
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "CreateNewMapPoints.h"
#include "NewMapPoints.h"

using namespace std;
using namespace ORB_SLAM2;

long unsigned int MapPoint::nNextId = 0;

struct Camera { float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factor; int nlevels; float sf[16], sigma2[16]; };
static_assert(sizeof(Camera) == sizeof(orbm_camera), "the case file stores orbm_camera records");

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

// one key frame record: n, camera, mvKeysUn, mvKeys[i].pt, mvuRight, mvDepth, descriptors, has-MapPoint flags, node id per feature
static KeyFrame *read_keyframe(FILE *f, long unsigned int id)
{
    int32_t n;
    if (!rd(f, &n, 4) || n < 0) return nullptr;
    Camera c;
    vector<orbx_keypoint> kp(n);
    vector<float> xy(2 * (size_t)n), ur(n), depth(n);
    vector<unsigned char> has(n);
    vector<int32_t> node(n);
    KeyFrame *pKF = new KeyFrame(id, n);
    pKF->mDescriptors = cv::Mat(n > 0 ? n : 1, 32, CV_8U);
    if (!rd(f, &c, sizeof(c)) || !rd(f, kp.data(), sizeof(orbx_keypoint) * n) || !rd(f, xy.data(), 8 * (size_t)n) || !rd(f, ur.data(), 4 * (size_t)n) ||
        !rd(f, depth.data(), 4 * (size_t)n) || !rd(f, pKF->mDescriptors.data, 32 * (size_t)n) || !rd(f, has.data(), n) || !rd(f, node.data(), 4 * (size_t)n))
        return nullptr;
    pKF->SetPose(c.Rcw, c.tcw, c.Ow);
    pKF->fx = c.fx; pKF->fy = c.fy; pKF->cx = c.cx; pKF->cy = c.cy; pKF->invfx = c.invfx; pKF->invfy = c.invfy; pKF->mb = c.mb; pKF->mbf = c.mbf;
    pKF->mfScaleFactor = c.scale_factor;
    pKF->mvScaleFactors.assign(c.sf, c.sf + c.nlevels); pKF->mvLevelSigma2.assign(c.sigma2, c.sigma2 + c.nlevels);
    pKF->mvKeys.resize(n); pKF->mvKeysUn.resize(n); pKF->mvuRight = ur; pKF->mvDepth = depth;
    for (int i = 0; i < n; i++) {
        cv::KeyPoint k;
        k.pt.x = kp[i].x; k.pt.y = kp[i].y; k.size = kp[i].size; k.angle = kp[i].angle; k.response = kp[i].response; k.octave = kp[i].octave;
        k.class_id = kp[i].class_id;
        pKF->mvKeysUn[i] = k;
        k.pt.x = xy[2 * i]; k.pt.y = xy[2 * i + 1];
        pKF->mvKeys[i] = k;
        if (node[i] >= 0) pKF->mFeatVec[(DBoW2::NodeId)node[i]].push_back((unsigned int)i);
        if (has[i]) pKF->AddMapPoint(new MapPoint(cv::Mat(3, 1, CV_32F), pKF, nullptr), i);      // a MapPoint from before this key frame's turn
    }
    return pKF;
}

struct World {
    KeyFrame *mpCurrentKeyFrame = nullptr;
    vector<KeyFrame *> vpNeighKFs;
    vector<cv::Mat> vF12;                       // ComputeF12(mpCurrentKeyFrame, vpNeighKFs[i]) stays with the caller: the case file has it
    Map map;
    Map *mpMap = &map;
    list<MapPoint *> mlpRecentAddedMapPoints;
    vector<int> newPerNeighbour;
    int stopBefore = -1, checks = 0;            // CheckNewKeyFrames() turns true at the check before neighbour `stopBefore`
    bool CheckNewKeyFrames() { return checks++ == stopBefore; }
};

static bool read_world(const char *path, World &w)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    int32_t nviews;
    bool ok = rd(f, &nviews, 4) && nviews >= 0 && (w.mpCurrentKeyFrame = read_keyframe(f, 1)) != nullptr;
    for (int v = 0; ok && v < nviews; v++) {
        KeyFrame *pKF2 = read_keyframe(f, 2 + v);
        cv::Mat F12(3, 3, CV_32F);
        float F[9];
        ok = pKF2 && rd(f, F, sizeof(F));
        for (int k = 0; ok && k < 9; k++) F12.at<float>(k / 3, k % 3) = F[k];
        w.vpNeighKFs.push_back(pKF2); w.vF12.push_back(F12);
    }
    fclose(f);
    if (!ok) fprintf(stderr, "short case file\n");
    return ok;
}

// :436-451 over the accepted pairs of one neighbour, in pair order
static void AddNewMapPoints(World &w, KeyFrame *pKF2, const vector<pair<size_t, size_t> > &vMatchedIndices, const vector<unsigned char> &status,
                            const vector<cv::Mat> &x3D)
{
    KeyFrame *mpCurrentKeyFrame = w.mpCurrentKeyFrame;
    Map *mpMap = w.mpMap;
    int nnew = 0;
    const int nmatches = vMatchedIndices.size();
    for (int ikp = 0; ikp < nmatches; ikp++) {
        if (status[ikp] > ORBM_TRI_STEREO2) continue;
        const int idx1 = vMatchedIndices[ikp].first;
        const int idx2 = vMatchedIndices[ikp].second;

        // Triangulation is succesfull
        MapPoint *pMP = new MapPoint(x3D[ikp], mpCurrentKeyFrame, mpMap);

        pMP->AddObservation(mpCurrentKeyFrame, idx1);
        pMP->AddObservation(pKF2, idx2);

        mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
        pKF2->AddMapPoint(pMP, idx2);

        pMP->UpdateNormalAndDepth();

        mpMap->AddMapPoint(pMP);
        w.mlpRecentAddedMapPoints.push_back(pMP);
        nnew++;
    }
    w.newPerNeighbour.push_back(nnew);
}

// ORBmatcher::SearchForTriangulation (my-slam_amd/host/ORBmatcher.h) with mbCheckOrientation == false, on a handle of its own
static bool SearchForTriangulation(orbm_matcher *m, KeyFrame *pKF1, KeyFrame *pKF2, const cv::Mat &F12, vector<pair<size_t, size_t> > &vMatchedPairs,
                                   const bool bOnlyStereo, string &err)
{
    vMatchedPairs.clear();
    const int n1 = pKF1->N, n2 = pKF2->N;
    if (n1 == 0 || n2 == 0) return true;
    vector<orbx_keypoint> kp1, kp2;
    vector<float> xy, ur, depth;
    orbm_detail::FillFeatures(pKF1, kp1, xy, ur, depth);
    orbm_detail::FillFeatures(pKF2, kp2, xy, ur, depth);
    vector<unsigned char> has1(n1), has2(n2);
    for (int i = 0; i < n1; i++) has1[i] = pKF1->GetMapPoint(i) ? 1 : 0;
    for (int i = 0; i < n2; i++) has2[i] = pKF2->GetMapPoint(i) ? 1 : 0;
    vector<int32_t> a0, a1, a2, b0, b1, b2;
    orbm_detail::AppendFeatureVector(pKF1->mFeatVec, a0, a1, a2);
    orbm_detail::AppendFeatureVector(pKF2->mFeatVec, b0, b1, b2);
    float Cw[3], T2w[16] = {0}, F[9];
    const cv::Mat Ow = pKF1->GetCameraCenter(), R = pKF2->GetRotation(), t = pKF2->GetTranslation();
    for (int r = 0; r < 3; r++) {
        Cw[r] = Ow.at<float>(r);
        for (int c = 0; c < 3; c++) { T2w[4 * r + c] = R.at<float>(r, c); F[3 * r + c] = F12.at<float>(r, c); }
        T2w[4 * r + 3] = t.at<float>(r);
    }
    T2w[15] = 1.f;
    vector<int32_t> match(n1, -1);
    int nm = 0;
    if (orbm_search_for_triangulation(m, kp1.data(), pKF1->mDescriptors.ptr<unsigned char>(), n1, has1.data(), pKF1->mvuRight.data(), a0.data(), a1.data(),
                                      a2.data(), (int)a0.size(), kp2.data(), pKF2->mDescriptors.ptr<unsigned char>(), n2, has2.data(), pKF2->mvuRight.data(),
                                      b0.data(), b1.data(), b2.data(), (int)b0.size(), Cw, T2w, pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy, F,
                                      pKF2->mvScaleFactors.data(), pKF2->mvLevelSigma2.data(), (int)pKF2->mvScaleFactors.size(), bOnlyStereo ? 1 : 0, 0,
                                      match.data(), &nm) != ORBX_OK) {
        err = orbm_last_error();
        return false;
    }
    for (int i = 0; i < n1; i++)
        if (match[i] >= 0) vMatchedPairs.push_back(make_pair((size_t)i, (size_t)match[i]));
    return true;
}

// INTEGRATION.md 3h, before: two GPU calls per neighbour
static bool CreateNewMapPoints_PerNeighbour(World &w, orbm_matcher *m, const bool bOnlyStereo, string &err)
{
    KeyFrame *mpCurrentKeyFrame = w.mpCurrentKeyFrame;
    const vector<KeyFrame *> &vpNeighKFs = w.vpNeighKFs;
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
        if (i > 0 && w.CheckNewKeyFrames())
            return true;

        KeyFrame *pKF2 = vpNeighKFs[i];

        // Search matches that fullfil epipolar constraint
        vector<pair<size_t, size_t> > vMatchedIndices;
        if (!SearchForTriangulation(m, mpCurrentKeyFrame, pKF2, w.vF12[i], vMatchedIndices, bOnlyStereo, err)) return false;

        vector<unsigned char> status;
        vector<cv::Mat> x3D;
        if (TriangulateMatches(mpCurrentKeyFrame, pKF2, vMatchedIndices, status, x3D, &err) < 0) return false;      // :288-434
        AddNewMapPoints(w, pKF2, vMatchedIndices, status, x3D);
    }
    return true;
}

// INTEGRATION.md 3h, after: one GPU call for all neighbours, read at each neighbour's turn
static bool CreateNewMapPoints_Batch(World &w, const bool bOnlyStereo, string &err)
{
    KeyFrame *mpCurrentKeyFrame = w.mpCurrentKeyFrame;
    const vector<KeyFrame *> &vpNeighKFs = w.vpNeighKFs;
    NewMapPointsBatch<KeyFrame> batch;
    if (!batch.Search(mpCurrentKeyFrame, vpNeighKFs, w.vF12, bOnlyStereo, &err)) return false;
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
        if (i > 0 && w.CheckNewKeyFrames())
            return true;

        KeyFrame *pKF2 = vpNeighKFs[i];

        vector<pair<size_t, size_t> > vMatchedIndices;
        vector<unsigned char> status;
        vector<cv::Mat> x3D;
        if (batch.Neighbour(i, vMatchedIndices, status, x3D) < 0) { err = "Neighbour() without a Search()"; return false; }
        AddNewMapPoints(w, pKF2, vMatchedIndices, status, x3D);
    }
    return true;
}

// a number for every MapPoint of a world that does not depend on the world: the MapPoints from before by (key frame, slot), the new
// ones by creation order
static map<MapPoint *, long> ordinals(World &w)
{
    map<MapPoint *, long> ord;
    for (size_t k = 0; k < w.map.mvpMapPoints.size(); k++) ord[w.map.mvpMapPoints[k]] = 1000000 + (long)k;
    vector<KeyFrame *> kfs(1, w.mpCurrentKeyFrame);
    kfs.insert(kfs.end(), w.vpNeighKFs.begin(), w.vpNeighKFs.end());
    for (size_t f = 0; f < kfs.size(); f++) {
        const vector<MapPoint *> v = kfs[f]->GetMapPointMatches();
        for (size_t i = 0; i < v.size(); i++)
            if (v[i] && !ord.count(v[i])) ord[v[i]] = -(long)(f * 100000 + i) - 1;
    }
    return ord;
}

static int kf_index(World &w, KeyFrame *pKF)
{
    if (pKF == w.mpCurrentKeyFrame) return 0;
    for (size_t v = 0; v < w.vpNeighKFs.size(); v++)
        if (w.vpNeighKFs[v] == pKF) return 1 + (int)v;
    return -1;
}

static bool same_graph(World &a, World &b)
{
    if (a.newPerNeighbour != b.newPerNeighbour) { fprintf(stderr, "new points per neighbour differ\n"); return false; }
    if (a.map.mvpMapPoints.size() != b.map.mvpMapPoints.size() || a.mlpRecentAddedMapPoints.size() != b.mlpRecentAddedMapPoints.size() ||
        a.map.mvpMapPoints.size() != a.mlpRecentAddedMapPoints.size()) {
        fprintf(stderr, "point counts differ: %zu against %zu\n", a.map.mvpMapPoints.size(), b.map.mvpMapPoints.size());
        return false;
    }
    auto la = a.mlpRecentAddedMapPoints.begin(), lb = b.mlpRecentAddedMapPoints.begin();
    for (size_t k = 0; k < a.map.mvpMapPoints.size(); k++, ++la, ++lb) {
        MapPoint *pa = a.map.mvpMapPoints[k], *pb = b.map.mvpMapPoints[k];
        if (*la != pa || *lb != pb) { fprintf(stderr, "point %zu: list and map disagree\n", k); return false; }
        const cv::Mat xa = pa->GetWorldPos(), xb = pb->GetWorldPos();
        for (int r = 0; r < 3; r++)
            if (memcmp(xa.ptr<float>(r), xb.ptr<float>(r), 4)) { fprintf(stderr, "point %zu: position differs\n", k); return false; }
        const map<KeyFrame *, size_t> oa = pa->GetObservations(), ob = pb->GetObservations();
        if (oa.size() != 2 || ob.size() != 2) { fprintf(stderr, "point %zu: %zu / %zu observations\n", k, oa.size(), ob.size()); return false; }
        map<int, size_t> ra, rb;                  // observations by key-frame role
        for (const auto &o : oa) ra[kf_index(a, o.first)] = o.second;
        for (const auto &o : ob) rb[kf_index(b, o.first)] = o.second;
        if (ra != rb || !ra.count(0)) { fprintf(stderr, "point %zu: observations differ\n", k); return false; }
        if (pa->nNormalUpdatesDone() != 1 || pa->GetReferenceKeyFrame() != a.mpCurrentKeyFrame || pb->GetReferenceKeyFrame() != b.mpCurrentKeyFrame) {
            fprintf(stderr, "point %zu: bookkeeping\n", k);
            return false;
        }
    }
    // every slot of every key frame holds the same MapPoint, or none
    map<MapPoint *, long> orda = ordinals(a), ordb = ordinals(b);
    for (size_t f = 0; f <= a.vpNeighKFs.size(); f++) {
        KeyFrame *ka = f ? a.vpNeighKFs[f - 1] : a.mpCurrentKeyFrame, *kb = f ? b.vpNeighKFs[f - 1] : b.mpCurrentKeyFrame;
        const vector<MapPoint *> va = ka->GetMapPointMatches(), vb = kb->GetMapPointMatches();
        if (va.size() != vb.size()) return false;
        for (size_t i = 0; i < va.size(); i++) {
            if ((va[i] == nullptr) != (vb[i] == nullptr)) { fprintf(stderr, "key frame %zu slot %zu differs\n", f, i); return false; }
            if (va[i] && orda[va[i]] != ordb[vb[i]]) { fprintf(stderr, "key frame %zu slot %zu holds another point\n", f, i); return false; }
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "compile-only")) return 0;
    const bool bOnlyStereo = argc > 2 && !strcmp(argv[2], "only-stereo");
    orbm_matcher *m = nullptr;
    if (orbm_create(&m, 0, 1024, 1024, 1024) != ORBX_OK) { fprintf(stderr, "orbm_create: %s\n", orbm_last_error()); return 1; }
    string err;
    for (int run = 0; run < 2; run++) {          // run 1: CheckNewKeyFrames() turns true before the third neighbour
        World seq, bat;
        if (!read_world(argv[1], seq) || !read_world(argv[1], bat)) return 2;
        seq.stopBefore = bat.stopBefore = run ? 1 : -1;      // the check is made from the second neighbour on: check 1 is the third's
        if (!CreateNewMapPoints_PerNeighbour(seq, m, bOnlyStereo, err)) { fprintf(stderr, "per-neighbour loop: %s\n", err.c_str()); return 1; }
        if (!CreateNewMapPoints_Batch(bat, bOnlyStereo, err)) { fprintf(stderr, "batch loop: %s\n", err.c_str()); return 1; }
        if (!same_graph(seq, bat)) { fprintf(stderr, "run %d: the two object graphs differ\n", run); return 1; }
        if (run && (seq.newPerNeighbour.size() != 2 || seq.vpNeighKFs.size() < 3)) { fprintf(stderr, "the early exit did not happen\n"); return 1; }
        printf("run %d: new MapPoints per neighbour:", run);
        for (int n : seq.newPerNeighbour) printf(" %d", n);
        printf("\n");
        if (run == 0) {                          // a neighbour named twice is refused, with a text, before any GPU work
            vector<KeyFrame *> twice = bat.vpNeighKFs;
            vector<cv::Mat> vF12 = bat.vF12;
            twice.push_back(twice[0]); vF12.push_back(vF12[0]);
            NewMapPointsBatch<KeyFrame> batch;
            string why;
            vector<pair<size_t, size_t> > pairs;
            vector<unsigned char> status;
            vector<cv::Mat> x3D;
            if (batch.Search(bat.mpCurrentKeyFrame, twice, vF12, bOnlyStereo, &why) || why.find("same key frame") == string::npos ||
                batch.Neighbour(0, pairs, status, x3D) != -1) {
                fprintf(stderr, "a duplicated neighbour was not refused (%s)\n", why.c_str());
                return 1;
            }
        }
    }
    orbm_destroy(m);
    printf("createnewmappoints_callsites ok\n");
    return 0;
}
