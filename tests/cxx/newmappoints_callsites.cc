// newmappoints_callsites.cc -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:209-454) for one neighbour, written as
// INTEGRATION.md 3h shows it: :288-434 replaced by one TriangulateMatches call, the bookkeeping of :436-451 over the accepted
// matches in match order, the ComputeDistinctiveDescriptors calls collected into the one batched call of 3g.  The resulting
// object graph is compared with a replay of :436-451 over the accepted list and positions of tests/triangulation_oracle.py, which
// tests/test_newmappoints_cxx.py writes into the case file together with the two key frames.
//   newmappoints_callsites compile-only      (no GPU: the call expressions compile and link)
//   newmappoints_callsites <case file>
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "MapPointDescriptors.h"
#include "NewMapPoints.h"

using namespace std;
using namespace ORB_SLAM2;

long unsigned int MapPoint::nNextId = 0;

struct Camera { float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factor; int nlevels; float sf[16], sigma2[16]; };
static_assert(sizeof(Camera) == sizeof(orbm_camera), "the case file stores orbm_camera records");

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static KeyFrame *read_keyframe(FILE *f, long unsigned int id, int n)
{
    Camera c;
    vector<orbx_keypoint> kp(n);
    vector<float> xy(2 * (size_t)n), ur(n), depth(n);
    KeyFrame *pKF = new KeyFrame(id, n);
    pKF->mDescriptors = cv::Mat(n > 0 ? n : 1, 32, CV_8U);
    if (!rd(f, &c, sizeof(c)) || !rd(f, kp.data(), sizeof(orbx_keypoint) * n) || !rd(f, xy.data(), 8 * (size_t)n) || !rd(f, ur.data(), 4 * (size_t)n) ||
        !rd(f, depth.data(), 4 * (size_t)n) || !rd(f, pKF->mDescriptors.data, 32 * (size_t)n))
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
    }
    return pKF;
}

struct World {
    KeyFrame *mpCurrentKeyFrame = nullptr, *pKF2 = nullptr;
    Map map;
    Map *mpMap = &map;
    list<MapPoint *> mlpRecentAddedMapPoints;
    int nnew = 0;
};

// INTEGRATION.md 3h
static int CreateNewMapPoints(World &w, const vector<pair<size_t, size_t> > &vMatchedIndices, vector<unsigned char> &status, string &err)
{
    KeyFrame *mpCurrentKeyFrame = w.mpCurrentKeyFrame, *pKF2 = w.pKF2;
    Map *mpMap = w.mpMap;
    vector<MapPoint *> vpNewMapPoints;
    vector<cv::Mat> x3D;
    if (TriangulateMatches(mpCurrentKeyFrame, pKF2, vMatchedIndices, status, x3D, &err) < 0) return -1;      // :288-434
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

        vpNewMapPoints.push_back(pMP);                     // pMP->ComputeDistinctiveDescriptors(); :444, batched below

        pMP->UpdateNormalAndDepth();

        mpMap->AddMapPoint(pMP);
        w.mlpRecentAddedMapPoints.push_back(pMP);

        w.nnew++;
    }
    if (ComputeDistinctiveDescriptors(vpNewMapPoints, &err) < 0) return -1;
    return w.nnew;
}

// :436-451 replayed over the oracle's accepted list; the descriptor of a point with two observations is the first row in the
// iteration order of its mObservations (src/MapPoint.cc:261-301: both medians are 0, the first wins)
static void Replay(World &w, const vector<pair<size_t, size_t> > &vMatchedIndices, const vector<unsigned char> &status, const vector<float> &x3d)
{
    for (size_t ikp = 0; ikp < vMatchedIndices.size(); ikp++) {
        if (status[ikp] > ORBM_TRI_STEREO2) continue;
        cv::Mat p(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) p.at<float>(r) = x3d[3 * ikp + r];
        MapPoint *pMP = new MapPoint(p, w.mpCurrentKeyFrame, w.mpMap);
        pMP->AddObservation(w.mpCurrentKeyFrame, vMatchedIndices[ikp].first);
        pMP->AddObservation(w.pKF2, vMatchedIndices[ikp].second);
        w.mpCurrentKeyFrame->AddMapPoint(pMP, vMatchedIndices[ikp].first);
        w.pKF2->AddMapPoint(pMP, vMatchedIndices[ikp].second);
        const map<KeyFrame *, size_t> obs = pMP->GetObservations();
        pMP->SetDescriptor(obs.begin()->first->mDescriptors.row((int)obs.begin()->second));
        pMP->UpdateNormalAndDepth();
        w.mpMap->AddMapPoint(pMP);
        w.mlpRecentAddedMapPoints.push_back(pMP);
        w.nnew++;
    }
}

static bool same_graph(World &a, World &b)
{
    if (a.nnew != b.nnew || a.map.mvpMapPoints.size() != b.map.mvpMapPoints.size() || a.mlpRecentAddedMapPoints.size() != b.mlpRecentAddedMapPoints.size()) {
        fprintf(stderr, "point counts differ: %d / %zu against %d / %zu\n", a.nnew, a.map.mvpMapPoints.size(), b.nnew, b.map.mvpMapPoints.size());
        return false;
    }
    auto la = a.mlpRecentAddedMapPoints.begin(), lb = b.mlpRecentAddedMapPoints.begin();
    for (size_t k = 0; k < a.map.mvpMapPoints.size(); k++, ++la, ++lb) {
        MapPoint *pa = a.map.mvpMapPoints[k], *pb = b.map.mvpMapPoints[k];
        if (*la != pa || *lb != pb) { fprintf(stderr, "point %zu: list and map disagree\n", k); return false; }
        if (memcmp(pa->GetWorldPos().data, pb->GetWorldPos().data, 4) || memcmp(pa->GetWorldPos().ptr<float>(1), pb->GetWorldPos().ptr<float>(1), 4) ||
            memcmp(pa->GetWorldPos().ptr<float>(2), pb->GetWorldPos().ptr<float>(2), 4)) { fprintf(stderr, "point %zu: position differs\n", k); return false; }
        const map<KeyFrame *, size_t> oa = pa->GetObservations(), ob = pb->GetObservations();
        if (oa.size() != 2 || ob.size() != 2) { fprintf(stderr, "point %zu: %zu / %zu observations\n", k, oa.size(), ob.size()); return false; }
        if (oa.at(a.mpCurrentKeyFrame) != ob.at(b.mpCurrentKeyFrame) || oa.at(a.pKF2) != ob.at(b.pKF2)) { fprintf(stderr, "point %zu: observations differ\n", k); return false; }
        if (a.mpCurrentKeyFrame->GetMapPoint(oa.at(a.mpCurrentKeyFrame)) == nullptr || a.pKF2->GetMapPoint(oa.at(a.pKF2)) == nullptr) { fprintf(stderr, "point %zu: missing in a key frame\n", k); return false; }
        if (pa->nNormalUpdatesDone() != 1 || pa->GetReferenceKeyFrame() != a.mpCurrentKeyFrame) { fprintf(stderr, "point %zu: bookkeeping\n", k); return false; }
        // the descriptor is one of the two observations' rows; which one depends on the pointer order of the two key frames in
        // each world, so it is compared by key-frame role
        const cv::Mat da = pa->GetDescriptor(), db = pb->GetDescriptor();
        if (da.empty() || db.empty()) { fprintf(stderr, "point %zu: no descriptor\n", k); return false; }
        KeyFrame *fa = oa.begin()->first;
        const cv::Mat want = fa->mDescriptors.row((int)oa.begin()->second);
        if (memcmp(da.data, want.data, 32)) { fprintf(stderr, "point %zu: descriptor is not the first observation's row\n", k); return false; }
    }
    // every slot of both key frames: the same match's point, or none
    for (int side = 0; side < 2; side++) {
        KeyFrame *ka = side ? a.pKF2 : a.mpCurrentKeyFrame, *kb = side ? b.pKF2 : b.mpCurrentKeyFrame;
        const vector<MapPoint *> va = ka->GetMapPointMatches(), vb = kb->GetMapPointMatches();
        for (size_t i = 0; i < va.size(); i++) {
            if ((va[i] == nullptr) != (vb[i] == nullptr)) { fprintf(stderr, "key frame %d slot %zu differs\n", side + 1, i); return false; }
            if (va[i] && va[i]->mnId - a.map.mvpMapPoints[0]->mnId != vb[i]->mnId - b.map.mvpMapPoints[0]->mnId) { fprintf(stderr, "key frame %d slot %zu holds another point\n", side + 1, i); return false; }
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "compile-only")) return 0;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[3];
    if (!rd(f, head, sizeof(head))) return 2;
    const int n1 = head[0], n2 = head[1], n = head[2];
    World lib, ref;
    lib.mpCurrentKeyFrame = read_keyframe(f, 1, n1); lib.pKF2 = read_keyframe(f, 2, n2);
    if (!lib.mpCurrentKeyFrame || !lib.pKF2) { fprintf(stderr, "short case file\n"); return 2; }
    vector<int32_t> pairs(2 * (size_t)n);
    vector<unsigned char> oracle_status(n);
    vector<float> oracle_x3d(3 * (size_t)n);
    if (!rd(f, pairs.data(), 8 * (size_t)n) || !rd(f, oracle_status.data(), n) || !rd(f, oracle_x3d.data(), 12 * (size_t)n)) { fprintf(stderr, "short case file\n"); return 2; }
    rewind(f);
    if (!rd(f, head, sizeof(head))) return 2;
    ref.mpCurrentKeyFrame = read_keyframe(f, 1, n1); ref.pKF2 = read_keyframe(f, 2, n2);
    fclose(f);
    vector<pair<size_t, size_t> > vMatchedIndices(n);
    for (int k = 0; k < n; k++) vMatchedIndices[k] = make_pair((size_t)pairs[2 * k], (size_t)pairs[2 * k + 1]);

    vector<unsigned char> status;
    string err;
    const int nnew = CreateNewMapPoints(lib, vMatchedIndices, status, err);
    if (nnew < 0) { fprintf(stderr, "CreateNewMapPoints: %s\n", err.c_str()); return 1; }
    if (status != oracle_status) { fprintf(stderr, "statuses differ from the oracle's\n"); return 1; }
    Replay(ref, vMatchedIndices, oracle_status, oracle_x3d);
    if (!same_graph(lib, ref)) return 1;
    printf("newmappoints_callsites ok: %d matches, %d new MapPoints\n", n, nnew);
    return 0;
}
