// localpoints_callsites.cc -- Tracking::SearchLocalPoints (src/Tracking.cc:1150-1200 of WChen09/My-SLAM) twice on the same object
// graph (tests/cxx/localpoints_shims/): once with the body the reference has from :1171 on -- the isInFrustum loop on the host,
// then the matcher, here through the C ABI's orbm_search_by_projection_map on the mTrack* members that loop left -- and once as
// INTEGRATION.md 3i rewrites it, with ORB_SLAM2::SearchLocalPoints (my-slam_amd/host/LocalPoints.h).  Both must leave every
// mbTrackInView, mTrack* member and visible counter and F.mvpMapPoints equal.
//   localpoints_callsites compile-only      0
//   localpoints_callsites <case.bin> <th>   0 when the two graphs are equal; prints nToMatch and the match count
// case.bin (tests/test_localpoints_cxx.py): int32 n, nc, frame id; orbm_frame_view; per MapPoint skip-kind (0: reached, 1: seen in
// this frame, 2: bad), xw, normal, mfMax, mfMin, descriptor, observations; per key point orbx_keypoint, descriptor, uRight, the slot's
// observations (-1: empty).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "LocalPoints.h"

using namespace ORB_SLAM2;
using namespace std;

struct Graph {
    Frame mCurrentFrame;
    vector<MapPoint *> mvpLocalMapPoints;
    vector<MapPoint *> slotPoints;          // the MapPoints the frame's slots hold already
    int nToMatch = 0, nmatches = 0;
};

static bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static bool load(const char *path, Graph &g)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int32_t head[3];
    orbm_frame_view v;
    if (!read_all(f, head, sizeof(head)) || !read_all(f, &v, sizeof(v))) return false;
    const int n = head[0], nc = head[1];
    Frame &F = g.mCurrentFrame;
    F.mnId = (unsigned long)head[2];
    F.SetPose(v.Rcw, v.tcw, v.Ow);
    Frame::fx = v.fx; Frame::fy = v.fy; Frame::cx = v.cx; Frame::cy = v.cy; F.mbf = v.mbf;
    Frame::mnMinX = v.bounds[0]; Frame::mnMaxX = v.bounds[1]; Frame::mnMinY = v.bounds[2]; Frame::mnMaxY = v.bounds[3];
    F.mfLogScaleFactor = v.log_scale_factor; F.mnScaleLevels = v.nlevels;
    F.mvScaleFactors.assign(v.scale_factors, v.scale_factors + v.nlevels);
    vector<uint8_t> kind(n), desc((size_t)n * 32);
    vector<float> xw((size_t)n * 3), nrm((size_t)n * 3), mx(n), mn(n);
    vector<int32_t> obs(n);
    if (!read_all(f, kind.data(), n) || !read_all(f, xw.data(), xw.size() * 4) || !read_all(f, nrm.data(), nrm.size() * 4) ||
        !read_all(f, mx.data(), (size_t)n * 4) || !read_all(f, mn.data(), (size_t)n * 4) || !read_all(f, desc.data(), desc.size()) ||
        !read_all(f, obs.data(), (size_t)n * 4))
        return false;
    for (int i = 0; i < n; i++) {
        MapPoint *p = new MapPoint(&xw[3 * (size_t)i], &nrm[3 * (size_t)i], &desc[32 * (size_t)i], obs[i], mx[i], mn[i]);
        p->mnLastFrameSeen = kind[i] == 1 ? F.mnId : F.mnId - 1;
        p->mbTrackInView = kind[i] == 2;    // a bad point keeps a stale flag from an earlier frame: the matcher must still skip it
        if (kind[i] == 2) p->SetBadFlag();
        g.mvpLocalMapPoints.push_back(p);
    }
    F.mvKeysUn.resize(nc); F.mvuRight.resize(nc); F.mvpMapPoints.assign(nc, static_cast<MapPoint *>(NULL));
    F.mDescriptors = cv::Mat(nc, 32, CV_8U);
    vector<int32_t> slot(nc);
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint layout");
    if (!read_all(f, F.mvKeysUn.data(), (size_t)nc * sizeof(orbx_keypoint)) || !read_all(f, F.mDescriptors.data, (size_t)nc * 32) ||
        !read_all(f, F.mvuRight.data(), (size_t)nc * 4) || !read_all(f, slot.data(), (size_t)nc * 4))
        return false;
    const float zero[3] = {0, 0, 0};
    const unsigned char nodesc[32] = {0};
    for (int i = 0; i < nc; i++)
        if (slot[i] >= 0) {
            MapPoint *p = new MapPoint(zero, zero, nodesc, slot[i], 1.f, 1.f);
            p->mnLastFrameSeen = F.mnId;
            F.mvpMapPoints[i] = p; g.slotPoints.push_back(p);
        }
    fclose(f);
    return true;
}

// src/Tracking.cc:1171-1199 as the reference has it; the matcher call of :1198 goes through the C ABI on the members the loop wrote
static bool SearchLocalPoints_reference(Graph &g, float th, orbm_matcher *m)
{
    Frame &mCurrentFrame = g.mCurrentFrame;
    vector<MapPoint *> &mvpLocalMapPoints = g.mvpLocalMapPoints;
    int nToMatch = 0;
    for (vector<MapPoint *>::iterator vit = mvpLocalMapPoints.begin(), vend = mvpLocalMapPoints.end(); vit != vend; vit++) {
        MapPoint *pMP = *vit;
        if (pMP->mnLastFrameSeen == mCurrentFrame.mnId)
            continue;
        if (pMP->isBad())
            continue;
        if (mCurrentFrame.isInFrustum(pMP, 0.5)) {
            pMP->IncreaseVisible();
            nToMatch++;
        }
    }
    g.nToMatch = nToMatch;
    if (nToMatch > 0) {
        const int n = (int)mvpLocalMapPoints.size(), nc = (int)mCurrentFrame.mvKeysUn.size();
        vector<uint8_t> inView(n, 0), desc((size_t)n * 32);
        vector<float> px(n), py(n), pxr(n), vc(n);
        vector<int32_t> lv(n), obs(n), curObs(nc, -1), match(nc, -1);
        for (int i = 0; i < n; i++) {
            MapPoint *pMP = mvpLocalMapPoints[i];
            if (!pMP->mbTrackInView || pMP->isBad()) continue;          // src/ORBmatcher.cc:56-60
            inView[i] = 1; px[i] = pMP->mTrackProjX; py[i] = pMP->mTrackProjY; pxr[i] = pMP->mTrackProjXR; vc[i] = pMP->mTrackViewCos;
            lv[i] = pMP->mnTrackScaleLevel; obs[i] = pMP->Observations();
            memcpy(&desc[(size_t)i * 32], pMP->GetDescriptor().ptr<unsigned char>(), 32);
        }
        for (int i = 0; i < nc; i++)
            if (mCurrentFrame.mvpMapPoints[i]) curObs[i] = mCurrentFrame.mvpMapPoints[i]->Observations();
        const orbx_keypoint *kps = reinterpret_cast<const orbx_keypoint *>(mCurrentFrame.mvKeysUn.data());
        if (orbm_grid_build(m, kps, nc, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY) != ORBX_OK) return false;
        const bool stereo = mCurrentFrame.mbf > 0;
        if (orbm_search_by_projection_map(m, n, inView.data(), px.data(), py.data(), stereo ? pxr.data() : NULL, lv.data(), vc.data(), desc.data(),
                                          obs.data(), mCurrentFrame.mvScaleFactors.data(), mCurrentFrame.mnScaleLevels, kps,
                                          mCurrentFrame.mDescriptors.ptr<unsigned char>(), stereo ? mCurrentFrame.mvuRight.data() : NULL, nc, th,
                                          0.8f, curObs.data(), match.data(), &g.nmatches) != ORBX_OK)
            return false;
        for (int i = 0; i < nc; i++)
            if (match[i] >= 0) mCurrentFrame.mvpMapPoints[i] = mvpLocalMapPoints[match[i]];
    }
    return true;
}

// the same lines as INTEGRATION.md 3i leaves them
static bool SearchLocalPoints_adapter(Graph &g, float th)
{
    Frame &mCurrentFrame = g.mCurrentFrame;
    vector<MapPoint *> &mvpLocalMapPoints = g.mvpLocalMapPoints;
    std::string err;
    const int nmatches = ORB_SLAM2::SearchLocalPoints(mCurrentFrame, mvpLocalMapPoints, th, 0.8f, &err);
    if (nmatches < 0) { cerr << "SearchLocalPoints: " << err << endl; return false; }
    g.nmatches = nmatches;
    g.nToMatch = 0;
    for (size_t i = 0; i < mvpLocalMapPoints.size(); i++)
        g.nToMatch += mvpLocalMapPoints[i]->mbTrackInView && !mvpLocalMapPoints[i]->isBad() && mvpLocalMapPoints[i]->mnLastFrameSeen != mCurrentFrame.mnId;
    return true;
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a != a && b != b); }

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "compile-only")) return 0;
    if (argc < 3) { fprintf(stderr, "usage: %s <case.bin> <th> | compile-only\n", argv[0]); return 2; }
    const float th = (float)atof(argv[2]);
    Graph a, b;
    if (!load(argv[1], a) || !load(argv[1], b)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    orbm_matcher *m = NULL;
    if (orbm_create(&m, 0, 8192, 8192, 1 << 21) != ORBX_OK) { fprintf(stderr, "orbm_create: %s\n", orbm_last_error()); return 2; }
    if (!SearchLocalPoints_reference(a, th, m)) { fprintf(stderr, "reference path: %s\n", orbm_last_error()); return 2; }
    orbm_destroy(m);
    if (!SearchLocalPoints_adapter(b, th)) return 2;
    int bad = 0;
    for (size_t i = 0; i < a.mvpLocalMapPoints.size(); i++) {
        const MapPoint *p = a.mvpLocalMapPoints[i], *q = b.mvpLocalMapPoints[i];
        const bool same = p->mbTrackInView == q->mbTrackInView && p->mnVisible == q->mnVisible && same_bits(p->mTrackProjX, q->mTrackProjX) &&
                          same_bits(p->mTrackProjY, q->mTrackProjY) && same_bits(p->mTrackProjXR, q->mTrackProjXR) &&
                          p->mnTrackScaleLevel == q->mnTrackScaleLevel && same_bits(p->mTrackViewCos, q->mTrackViewCos);
        if (!same && bad++ < 5)
            printf("MapPoint %zu differs: in view %d / %d, visible %d / %d, level %d / %d, u %.9g / %.9g\n", i, p->mbTrackInView, q->mbTrackInView,
                   p->mnVisible, q->mnVisible, p->mnTrackScaleLevel, q->mnTrackScaleLevel, p->mTrackProjX, q->mTrackProjX);
    }
    for (size_t i = 0; i < a.mCurrentFrame.mvpMapPoints.size(); i++) {
        // a slot holds the frame's own earlier point, a local MapPoint (compare by index), or nothing
        const MapPoint *p = a.mCurrentFrame.mvpMapPoints[i], *q = b.mCurrentFrame.mvpMapPoints[i];
        long ip = -1, iq = -1;
        for (size_t k = 0; k < a.mvpLocalMapPoints.size(); k++) { if (a.mvpLocalMapPoints[k] == p) ip = (long)k; if (b.mvpLocalMapPoints[k] == q) iq = (long)k; }
        if ((p == NULL) != (q == NULL) || ip != iq) { if (bad++ < 5) printf("slot %zu differs: MapPoint %ld / %ld\n", i, ip, iq); }
    }
    if (a.nToMatch != b.nToMatch || a.nmatches != b.nmatches) { printf("nToMatch %d / %d, matches %d / %d\n", a.nToMatch, b.nToMatch, a.nmatches, b.nmatches); bad++; }
    printf("nToMatch %d, %d matches, %d differences\n", a.nToMatch, a.nmatches, bad);
    return bad ? 1 : 0;
}
