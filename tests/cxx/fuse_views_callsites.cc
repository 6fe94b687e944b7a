// fuse_views_callsites.cc -- LocalMapping::SearchInNeighbors (src/LocalMapping.cc:484-516 of WChen09/My-SLAM) written twice on the
// drop-in class of my-slam_amd/host/ORBmatcher.h: with the reference's own expressions (one matcher.Fuse(pKFi,vpMapPointMatches)
// per target key frame, then matcher.Fuse(mpCurrentKeyFrame,vpFuseCandidates)) and as INTEGRATION.md section 3k rewrites it (one
// matcher.Fuse(vpTargetKFs,vpMapPointMatches), then matcher.Fuse(vector<KeyFrame*>(1,mpCurrentKeyFrame),vpFuseCandidates)).  Both
// run on their own copy of one synthetic map; afterwards the two object graphs must be identical: bad flags, replaced-by links,
// the observations and Observations() of every MapPoint, its descriptor, the slots of every key frame; and the overload's per-view
// counts and return value must be the single calls' return values.
// The classes are the minimal ones of tests/cxx/fuse_shims/ (an ORB-SLAM2 tree brings its own): their MapPoint::Replace recomputes
// the survivor's descriptor from its observations as the reference's does, which is what makes the loop order-dependent, and their
// KeyFrame::GetFeaturesInArea serves the overload's host re-selection.
// The key frames of a map live in one block in creation order, so the std::map<KeyFrame*, size_t> of both copies iterate alike.
// usage: fuse_views_callsites              both loops on the GPU, compared
//        fuse_views_callsites no-device    without a HIP device: the overload returns 0 and touches nothing
//        fuse_views_callsites compile-only
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>
#include "ORBmatcher.h"

using namespace std;
using namespace ORB_SLAM2;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 17) {}
    uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }
    float uni() { return (float)(next() & 0xFFFFFF) / 16777216.f; }
    float range(float a, float b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    float noise(float s_) { return s_ * (uni() + uni() + uni() + uni() - 2.f); }
};

static const int W = 640, H = 480, NLEVELS = 8;
static const float FX = 500.f, FY = 500.f, CX = 320.f, CY = 240.f, BF = 40.f;

struct Desc { unsigned char b[32]; };
static Desc random_desc(Rng &r) { Desc d; for (int k = 0; k < 32; k++) d.b[k] = (unsigned char)r.below(256); return d; }
static Desc flipped(Rng &r, Desc d, int nbits) { for (int k = 0; k < nbits; k++) { const int bit = r.below(256); d.b[bit >> 3] ^= (unsigned char)(1 << (bit & 7)); } return d; }

struct KfSpec {                                  // a key frame before it is constructed (its feature members are const)
    float C[3];                                  // camera centre; Rcw = I, tcw = -C
    vector<cv::KeyPoint> keys;
    vector<float> uRight;
    vector<Desc> desc;
    int add(float x, float y, int octave, float ur, const Desc &d)
    {
        cv::KeyPoint kp; kp.pt.x = x; kp.pt.y = y; kp.octave = octave; kp.angle = 0.f; kp.size = 31.f;
        keys.push_back(kp); uRight.push_back(ur); desc.push_back(d);
        return (int)keys.size() - 1;
    }
};
struct MpSpec { float X[3], n[3], mfMax, mfMin; Desc d; vector<pair<int, int> > obs; };   // obs: (key frame, slot)

struct World {
    KeyFrame *kfs = nullptr;
    int nkf = 0, ntargets = 0;
    vector<MapPoint *> mps;
    vector<KeyFrame *> vpTargetKFs;
    KeyFrame *mpCurrentKeyFrame = nullptr;
};

// key frame 0 = mpCurrentKeyFrame at the origin, 1 .. ntargets = the targets (the last one has no feature), then two key frames
// outside the loop that hold further observations
static World build(uint64_t seed, int ntargets, int npoints)
{
    Rng r(seed);
    vector<float> sf(NLEVELS, 1.f), inv(NLEVELS, 1.f);
    for (int l = 1; l < NLEVELS; l++) sf[l] = sf[l - 1] * 1.2f;
    for (int l = 0; l < NLEVELS; l++) inv[l] = 1.0f / (sf[l] * sf[l]);
    const float logSf = logf(1.2f);
    const int nkf = 1 + ntargets + 2, home0 = 1 + ntargets;
    vector<KfSpec> ks(nkf);
    for (int k = 0; k < nkf; k++) { ks[k].C[0] = k == 0 ? 0.f : r.noise(0.35f); ks[k].C[1] = k == 0 ? 0.f : r.noise(0.1f); ks[k].C[2] = k == 0 ? 0.f : r.noise(0.2f); }
    vector<MpSpec> ms;
    auto home_obs = [&](MpSpec &m, int count) {
        for (int c = 0; c < count; c++) {
            const int h = home0 + c % 2;
            m.obs.push_back(make_pair(h, ks[h].add(r.range(0, W), r.range(0, H), r.below(NLEVELS), r.uni() < 0.5f ? r.range(0, W) : -1.f, flipped(r, m.d, r.below(8)))));
        }
    };
    // the MapPoints of the current key frame
    for (int j = 0; j < npoints; j++) {
        MpSpec m;
        const float z = r.range(3.f, 25.f), u = r.range(20.f, W - 20.f), v = r.range(20.f, H - 20.f);
        m.X[0] = (u - CX) * z / FX; m.X[1] = (v - CY) * z / FY; m.X[2] = z;
        const float dist = sqrtf(m.X[0] * m.X[0] + m.X[1] * m.X[1] + m.X[2] * m.X[2]);
        for (int k = 0; k < 3; k++) m.n[k] = m.X[k] / dist;
        const int octave = r.below(4);
        m.mfMax = dist * sf[octave]; m.mfMin = m.mfMax / sf[NLEVELS - 1];
        m.d = random_desc(r);
        m.obs.push_back(make_pair(0, ks[0].add(u, v, octave, r.uni() < 0.6f ? u - BF / z : -1.f, flipped(r, m.d, r.below(6)))));
        home_obs(m, 1 + r.below(2));
        ms.push_back(m);
    }
    for (int c = 0; c < 40; c++) ks[0].add(r.range(0, W), r.range(0, H), r.below(NLEVELS), -1.f, random_desc(r));      // features without a MapPoint
    // the targets: where the points project, a key point that holds the point itself, a foreign MapPoint, or nothing
    for (int t = 1; t < ntargets; t++) {                                   // the last target stays empty
        KfSpec &K = ks[t];
        for (int j = 0; j < npoints; j++) {
            if (r.uni() > 0.7f) continue;
            const float pc[3] = {ms[j].X[0] - K.C[0], ms[j].X[1] - K.C[1], ms[j].X[2] - K.C[2]};
            if (pc[2] < 0.5f) continue;
            const float u = FX * pc[0] / pc[2] + CX, v = FY * pc[1] / pc[2] + CY;
            if (u < 5 || u > W - 5 || v < 5 || v > H - 5) continue;
            const float dist = sqrtf(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
            int level = (int)ceilf(logf(ms[j].mfMax / dist) / logSf);
            level = min(max(level, 0), NLEVELS - 1);
            const int octave = max(level - r.below(2), 0);
            const Desc d = flipped(r, ms[j].d, r.below(26));
            const float ur = r.uni() < 0.5f ? u - BF / pc[2] + r.noise(0.4f) : -1.f;
            const int slot = K.add(u + r.noise(0.7f), v + r.noise(0.7f), octave, ur, d);
            const float what = r.uni();
            if (what < 0.2f) ms[j].obs.push_back(make_pair(t, slot));
            else if (what < 0.6f) {
                MpSpec f = ms[j];
                f.obs.clear();
                f.d = d;
                f.obs.push_back(make_pair(t, slot));
                home_obs(f, r.below(5));
                ms.push_back(f);
            }
        }
        for (int c = 0; c < 60; c++) K.add(r.range(0, W), r.range(0, H), r.below(NLEVELS), r.uni() < 0.5f ? r.range(0, W) : -1.f, random_desc(r));
    }
    // construction
    World w;
    w.nkf = nkf; w.ntargets = ntargets;
    w.kfs = static_cast<KeyFrame *>(::operator new(sizeof(KeyFrame) * (size_t)nkf));
    Frame::mnMinX = 0.f; Frame::mnMaxX = (float)W; Frame::mnMinY = 0.f; Frame::mnMaxY = (float)H;
    Frame::mfGridElementWidthInv = 64.f / (Frame::mnMaxX - Frame::mnMinX); Frame::mfGridElementHeightInv = 48.f / (Frame::mnMaxY - Frame::mnMinY);
    for (int k = 0; k < nkf; k++) {
        const int n = (int)ks[k].keys.size();
        cv::Mat D(max(n, 1), 32, CV_8U);
        for (int i = 0; i < n; i++) memcpy(D.ptr<unsigned char>(i), ks[k].desc[i].b, 32);
        KeyFrame *kf = new (&w.kfs[k]) KeyFrame(100 + k, ks[k].keys, ks[k].uRight, D, FX, FY, CX, CY, BF, Frame::mfGridElementWidthInv,
                                                Frame::mfGridElementHeightInv, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY, sf, inv, logSf);
        cv::Mat T(4, 4, CV_32F), Ow(3, 1, CV_32F);
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) T.at<float>(a, b) = a == b ? 1.f : 0.f;
        for (int a = 0; a < 3; a++) { T.at<float>(a, 3) = -ks[k].C[a]; Ow.at<float>(a) = ks[k].C[a]; }
        kf->SetPose(T); kf->SetCameraCenter(Ow);
    }
    MapPoint::nNextId = 0;
    for (size_t j = 0; j < ms.size(); j++) {
        cv::Mat X(3, 1, CV_32F), N(3, 1, CV_32F), d(1, 32, CV_8U);
        for (int a = 0; a < 3; a++) { X.at<float>(a) = ms[j].X[a]; N.at<float>(a) = ms[j].n[a]; }
        memcpy(d.ptr<unsigned char>(), ms[j].d.b, 32);
        MapPoint *p = new MapPoint(X, N, d, ms[j].mfMin, ms[j].mfMax);
        for (size_t o = 0; o < ms[j].obs.size(); o++) {
            KeyFrame *kf = &w.kfs[ms[j].obs[o].first];
            p->AddObservation(kf, ms[j].obs[o].second);
            kf->AddMapPoint(p, ms[j].obs[o].second);
        }
        if (j % 37 == 5) p->SetBadFlag();                                  // a bad point that is still in the current key frame's list
        w.mps.push_back(p);
    }
    w.mpCurrentKeyFrame = &w.kfs[0];
    for (int t = 1; t <= ntargets; t++) w.vpTargetKFs.push_back(&w.kfs[t]);
    return w;
}

// everything the loops can write, as text
static vector<string> graph(const World &w)
{
    map<MapPoint *, int> id;
    for (size_t j = 0; j < w.mps.size(); j++) id[w.mps[j]] = (int)j;
    vector<string> out;
    char buf[256];
    for (size_t j = 0; j < w.mps.size(); j++) {
        MapPoint *p = w.mps[j];
        string s;
        snprintf(buf, sizeof buf, "mp %zu bad %d replaced %d nobs %d obs", j, (int)p->isBad(), p->GetReplaced() ? id[p->GetReplaced()] : -1, p->Observations());
        s = buf;
        const map<KeyFrame *, size_t> obs = p->GetObservations();
        for (map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) { snprintf(buf, sizeof buf, " %d:%zu", (int)(it->first - w.kfs), it->second); s += buf; }
        s += " desc ";
        const cv::Mat d = p->GetDescriptor();
        for (int k = 0; k < 32; k++) { snprintf(buf, sizeof buf, "%02x", d.ptr<unsigned char>()[k]); s += buf; }
        out.push_back(s);
    }
    for (int k = 0; k < w.nkf; k++) {
        string s = "kf " + to_string(k) + " slots";
        const vector<MapPoint *> v = w.kfs[k].GetMapPointMatches();
        for (size_t i = 0; i < v.size(); i++) s += " " + to_string(v[i] ? id[v[i]] : -1);
        out.push_back(s);
    }
    return out;
}

// src/LocalMapping.cc:494-514 with the reference's expressions
static vector<MapPoint *> fuse_candidates(const vector<KeyFrame *> &vpTargetKFs, const vector<MapPoint *> &vpMapPointMatches, KeyFrame *mpCurrentKeyFrame)
{
    vector<MapPoint*> vpFuseCandidates;
    vpFuseCandidates.reserve(vpTargetKFs.size()*vpMapPointMatches.size());

    for(vector<KeyFrame*>::const_iterator vitKF=vpTargetKFs.begin(), vendKF=vpTargetKFs.end(); vitKF!=vendKF; vitKF++)
    {
        KeyFrame* pKFi = *vitKF;

        vector<MapPoint*> vpMapPointsKFi = pKFi->GetMapPointMatches();

        for(vector<MapPoint*>::iterator vitMP=vpMapPointsKFi.begin(), vendMP=vpMapPointsKFi.end(); vitMP!=vendMP; vitMP++)
        {
            MapPoint* pMP = *vitMP;
            if(!pMP)
                continue;
            if(pMP->isBad() || pMP->mnFuseCandidateForKF == mpCurrentKeyFrame->mnId)
                continue;
            pMP->mnFuseCandidateForKF = mpCurrentKeyFrame->mnId;
            vpFuseCandidates.push_back(pMP);
        }
    }
    return vpFuseCandidates;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    const uint64_t seed = 7;
    const int ntargets = 7, npoints = 180;

    if (argc > 1 && !strcmp(argv[1], "no-device")) {
        orbm_matcher *probe = nullptr;
        if (orbm_create(&probe, 0, 64, 64, 64) == ORBX_OK) { orbm_destroy(probe); printf("fuse_views_callsites: a device is present, nothing to check\n"); return 0; }
        World w = build(seed, ntargets, npoints), fresh = build(seed, ntargets, npoints);
        ORBmatcher matcher;
        vector<MapPoint*> vpMapPointMatches = w.mpCurrentKeyFrame->GetMapPointMatches();
        vector<int> vnFused(3, 77);
        int nReselected = 77;
        const int n = matcher.Fuse(w.vpTargetKFs,vpMapPointMatches,3.0,&vnFused,&nReselected);
        bool same = n == 0 && nReselected == 0 && (int)vnFused.size() == ntargets && graph(w) == graph(fresh);
        for (size_t v = 0; v < vnFused.size(); v++) same = same && vnFused[v] == 0;
        printf("fuse_views_callsites no-device: returned %d, graph %s\n", n, same ? "untouched" : "FAILED");
        return same ? 0 : 1;
    }

    int nfail = 0;
    // ---- A: the reference's loop ----
    World a = build(seed, ntargets, npoints);
    vector<int> singles;
    int reverseA = 0;
    {
        const vector<KeyFrame*> &vpTargetKFs = a.vpTargetKFs;
        KeyFrame *mpCurrentKeyFrame = a.mpCurrentKeyFrame;
        // Search matches by projection from current KF in target KFs
        ORBmatcher matcher;
        vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
        for(vector<KeyFrame*>::const_iterator vit=vpTargetKFs.begin(), vend=vpTargetKFs.end(); vit!=vend; vit++)
        {
            KeyFrame* pKFi = *vit;

            singles.push_back(matcher.Fuse(pKFi,vpMapPointMatches));
        }
        // Search matches by projection from target KFs in current KF
        vector<MapPoint*> vpFuseCandidates = fuse_candidates(vpTargetKFs, vpMapPointMatches, mpCurrentKeyFrame);
        reverseA = matcher.Fuse(mpCurrentKeyFrame,vpFuseCandidates);
        if (!matcher.LastError().empty()) { printf("FAILED: %s\n", matcher.LastError().c_str()); return 1; }
    }
    // ---- B: the loop of INTEGRATION.md section 3k ----
    World b = build(seed, ntargets, npoints);
    vector<int> vnFused, vnReverse;
    int forwardB = 0, reverseB = 0, nReselected = 0, nReselectedReverse = 0;
    {
        const vector<KeyFrame*> &vpTargetKFs = b.vpTargetKFs;
        KeyFrame *mpCurrentKeyFrame = b.mpCurrentKeyFrame;
        ORBmatcher matcher;
        vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
        forwardB = matcher.Fuse(vpTargetKFs,vpMapPointMatches,3.0,&vnFused,&nReselected);
        vector<MapPoint*> vpFuseCandidates = fuse_candidates(vpTargetKFs, vpMapPointMatches, mpCurrentKeyFrame);
        reverseB = matcher.Fuse(vector<KeyFrame*>(1,mpCurrentKeyFrame),vpFuseCandidates,3.0,&vnReverse,&nReselectedReverse);
        if (!matcher.LastError().empty()) { printf("FAILED: %s\n", matcher.LastError().c_str()); return 1; }
    }
    int sumA = 0;
    printf("per target:");
    for (size_t v = 0; v < singles.size(); v++) { printf(" %d/%d", singles[v], v < vnFused.size() ? vnFused[v] : -1); sumA += singles[v]; }
    printf("\n");
    if (vnFused != singles) { printf("FAILED: per-view counts differ\n"); nfail++; }
    if (forwardB != sumA) { printf("FAILED: forward return value %d, single calls %d\n", forwardB, sumA); nfail++; }
    if (reverseB != reverseA || vnReverse.size() != 1 || vnReverse[0] != reverseA) { printf("FAILED: reverse half %d / %d\n", reverseB, reverseA); nfail++; }
    const vector<string> ga = graph(a), gb = graph(b), g0 = graph(build(seed, ntargets, npoints));
    int ndiff = 0, nchanged = 0;
    for (size_t i = 0; i < ga.size(); i++) {
        if (ga[i] != gb[i] && ndiff++ < 5) printf("FAILED: graphs differ\n  A %s\n  B %s\n", ga[i].c_str(), gb[i].c_str());
        nchanged += ga[i] != g0[i];
    }
    nfail += ndiff;
    printf("forward fused %d, reverse fused %d, reselected %d + %d, graph lines changed by the loop %d of %zu\n", forwardB, reverseB, nReselected,
           nReselectedReverse, nchanged, ga.size());
    if (nfail == 0) printf("fuse_views_callsites ok\n");
    return nfail ? 1 : 0;
}
