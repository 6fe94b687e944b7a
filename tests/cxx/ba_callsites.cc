// ba_callsites.cc -- Optimizer::GlobalBundleAdjustemnt / BundleAdjustment of my-slam_amd/host/PnPsolver.h at their call sites: the
// lines src/Tracking.cc:695 and src/LoopClosing.cc:651 verbatim, on the classes of tests/cxx/ba_shims/.  A small map goes through
// gather, host call and scatter; the object graph after it must be what the flat call orbp_bundle_adjustment dictates for the same
// gather, written to the members the reference writes for nLoopKF == 0 and nLoopKF != 0, and to no others.
//   ba_callsites compile-only        nothing runs
//   ba_callsites host                both lines as written (host path), against the flat call on a second, identical graph
// Built with -DBA_CALLSITES_STANDALONE (tests/test_ba_cxx.py) it links orbp_ba.cc, orbp_lba.cc and orbp.cc instead of the library
// and runs under AddressSanitizer and UBSan: the gather, the host solver and the scatter, host code only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>
#include "KeyFrame.h"
#include "PnPsolver.h"

#ifdef BA_CALLSITES_STANDALONE
// the handle overloads name these; with a NULL matcher they are never called
extern "C" int orbm_bundle_adjustment(orbm_matcher *, const orbp_lba_problem *, int, int, float *, float *, const volatile uint8_t *, orbp_ba_stats *) { abort(); }
extern "C" const char *orbm_last_error(void) { return ""; }
#endif

using namespace ORB_SLAM2;
using namespace std;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Rng {                                    // a fixed generator: the graphs of a run are built from the same draws
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 88172645463325252ull) {}
    double uniform() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; }
    double uniform(double a, double b) { return a + (b - a) * uniform(); }
    double normal() { double v = 0; for (int i = 0; i < 12; i++) v += uniform(); return v - 6.0; }
};

struct World {
    vector<unique_ptr<KeyFrame>> kfs;
    vector<unique_ptr<MapPoint>> mps;
    Map map;
};

// 7 key frames side by side looking down z, in the map in the order of ids 3, 0, 5, 9 (bad), 4, 1; id 2 is good but not in the
// map (an observation of it counts towards nEdges, since 2 <= maxKFid = 5, and is no edge).  60 points seen by 2..5 key frames, stereo and monocular mixed;
// point 17 is bad, point 23 is seen by the bad key frame alone (not included), point 31 by key frame 2 alone (included, no edge).
static void build(World &w, uint64_t seed)
{
    Rng rng(seed);
    const int NK = 7, NP = 60;
    const long unsigned int ids[NK] = {3, 0, 5, 9, 4, 1, 2};
    vector<float> invSigma2(8);
    for (int l = 0; l < 8; l++) invSigma2[l] = (float)(1.0 / pow(1.2, 2 * l));
    double cx[NK];
    for (int k = 0; k < NK; k++) {
        cx[k] = rng.uniform(-1.5, 1.5);
        cv::Mat T(4, 4, CV_32F);
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) T.at<float>(i, j) = i == j ? 1.f : 0.f;
        const bool free_kf = ids[k] != 0;
        T.at<float>(0, 3) = (float)(-cx[k] + (free_kf ? rng.normal() * 0.03 : 0));
        T.at<float>(1, 3) = (float)(free_kf ? rng.normal() * 0.03 : 0);
        w.kfs.emplace_back(new KeyFrame(ids[k], 718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f, T, invSigma2));
        if (k < 6) w.map.AddKeyFrame(w.kfs.back().get());
    }
    w.kfs[3]->mbBad = true;
    for (int p = 0; p < NP; p++) {
        double X[3] = {rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(6, 20)};
        X[0] *= X[2] / 20;
        cv::Mat Pos(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) Pos.at<float>(i) = (float)(X[i] + rng.normal() * 0.03);
        w.mps.emplace_back(new MapPoint(100 + p, Pos));
        MapPoint *mp = w.mps.back().get();
        w.map.AddMapPoint(mp);
        if (p == 17) mp->mbBad = true;
        const int deg = 2 + (int)(rng.uniform() * 4);
        for (int d = 0; d < deg; d++) {
            int k = (p + d * (1 + p % 2)) % 6;
            if (p == 23) k = 3;
            if (p == 31) k = 6;
            KeyFrame *kf = w.kfs[k].get();
            if (mp->GetObservations().count(kf)) continue;
            const double pc[3] = {X[0] - cx[k], X[1], X[2]};
            cv::KeyPoint kp;
            kp.pt.x = (float)(kf->fx * pc[0] / pc[2] + kf->cx + rng.normal() * 0.7);
            kp.pt.y = (float)(kf->fy * pc[1] / pc[2] + kf->cy + rng.normal() * 0.7);
            kp.octave = (int)(rng.uniform() * 8);
            float ur = (float)(kf->fx * pc[0] / pc[2] + kf->cx - kf->mbf / pc[2] + rng.normal() * 0.7);
            if (rng.uniform() < 0.4 || ur < 0) ur = -1.f;
            mp->AddObservation(kf, kf->AddFeature(kp, ur));
        }
    }
}

// the call sites: src/Tracking.cc:693-695 and src/LoopClosing.cc:646-651
struct Tracking {
    Map *mpMap;
    void CreateInitialMapMonocular()
    {
        cout << "New Map created with " << mpMap->MapPointsInMap() << " points" << endl;

        Optimizer::GlobalBundleAdjustemnt(mpMap,20);
    }
};
struct LoopClosing {
    Map *mpMap;
    bool mbStopGBA = false;
    void RunGlobalBundleAdjustment(unsigned long nLoopKF)
    {
        Optimizer::GlobalBundleAdjustemnt(mpMap,10,&mbStopGBA,nLoopKF,false);
    }
};

static bool same_bits(const cv::Mat &a, const float *b, int n)
{
    if (a.rows * a.cols != n) return false;
    for (int i = 0; i < n; i++)
        if (memcmp(&a.ptr<float>(i / a.cols)[i % a.cols], b + i, 4)) return false;
    return true;
}

static void run(unsigned long nLoopKF)
{
    World a, b;
    build(a, 11); build(b, 11);
    int nIterations;
    bool robust;
    if (nLoopKF == 0) {
        Tracking tr{&a.map};
        tr.CreateInitialMapMonocular();
        nIterations = 20; robust = true;
    } else {
        LoopClosing lc{&a.map};
        lc.RunGlobalBundleAdjustment(nLoopKF);
        nIterations = 10; robust = false;
    }
    // the flat call on the second graph's gather
    Optimizer::BaProblem<KeyFrame, MapPoint> P;
    Optimizer::GatherBundleAdjustment(b.map.GetAllKeyFrames(), b.map.GetAllMapPoints(), P);
    CHECK(P.kfs.size() == 5 && P.localFixed[1] == 1 && P.localFixed[0] == 0 && P.localFixed[2] == 0, "key frames: %zu", P.kfs.size());   // 3 0 5 4 1
    CHECK(P.points.size() == 59, "points: %zu", P.points.size());
    const orbp_lba_problem flat = P.flat();
    orbp_ba_stats st;
    const int rc = orbp_bundle_adjustment(&flat, nIterations, robust, P.TcwOut.data(), P.xw.data(), nullptr, &st);
    CHECK(rc == 0 && st.iterations >= 3, "flat call: %d %s, %d iterations", rc, orbp_last_error(), st.iterations);
    int written = 0;
    for (size_t p = 0; p < P.points.size(); p++) {
        const size_t ip = (size_t)(P.points[p]->mnId - 100);
        MapPoint *mp = a.mps[ip].get();
        const bool inc = P.included[p] != 0;
        CHECK(inc == (ip != 23), "point %zu included", ip);
        if (ip == 31) CHECK(P.edgeOff[p] == P.edgeOff[p + 1], "point 31 has an edge");
        written += inc;
        if (nLoopKF == 0) {
            CHECK(mp->nSetWorldPos == (inc ? 1 : 0) && mp->nUpdateNormalAndDepth == (inc ? 1 : 0), "point %zu: %d SetWorldPos", ip, mp->nSetWorldPos);
            CHECK(same_bits(mp->GetWorldPos(), &P.xw[3 * p], 3), "position of point %zu", ip);
            CHECK(mp->mPosGBA.rows == 0 && mp->mnBAGlobalForKF == 0, "point %zu: GBA members written", ip);
        } else {
            CHECK(mp->nSetWorldPos == 0 && mp->nUpdateNormalAndDepth == 0, "point %zu: SetWorldPos called", ip);
            CHECK(same_bits(mp->GetWorldPos(), &b.mps[ip]->GetWorldPos().at<float>(0), 3), "point %zu moved", ip);
            CHECK(mp->mnBAGlobalForKF == (inc ? nLoopKF : 0), "point %zu: mnBAGlobalForKF", ip);
            if (inc) CHECK(mp->mPosGBA.rows == 3 && mp->mPosGBA.cols == 1 && same_bits(mp->mPosGBA, &P.xw[3 * p], 3), "mPosGBA of point %zu", ip);
            else CHECK(mp->mPosGBA.rows == 0, "mPosGBA of point %zu", ip);
        }
    }
    CHECK(written == 58, "%d points written", written);
    CHECK(a.mps[17]->nSetWorldPos == 0 && a.mps[17]->mnBAGlobalForKF == 0 && a.mps[17]->mPosGBA.rows == 0, "the bad point was written");
    CHECK(same_bits(a.mps[23]->GetWorldPos(), &b.mps[23]->GetWorldPos().at<float>(0), 3), "the not-included point moved");
    for (size_t k = 0; k < P.kfs.size(); k++) {
        size_t ik = 0;
        while (b.kfs[ik].get() != P.kfs[k]) ik++;
        KeyFrame *kf = a.kfs[ik].get();
        if (nLoopKF == 0) {
            CHECK(same_bits(kf->GetPose(), &P.TcwOut[16 * k], 16) && kf->nSetPose == 1, "pose of key frame %lu", kf->mnId);
            CHECK(kf->mTcwGBA.rows == 0 && kf->mnBAGlobalForKF == 0, "key frame %lu: GBA members written", kf->mnId);
        } else {
            CHECK(kf->nSetPose == 0, "key frame %lu: SetPose called", kf->mnId);
            CHECK(kf->mTcwGBA.rows == 4 && kf->mTcwGBA.cols == 4 && same_bits(kf->mTcwGBA, &P.TcwOut[16 * k], 16), "mTcwGBA of key frame %lu", kf->mnId);
            CHECK(kf->mnBAGlobalForKF == nLoopKF, "key frame %lu: mnBAGlobalForKF", kf->mnId);
        }
    }
    for (size_t ik : {size_t(3), size_t(6)})
        CHECK(a.kfs[ik]->nSetPose == 0 && a.kfs[ik]->mTcwGBA.rows == 0 && a.kfs[ik]->mnBAGlobalForKF == 0, "key frame %lu was written", a.kfs[ik]->mnId);
    float moved = 0;
    for (int i = 0; i < 16; i++) moved = fmaxf(moved, fabsf(P.TcwOut[i] - P.Tcw[i]));
    CHECK(moved > 1e-4f, "the first key frame did not move");
    printf("nLoopKF %lu: %zu key frames, %zu points, %d written, %d iterations\n", nLoopKF, P.kfs.size(), P.points.size(), written, st.iterations);
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    run(0);
    run(7);
    // pbStopFlag up when the call begins: no entry check, so the round-tripped inputs are written back (LocalBundleAdjustment writes nothing)
    World c;
    build(c, 11);
    LoopClosing stopped{&c.map};
    stopped.mbStopGBA = true;
    stopped.RunGlobalBundleAdjustment(3);
    CHECK(c.kfs[0]->mnBAGlobalForKF == 3 && c.kfs[0]->mTcwGBA.rows == 4, "stopped: nothing written");
    CHECK(fabsf(c.kfs[0]->mTcwGBA.at<float>(0, 3) - c.kfs[0]->GetPose().at<float>(0, 3)) < 1e-6f, "stopped: the pose moved");
    string err;
    CHECK(Optimizer::GlobalBundleAdjustemnt(static_cast<orbm_matcher *>(nullptr), &c.map, &err, ORBP_BA_MAX_ITERATIONS + 1) == ORBX_E_INVALID &&
          err.find("n_iterations") != string::npos, "n_iterations beyond the bound: %s", err.c_str());
    if (failures == 0) printf("ba_callsites ok\n");
    return failures ? 1 : 0;
}
