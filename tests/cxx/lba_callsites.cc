// lba_callsites.cc -- Optimizer::LocalBundleAdjustment of my-slam_amd/host/PnPsolver.h at its call site: the line
// src/LocalMapping.cc:82 verbatim, on the classes of tests/cxx/lba_shims/.  The object graph after the call must be what the flat
// call orbp_local_bundle_adjustment dictates for the same gather: the erased matches on both sides, the poses, the positions, one
// UpdateNormalAndDepth per local point.
//   lba_callsites compile-only       nothing runs
//   lba_callsites host               the line as written (host path), against the flat call on a second, identical graph
//   lba_callsites gpu R T X          the handle overload against the host form: same erased pairs, poses / positions within the
//                                    bars R (rotation entries), T (translation), X (point coordinates) plus float rounding
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "KeyFrame.h"
#include "PnPsolver.h"

using namespace ORB_SLAM2;
using namespace std;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Rng {                                    // a fixed generator: the two graphs of a run are built from the same draws
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
    KeyFrame *current = nullptr;
};

static void rodrigues(const double w[3], double R[9])
{
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double k[3] = {th > 0 ? w[0] / th : 0, th > 0 ? w[1] / th : 0, th > 0 ? w[2] / th : 0};
    const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    const double s = sin(th), c = 1 - cos(th);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double kk = 0;
            for (int m = 0; m < 3; m++) kk += K[3 * i + m] * K[3 * m + j];
            R[3 * i + j] = (i == j) + s * K[3 * i + j] + c * kk;
        }
}

// 8 key frames: ids 5 (current), 4, 3, 2 (bad), 0 local through the covisibility list; ids 1, 6, 7 see local points only (fixed
// cameras; 7 is bad).  120 points, each seen by 3..6 key frames, stereo and monocular mixed, a tenth gross outliers; one bad point.
static void build(World &w, uint64_t seed)
{
    Rng rng(seed);
    const int NK = 8, NP = 120;
    const long unsigned int ids[NK] = {5, 4, 3, 2, 0, 1, 6, 7};
    vector<float> invSigma2(8);
    for (int l = 0; l < 8; l++) invSigma2[l] = (float)(1.0 / pow(1.2, 2 * l));
    double R[NK][9], t[NK][3];
    for (int k = 0; k < NK; k++) {
        const double wv[3] = {rng.normal() * 0.04, rng.normal() * 0.04, rng.normal() * 0.04};
        rodrigues(wv, R[k]);
        const double c[3] = {rng.uniform(-1.5, 1.5), rng.uniform(-0.3, 0.3), rng.uniform(-1, 1)};
        for (int i = 0; i < 3; i++) t[k][i] = -(R[k][3 * i] * c[0] + R[k][3 * i + 1] * c[1] + R[k][3 * i + 2] * c[2]);
        cv::Mat T(4, 4, CV_32F);
        // the free key frames start a few centimetres and tenths of a degree off
        const bool free_kf = ids[k] == 5 || ids[k] == 4 || ids[k] == 3;
        double dR[9], Rp[9], tp[3];
        const double dw[3] = {free_kf ? rng.normal() * 0.003 : 0, free_kf ? rng.normal() * 0.003 : 0, free_kf ? rng.normal() * 0.003 : 0};
        rodrigues(dw, dR);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) Rp[3 * i + j] = dR[3 * i] * R[k][j] + dR[3 * i + 1] * R[k][3 + j] + dR[3 * i + 2] * R[k][6 + j];
            tp[i] = dR[3 * i] * t[k][0] + dR[3 * i + 1] * t[k][1] + dR[3 * i + 2] * t[k][2] + (free_kf ? rng.normal() * 0.03 : 0);
        }
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) T.at<float>(i, j) = i < 3 ? (j < 3 ? (float)Rp[3 * i + j] : (float)tp[i]) : (j == 3 ? 1.f : 0.f);
        const bool tum = k % 4 == 3;
        w.kfs.emplace_back(new KeyFrame(ids[k], tum ? 517.306408f : 718.856f, tum ? 516.469215f : 718.856f, tum ? 318.643040f : 607.1928f,
                                        tum ? 255.313989f : 185.2157f, tum ? 40.0f : 386.1448f, T, invSigma2));
    }
    w.kfs[3]->mbBad = true;
    w.kfs[7]->mbBad = true;
    w.current = w.kfs[0].get();
    for (int k = 1; k <= 4; k++) w.current->mvpOrderedConnectedKeyFrames.push_back(w.kfs[k].get());
    for (int p = 0; p < NP; p++) {
        double X[3] = {rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(6, 20)};
        X[0] *= X[2] / 20;
        cv::Mat Pos(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) Pos.at<float>(i) = (float)(X[i] + rng.normal() * 0.03);
        w.mps.emplace_back(new MapPoint(100 + p, Pos));
        MapPoint *mp = w.mps.back().get();
        if (p == 17) mp->mbBad = true;
        const int deg = 3 + (int)(rng.uniform() * 4);
        const int first = p < 40 ? 0 : (int)(rng.uniform() * 3);           // every point is seen by a local key frame
        for (int d = 0; d < deg; d++) {
            const int k = (first + d * (d == 0 ? 1 : 1 + (p % 2))) % NK;
            KeyFrame *kf = w.kfs[k].get();
            if (mp->GetObservations().count(kf)) continue;
            double pc[3];
            for (int i = 0; i < 3; i++) pc[i] = R[k][3 * i] * X[0] + R[k][3 * i + 1] * X[1] + R[k][3 * i + 2] * X[2] + t[k][i];
            cv::KeyPoint kp;
            kp.pt.x = (float)(kf->fx * pc[0] / pc[2] + kf->cx + rng.normal() * 0.7);
            kp.pt.y = (float)(kf->fy * pc[1] / pc[2] + kf->cy + rng.normal() * 0.7);
            kp.octave = (int)(rng.uniform() * 8);
            float ur = (float)(kf->fx * pc[0] / pc[2] + kf->cx - kf->mbf / pc[2] + rng.normal() * 0.7);
            if (rng.uniform() < 0.1) { kp.pt.x += (float)rng.uniform(30, 80); kp.pt.y -= (float)rng.uniform(30, 80); ur += 50.f; }
            if (rng.uniform() < 0.5 || ur < 0) ur = -1.f;
            mp->AddObservation(kf, kf->AddFeature(kp, ur, mp));
        }
    }
}

// the call site: src/LocalMapping.cc:78-83
struct LocalMapping {
    KeyFrame *mpCurrentKeyFrame;
    Map *mpMap;
    bool mbAbortBA = false;
    void Run()
    {
        Optimizer::LocalBundleAdjustment(mpCurrentKeyFrame,&mbAbortBA, mpMap);
    }
};

static bool same_bits(const cv::Mat &a, const cv::Mat &b)
{
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int r = 0; r < a.rows; r++)
        if (memcmp(a.ptr<float>(r), b.ptr<float>(r), sizeof(float) * a.cols)) return false;
    return true;
}

static int run_host()
{
    World a, b, c;
    build(a, 7); build(b, 7); build(c, 7);
    LocalMapping lm{a.current, &a.map};
    lm.Run();
    // the flat call on the second graph's gather
    Optimizer::LbaProblem<KeyFrame, MapPoint> P;
    Optimizer::GatherLocalBundleAdjustment(b.current, P);
    CHECK(P.local.size() == 4 && P.localFixed[3] == 1 && P.localFixed[0] == 0, "local key frames: %zu", P.local.size());   // 5 4 3 0; 2 is bad
    CHECK(P.fixed.size() == 2, "fixed cameras: %zu", P.fixed.size());                                                       // 1 6; 7 is bad
    CHECK(P.points.size() == 119, "local points: %zu", P.points.size());
    CHECK(b.kfs[3]->mnBALocalForKF == 5 && b.kfs[7]->mnBAFixedForKF == 5 && b.kfs[5]->mnBAFixedForKF == 5, "marks");
    const orbp_lba_problem flat = P.flat();
    orbp_lba_stats st;
    const int rc = orbp_local_bundle_adjustment(&flat, P.TcwLocal.data(), P.xw.data(), P.erase.data(), nullptr, &st);
    CHECK(rc == ORBP_LBA_DONE, "flat call: %d %s", rc, orbp_last_error());
    CHECK(st.n_level1 > 5 && st.iterations[1] > 0, "rounds: %d level-1 edges, %d iterations", st.n_level1, st.iterations[1]);
    int erased = 0;
    for (size_t p = 0; p < P.points.size(); p++) {
        const size_t ip = (size_t)(P.points[p]->mnId - 100);
        MapPoint *mp = a.mps[ip].get();
        const cv::Mat X = mp->GetWorldPos();
        CHECK(memcmp(&X.at<float>(0), &P.xw[3 * p], 4) == 0 && X.at<float>(1) == P.xw[3 * p + 1] && X.at<float>(2) == P.xw[3 * p + 2], "position of point %zu", ip);
        CHECK(mp->nUpdateNormalAndDepth == 1 && mp->nSetWorldPos == 1, "point %zu: %d UpdateNormalAndDepth", ip, mp->nUpdateNormalAndDepth);
        const auto obs_b = P.points[p]->GetObservations();
        const auto obs_a = mp->GetObservations();
        int e = P.edgeOff[p], gone = 0;
        for (auto it = obs_b.begin(); it != obs_b.end(); ++it) {
            if (it->first->isBad()) continue;
            size_t ik = 0;
            while (b.kfs[ik].get() != it->first) ik++;
            KeyFrame *kf = a.kfs[ik].get();
            const bool er = P.erase[e++] != 0;
            gone += er;
            CHECK((obs_a.count(kf) == 0) == er, "observation of point %zu in key frame %lu", ip, kf->mnId);
            CHECK((kf->GetMapPointMatches()[it->second] == NULL) == er, "match %zu of key frame %lu", it->second, kf->mnId);
        }
        CHECK(e == P.edgeOff[p + 1] && mp->nEraseObservation == gone, "edges of point %zu", ip);
        erased += gone;
    }
    CHECK(erased > 5, "%d pairs erased", erased);
    for (size_t k = 0; k < P.local.size(); k++) {
        size_t ik = 0;
        while (b.kfs[ik].get() != P.local[k]) ik++;
        cv::Mat want(4, 4, CV_32F);
        memcpy(want.ptr<float>(0), &P.TcwLocal[16 * k], 64);
        CHECK(same_bits(a.kfs[ik]->GetPose(), want) && a.kfs[ik]->nSetPose == 1, "pose of key frame %lu", a.kfs[ik]->mnId);
    }
    for (size_t ik : {size_t(3), size_t(5), size_t(6), size_t(7)}) CHECK(a.kfs[ik]->nSetPose == 0, "key frame %lu was written", a.kfs[ik]->mnId);
    CHECK(a.mps[17]->nSetWorldPos == 0 && a.mps[17]->nUpdateNormalAndDepth == 0, "the bad point was written");
    // :655-657: nothing is written when the flag is up at entry
    LocalMapping stopped{c.current, &c.map};
    stopped.mbAbortBA = true;
    stopped.Run();
    for (auto &kf : c.kfs) CHECK(kf->nSetPose == 0 && kf->nEraseMapPointMatch == 0, "stopped: key frame %lu", kf->mnId);
    for (auto &mp : c.mps) CHECK(mp->nSetWorldPos == 0 && mp->nUpdateNormalAndDepth == 0, "stopped: point %lu", mp->mnId);
    printf("host: %zu local, %zu fixed, %zu points, %d pairs erased, iterations %d + %d\n", P.local.size(), P.fixed.size(), P.points.size(), erased,
           st.iterations[0], st.iterations[1]);
    return failures;
}

static int run_gpu(double barR, double barT, double barX)
{
    World a, b;
    build(a, 7); build(b, 7);
    LocalMapping lm{a.current, &a.map};
    lm.Run();
    orbm_matcher *m = nullptr;
    if (orbm_create(&m, 0, 64, 64, 256) != ORBX_OK) { printf("FAILED orbm_create: %s\n", orbm_last_error()); return 1; }
    string err;
    bool flag = false;
    orbp_lba_stats st;
    const int rc = Optimizer::LocalBundleAdjustment(m, b.current, &flag, &b.map, &err, &st);
    CHECK(rc == ORBP_LBA_DONE, "handle overload: %d %s", rc, err.c_str());
    double dR = 0, dT = 0, dX = 0, mT = 0, mX = 0;
    for (size_t k = 0; k < a.kfs.size(); k++) {
        const cv::Mat A = a.kfs[k]->GetPose(), B = b.kfs[k]->GetPose();
        CHECK(a.kfs[k]->nSetPose == b.kfs[k]->nSetPose && a.kfs[k]->nEraseMapPointMatch == b.kfs[k]->nEraseMapPointMatch, "key frame %lu", a.kfs[k]->mnId);
        for (int r = 0; r < 3; r++) {
            for (int c2 = 0; c2 < 3; c2++) dR = fmax(dR, fabs((double)A.at<float>(r, c2) - B.at<float>(r, c2)));
            dT = fmax(dT, fabs((double)A.at<float>(r, 3) - B.at<float>(r, 3)));
            mT = fmax(mT, fabs((double)A.at<float>(r, 3)));
        }
        const auto ma = a.kfs[k]->GetMapPointMatches(), mb = b.kfs[k]->GetMapPointMatches();
        for (size_t i = 0; i < ma.size(); i++) CHECK((ma[i] == NULL) == (mb[i] == NULL), "match %zu of key frame %lu", i, a.kfs[k]->mnId);
    }
    for (size_t p = 0; p < a.mps.size(); p++) {
        const cv::Mat A = a.mps[p]->GetWorldPos(), B = b.mps[p]->GetWorldPos();
        for (int r = 0; r < 3; r++) { dX = fmax(dX, fabs((double)A.at<float>(r) - B.at<float>(r))); mX = fmax(mX, fabs((double)A.at<float>(r))); }
        CHECK(a.mps[p]->GetObservations().size() == b.mps[p]->GetObservations().size() && a.mps[p]->nUpdateNormalAndDepth == b.mps[p]->nUpdateNormalAndDepth,
              "point %lu", a.mps[p]->mnId);
    }
    const double ulp = ldexp(1.0, -23);
    printf("gpu against host: |d rotation| %.3g, |d translation| %.3g, |d point| %.3g\n", dR, dT, dX);
    CHECK(dR <= barR + ulp && dT <= barT + ulp * mT && dX <= barX + ulp * mX, "beyond the bars %.3g %.3g %.3g", barR, barT, barX);
    orbm_destroy(m);
    return failures;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    int rc;
    if (argc > 4 && !strcmp(argv[1], "gpu")) rc = run_gpu(atof(argv[2]), atof(argv[3]), atof(argv[4]));
    else rc = run_host();
    if (rc == 0) printf("lba_callsites ok\n");
    return rc ? 1 : 0;
}
