// eg_callsites.cc -- Optimizer::OptimizeEssentialGraph of my-slam_amd/host/PnPsolver.h at its call site: the line
// src/LoopClosing.cc:568 verbatim, on the classes of tests/cxx/eg_shims/.  A small map goes through gather, host call and scatter;
// the edge list of the gather must be the hand-written walk of src/Optimizer.cc:852-983 over the same objects (the list below, with
// the reason of every skip), and the object graph afterwards what the flat call orbp_optimize_essential_graph dictates.
//   eg_callsites compile-only        nothing runs
//   eg_callsites host                the line as written (host path), against the flat call on a second, identical graph
// Built with -DEG_CALLSITES_STANDALONE (tests/test_eg_cxx.py) it links orbp_eg.cc, orbp_sim3opt.cc and orbp.cc instead of the
// library and runs under AddressSanitizer and UBSan: the gather, the host solver and the scatter, host code only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "LoopClosing.h"
#include "PnPsolver.h"

#ifdef EG_CALLSITES_STANDALONE
// the handle overload names these; with a NULL matcher they are never called
extern "C" int orbm_optimize_essential_graph(orbm_matcher *, const orbp_eg_problem *, int, float *, float *, double *, orbp_eg_stats *) { abort(); }
extern "C" const char *orbm_last_error(void) { return ""; }
#endif

using namespace ORB_SLAM2;
using namespace std;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int NK = 10, NP = 12, BAD_KF = 9, LOOP_KF = 1, CUR_KF = 8;
static long unsigned int id_of(int k) { return 2 * (long unsigned int)k + 1; }

struct World {
    vector<KeyFrame> kfs;                       // one array: pointer order is index order, so the std::set / std::map walks are fixed
    vector<MapPoint> mps;
    Map map;
    LoopClosing::KeyFrameAndPose NonCorrectedSim3, CorrectedSim3;
    std::map<KeyFrame *, set<KeyFrame *> > LoopConnections;
};

static void pose(int k, double extra_angle, double dx, float *R, float *t)
{
    const double a = 0.05 * k + extra_angle, c = cos(a), s = sin(a);
    const double Rd[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int i = 0; i < 9; i++) R[i] = (float)Rd[i];
    t[0] = (float)(-0.4 * k + dx); t[1] = (float)(0.01 * k); t[2] = (float)(0.02 * k * k);
}

static void build(World &w)
{
    w.kfs.reserve(NK); w.mps.reserve(NP);
    for (int k = 0; k < NK; k++) {
        float R[9], t[3];
        pose(k, 0, 0, R, t);
        cv::Mat T(4, 4, CV_32F);
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) T.at<float>(i, j) = i == j ? 1.f : 0.f;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T.at<float>(i, j) = R[3 * i + j];
            T.at<float>(i, 3) = t[i];
        }
        w.kfs.emplace_back(id_of(k), T);
    }
    KeyFrame *K = w.kfs.data();
    K[BAD_KF].mbBad = true;
    for (int k = 1; k < NK; k++) { K[k].mpParent = &K[k - 1]; K[k - 1].mspChildrens.insert(&K[k]); }
    const int order[NK] = {4, 0, 7, 2, 9, 5, 1, 3, 8, 6};
    for (int i = 0; i < NK; i++) w.map.AddKeyFrame(&K[order[i]]);
    const auto weight = [&](int a, int b, int v) { K[a].mConnectedKeyFrameWeights[&K[b]] = v; K[b].mConnectedKeyFrameWeights[&K[a]] = v; };
    weight(8, 1, 30); weight(8, 0, 150); weight(7, 1, 50); weight(7, 2, 110);
    w.LoopConnections[&K[7]] = {&K[1], &K[2]};
    w.LoopConnections[&K[8]] = {&K[0], &K[1]};
    K[4].mvpOrderedConnectedKeyFrames = {&K[3], &K[5], &K[2]};
    K[0].mvpOrderedConnectedKeyFrames = {&K[8]};
    K[7].mvpOrderedConnectedKeyFrames = {&K[2], &K[5]};
    K[2].mvpOrderedConnectedKeyFrames = {&K[4], &K[7]};
    K[5].mvpOrderedConnectedKeyFrames = {&K[2], &K[3], &K[9]};
    K[3].mvpOrderedConnectedKeyFrames = {nullptr, &K[1]};
    K[8].mvpOrderedConnectedKeyFrames = {&K[0], &K[9], &K[6]};
    K[6].mvpOrderedConnectedKeyFrames = {&K[8]};
    K[5].mspLoopEdges = {&K[2]}; K[2].mspLoopEdges = {&K[5]};
    for (int k = 7; k <= 8; k++) {              // the current key frame and its neighbour were corrected (src/LoopClosing.cc:437-470)
        float R[9], t[3];
        g2o::Sim3 S;
        pose(k, 0, 0, R, t);
        orbp_sim3_from_rts(R, t, 1.f, S.v);
        w.NonCorrectedSim3[&K[k]] = S;
        pose(k, 0.1, 0.3, R, t);
        orbp_sim3_from_rts(R, t, 1.05f, S.v);
        w.CorrectedSim3[&K[k]] = S;
    }
    for (int p = 0; p < NP; p++) {
        cv::Mat X(3, 1, CV_32F);
        X.at<float>(0) = 0.7f * p - 3.f; X.at<float>(1) = 0.3f * (p % 4) - 0.5f; X.at<float>(2) = 6.f + 0.9f * p;
        w.mps.emplace_back(100 + p, X, &K[p % 9]);
        w.map.AddMapPoint(&w.mps.back());
    }
    w.mps[3].mbBad = true;
    w.mps[5].mnCorrectedByKF = id_of(CUR_KF); w.mps[5].mnCorrectedReference = id_of(7);    // :1021-1024
    w.mps[6] = MapPoint(106, w.mps[6].GetWorldPos(), &K[BAD_KF]);                            // its reference has no vertex
}

// src/Optimizer.cc:852-983 walked by hand over build()'s objects, as (vertex 0, vertex 1, measured from the corrected Sim3s)
static const int EXPECTED[][3] = {
    // LoopConnections, key frame 7: (7, 1) has weight 50 < minFeat and is not (current, loop): skipped; (7, 2) has 110
    {7, 2, 1},
    // key frame 8: (8, 0) has 150; (8, 1) has 30 but is (pCurKF, pLoopKF), the exception of :863
    {8, 0, 1}, {8, 1, 1},
    // then the key frames in the map's order 4 0 7 2 9 5 1 3 8 6: parent, loop edges, covisibles
    {4, 3, 0}, {4, 2, 0},           // covisibles 3 (parent) and 5 (child) skipped
    /* 0: no parent; covisible 8 has the larger id */
    {7, 6, 0}, {7, 5, 0},           // covisible 2: (2, 7) is in sInsertedEdges
    {2, 1, 0},                      // loop edge 5 and covisibles 4, 7 have larger ids
    /* 9 is bad: no vertex */
    {5, 4, 0}, {5, 2, 0}, {5, 3, 0},    // loop edge 2; covisible 2 is a loop edge, 9 is bad
    {1, 0, 0},
    {3, 2, 0}, {3, 1, 0},           // a NULL covisible is passed over
    {8, 7, 0}, {8, 6, 0},           // covisible 0: (0, 8) is in sInsertedEdges; 9 is bad
    {6, 5, 0},
};

typedef Optimizer::EgProblem<KeyFrame, MapPoint> Problem;

static void gather(World &w, Problem &P)
{
    Optimizer::GatherEssentialGraph(&w.map, &w.kfs[LOOP_KF], &w.kfs[CUR_KF], w.NonCorrectedSim3, w.CorrectedSim3, w.LoopConnections, false, P);
}

// what src/LoopClosing.cc:568 sees: its members by the reference's names
struct LoopClosingAtCorrectLoop {
    Map *mpMap;
    KeyFrame *mpMatchedKF, *mpCurrentKF;
    bool mbFixScale;
    void CorrectLoop(const LoopClosing::KeyFrameAndPose &NonCorrectedSim3, const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                     const map<KeyFrame *, set<KeyFrame *> > &LoopConnections)
    {
        // src/LoopClosing.cc:568
        Optimizer::OptimizeEssentialGraph(mpMap, mpMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, mbFixScale);
    }
};

static int run()
{
    World a, b;
    build(a); build(b);
    Problem P;
    gather(b, P);
    const orbp_eg_problem flat = P.flat();
    const int NE = (int)(sizeof EXPECTED / sizeof EXPECTED[0]);
    CHECK(flat.n_kfs == 9 && flat.fixed == LOOP_KF && flat.fix_scale == 0 && flat.n_points == NP - 1, "counts %d %d %d", flat.n_kfs, flat.fixed, flat.n_points);
    CHECK(flat.n_edges == NE, "%d edges, expected %d", flat.n_edges, NE);
    for (int e = 0; e < NE && e < flat.n_edges; e++)
        CHECK(P.edgeI[e] == EXPECTED[e][0] && P.edgeJ[e] == EXPECTED[e][1] && P.edgeCorrected[e] == EXPECTED[e][2], "edge %d is (%d, %d, %d)", e,
              P.edgeI[e], P.edgeJ[e], P.edgeCorrected[e]);
    for (int k = 0; k < 9; k++) {
        CHECK(P.kfs[k] == &b.kfs[k], "vertex %d", k);
        CHECK(b.kfs[k].nAskedWeight == 100, "GetCovisiblesByWeight(%d)", b.kfs[k].nAskedWeight);
        const bool corrected = k >= 7;
        CHECK((memcmp(&P.Scw[8 * k], &P.Snc[8 * k], 64) != 0) == corrected, "Snc of %d", k);
        if (corrected) CHECK(memcmp(&P.Scw[8 * k], b.CorrectedSim3[&b.kfs[k]].v, 64) == 0 && memcmp(&P.Snc[8 * k], b.NonCorrectedSim3[&b.kfs[k]].v, 64) == 0, "Sim3 of %d", k);
        else CHECK(P.Scw[8 * k + 7] == 1.0, "scale of %d", k);
    }
    // points in map order without the bad one: 0 1 2 4 5 6 ...
    CHECK(P.ref[4] == 7 && P.ref[5] == -1 && P.ref[0] == 0 && P.ref[3] == 4, "refs %d %d %d %d", P.ref[4], P.ref[5], P.ref[0], P.ref[3]);
    vector<float> Tcw(16 * 9), xw(P.xw);
    orbp_eg_stats st;
    const int rc = orbp_optimize_essential_graph(&flat, 20, Tcw.data(), xw.data(), nullptr, &st);
    CHECK(rc == 0, "flat call: %d %s", rc, orbp_last_error());
    CHECK(st.iterations > 0 && st.chi2_final < 0.5 * st.chi2_initial, "chi2 %g -> %g", st.chi2_initial, st.chi2_final);

    LoopClosingAtCorrectLoop lc = {&a.map, &a.kfs[LOOP_KF], &a.kfs[CUR_KF], false};
    lc.CorrectLoop(a.NonCorrectedSim3, a.CorrectedSim3, a.LoopConnections);
    int moved = 0;
    for (int k = 0; k < NK; k++) {
        CHECK(a.kfs[k].nSetPose == (k == BAD_KF ? 0 : 1), "SetPose of %d: %d", k, a.kfs[k].nSetPose);
        if (k == BAD_KF) continue;
        const cv::Mat T = a.kfs[k].GetPose(), T0 = b.kfs[k].GetPose();
        for (int i = 0; i < 16; i++) {
            CHECK(T.at<float>(i / 4, i % 4) == Tcw[16 * k + i], "pose of %d, entry %d", k, i);
            moved += T.at<float>(i / 4, i % 4) != T0.at<float>(i / 4, i % 4);
        }
    }
    CHECK(moved > 50, "only %d pose entries moved", moved);
    int row = 0, written = 0;
    for (int p = 0; p < NP; p++) {
        MapPoint &mp = a.mps[p];
        CHECK(mp.nSetWorldPos == (p == 3 ? 0 : 1) && mp.nUpdateNormalAndDepth == mp.nSetWorldPos, "point %d: %d %d", p, mp.nSetWorldPos, mp.nUpdateNormalAndDepth);
        if (p == 3) continue;
        const cv::Mat X = mp.GetWorldPos(), X0 = b.mps[p].GetWorldPos();
        for (int r = 0; r < 3; r++) CHECK(X.at<float>(r) == xw[3 * row + r], "point %d", p);
        if (p == 6) CHECK(memcmp(X.ptr<float>(), X0.ptr<float>(), 4) == 0 && X.at<float>(1) == X0.at<float>(1) && X.at<float>(2) == X0.at<float>(2), "point 6 moved");
        else written += X.at<float>(0) != X0.at<float>(0);
        row++;
    }
    CHECK(written >= 8, "only %d points moved", written);
    // the handle overload with no handle is the host path, and hands the stats back
    World c;
    build(c);
    string err;
    orbp_eg_stats st2;
    const int rc2 = Optimizer::OptimizeEssentialGraph(static_cast<orbm_matcher *>(nullptr), &c.map, &c.kfs[LOOP_KF], &c.kfs[CUR_KF], c.NonCorrectedSim3,
                                                      c.CorrectedSim3, c.LoopConnections, false, &err, &st2);
    CHECK(rc2 == 0 && st2.iterations == st.iterations && st2.chi2_final == st.chi2_final, "handle overload: %d %s", rc2, err.c_str());
    printf("%d key frames, %d edges, %d points, %d written, chi2 %.3g -> %.3g in %d iterations\n", flat.n_kfs, flat.n_edges, flat.n_points, written,
           st.chi2_initial, st.chi2_final, st.iterations);
    return failures;
}

int main(int argc, char **argv)
{
    if (argc < 2 || !strcmp(argv[1], "compile-only")) return 0;
    if (run() == 0) { printf("eg_callsites ok\n"); return 0; }
    return 1;
}
