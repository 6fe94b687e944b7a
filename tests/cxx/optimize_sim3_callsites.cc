// optimize_sim3_callsites.cc -- Optimizer::OptimizeSim3 at its call site, LoopClosing::ComputeSim3 (src/LoopClosing.cc:287-343 of the
// reference), against my-slam_amd/host/PnPsolver.h on the classes of tests/cxx/slam_shims/: the line :327 verbatim, and the loop
// rewritten round by round with ONE Optimizer::OptimizeSim3Batch call per round.  g2o::Sim3 below is a stand-in
// with operator[] and an (R, t, s) constructor: test scaffolding, an ORB-SLAM2 tree brings g2o's.
// usage: optimize_sim3_callsites compile-only
//        optimize_sim3_callsites host                 (no GPU: the line :327 on the RANSAC inliers of every candidate)
//        optimize_sim3_callsites QBAR TBAR SBAR       (needs a GPU: both loop forms, compared; the bars on |d gScm| per part)
//
// Scene: key frame 1 (mpCurrentKF) with 100 MapPoints and three candidate key frames with one calibration; per candidate a planted
// similarity, key points at the projections (+- 0.4 px), every sixth pair a gross outlier, every fourth pair left for SearchBySim3
// to find.  Candidate 0 carries a mvInvLevelSigma2 2000 times too large: RANSAC returns a pose for it, OptimizeSim3 removes nearly
// every pair and returns fewer than 20, so the loop goes on to candidate 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "PnPsolver.h"
#include "Sim3Solver.h"

using namespace std;
using namespace ORB_SLAM2;

namespace g2o {
struct Sim3 {
    double v[8];
    Sim3() { for (int k = 0; k < 8; k++) v[k] = k == 3 || k == 7; }
    Sim3(const cv::Mat &R, const cv::Mat &t, double s)
    {
        float Rf[9], tf[3];
        for (int k = 0; k < 9; k++) Rf[k] = R.at<float>(k / 3, k % 3);
        for (int k = 0; k < 3; k++) tf[k] = t.at<float>(k);
        orbp_sim3_from_rts(Rf, tf, (float)s, v);
    }
    double operator[](int i) const { return v[i]; }
    double &operator[](int i) { return v[i]; }
};
}   // namespace g2o

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct Lcg { unsigned s; };
static int lcg_next(void *ctx) { Lcg *g = (Lcg *)ctx; g->s = (1103515245u * g->s + 12345u) & 0x7fffffffu; return (int)g->s; }
static double uni(Lcg &g, double a, double b) { return a + (b - a) * (lcg_next(&g) / 2147483648.0); }

static void rodrigues(const double *w, double *R)
{
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), c = cos(th), s = sin(th), x = w[0] / th, y = w[1] / th, z = w[2] / th;
    const double r[9] = {c + (1 - c) * x * x, (1 - c) * x * y - s * z, (1 - c) * x * z + s * y, (1 - c) * x * y + s * z, c + (1 - c) * y * y,
                         (1 - c) * y * z - s * x, (1 - c) * x * z - s * y, (1 - c) * y * z + s * x, c + (1 - c) * z * z};
    memcpy(R, r, sizeof r);
}
static cv::Mat pose(const double *R, const double *t)
{
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T.at<float>(r, c) = (float)R[3 * r + c]; T.at<float>(r, 3) = (float)t[r]; }
    return T;
}
static cv::Mat to_world(const double *R, const double *t, const double *xc)        // Xw with Rcw Xw + tcw = xc
{
    double d[3] = {xc[0] - t[0], xc[1] - t[1], xc[2] - t[2]};
    cv::Mat m(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) m.at<float>(k) = (float)(R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2]);
    return m;
}

static const float FX = 525.f, FY = 530.f, CX = 319.5f, CY = 239.5f, W = 640.f, H = 480.f;
static const int NP = 100, N1 = 120, N2 = 110;

struct KfSpec { vector<cv::KeyPoint> keys; cv::Mat desc; };
static KfSpec random_features(int n, Lcg &g)
{
    KfSpec k;
    k.keys.resize(n);
    k.desc = cv::Mat(n, 32, CV_8U);
    for (int i = 0; i < n; i++) {
        k.keys[i].pt = cv::Point2f((float)uni(g, 5, W - 5), (float)uni(g, 5, H - 5));
        k.keys[i].octave = lcg_next(&g) % 4;
        for (int b = 0; b < 32; b++) k.desc.ptr<unsigned char>(i)[b] = (unsigned char)(lcg_next(&g) >> 8);
    }
    return k;
}
static KeyFrame *make_kf(long unsigned id, const KfSpec &k, const double *R, const double *t, float invSigmaFactor)
{
    const int n = (int)k.keys.size();
    vector<float> sf(8), s2(8), is2(8);
    for (int l = 0; l < 8; l++) { sf[l] = l ? sf[l - 1] * 1.2f : 1.f; s2[l] = sf[l] * sf[l]; is2[l] = invSigmaFactor / s2[l]; }
    KeyFrame *kf = new KeyFrame(id, k.keys, vector<float>(n, -1.f), k.desc, DBoW2::FeatureVector(), vector<MapPoint *>(n, static_cast<MapPoint *>(NULL)),
                                FX, FY, CX, CY, 0.f, 64.f / W, 48.f / H, 0.f, 0.f, W, H, sf, s2, is2, logf(1.2f));
    kf->SetPose(pose(R, t));
    return kf;
}
static void place(KfSpec &k, int slot, const double *xc, int octave, const unsigned char *desc, int flip, Lcg &g)
{
    float u = (float)(FX * xc[0] / xc[2] + CX + uni(g, -0.4, 0.4)), v = (float)(FY * xc[1] / xc[2] + CY + uni(g, -0.4, 0.4));
    k.keys[slot].pt = cv::Point2f(min(max(u, 1.f), W - 2.f), min(max(v, 1.f), H - 2.f));
    k.keys[slot].octave = octave;
    memcpy(k.desc.ptr<unsigned char>(slot), desc, 32);
    for (int b = 0; b < flip; b++) k.desc.ptr<unsigned char>(slot)[(7 * b + slot) % 32] ^= (unsigned char)(1u << (b % 8));
}

struct Scene {
    KeyFrame *mpCurrentKF = nullptr;
    vector<KeyFrame *> mvpEnoughConsistentCandidates;
    vector<vector<MapPoint *> > vvpMapPointMatches;
    vector<MapPoint *> owned;
};

static Scene make_scene(bool mbFixScale, unsigned seed)
{
    Scene sc;
    Lcg g{seed};
    double R1[9], t1[3] = {0.3, -0.2, 0.5};
    const double w1[3] = {0.1, -0.15, 0.2};
    rodrigues(w1, R1);
    KfSpec k1 = random_features(N1, g);
    vector<double> x1(3 * NP);
    vector<int> oct(NP);
    vector<vector<unsigned char> > desc(NP, vector<unsigned char>(32));
    for (int i = 0; i < NP; i++) {
        const double z = uni(g, 3, 9);
        x1[3 * i] = uni(g, -0.3, 0.3) * z; x1[3 * i + 1] = uni(g, -0.2, 0.2) * z; x1[3 * i + 2] = z;
        oct[i] = lcg_next(&g) % 4;
        for (int b = 0; b < 32; b++) desc[i][b] = (unsigned char)(lcg_next(&g) >> 8);
        place(k1, i, &x1[3 * i], oct[i], desc[i].data(), 0, g);
    }
    sc.mpCurrentKF = make_kf(100, k1, R1, t1, 1.f);
    vector<MapPoint *> p1(NP);
    for (int i = 0; i < NP; i++) {
        const double d = sqrt(x1[3 * i] * x1[3 * i] + x1[3 * i + 1] * x1[3 * i + 1] + x1[3 * i + 2] * x1[3 * i + 2]);
        const float mx = (float)(d * pow(1.2, oct[i])), mn = mx / (float)pow(1.2, 7);
        p1[i] = new MapPoint(to_world(R1, t1, &x1[3 * i]), sc.mpCurrentKF->mDescriptors.row(i), 2, mn, mx);
        sc.owned.push_back(p1[i]);
        if (i == 10) p1[i]->SetBadFlag();
        if (i != 22) p1[i]->AddObservation(sc.mpCurrentKF, i);          // 22: without an index in key frame 1
        if (i != 34) sc.mpCurrentKF->AddMapPoint(p1[i], i);              // 34: the slot holds no MapPoint (:1112)
    }
    for (int c = 0; c < 3; c++) {
        const double s = mbFixScale ? 1.0 : uni(g, 0.92, 1.08);
        double R[9], t[3], R2[9], t2[3];
        const double w[3] = {uni(g, -0.06, 0.06), uni(g, -0.06, 0.06), uni(g, 0.02, 0.08)};
        rodrigues(w, R);
        for (int k = 0; k < 3; k++) t[k] = uni(g, -0.25, 0.25);
        const double w2[3] = {uni(g, -0.3, 0.3), uni(g, -0.3, 0.3), uni(g, 0.1, 0.3)};
        rodrigues(w2, R2);
        for (int k = 0; k < 3; k++) t2[k] = uni(g, -1, 1);
        KfSpec k2 = random_features(N2, g);
        vector<double> x2(3 * NP);
        for (int i = 0; i < NP; i++) {
            const double dx[3] = {x1[3 * i] - t[0], x1[3 * i + 1] - t[1], x1[3 * i + 2] - t[2]};
            for (int k = 0; k < 3; k++) x2[3 * i + k] = (R[k] * dx[0] + R[3 + k] * dx[1] + R[6 + k] * dx[2]) / s;      // x1 = s R x2 + t
            if (i % 6 == 5) {                                             // a gross outlier: 120 px to the side that stays in the image
                const double u = FX * x2[3 * i] / x2[3 * i + 2] + CX;
                x2[3 * i] += (u < W / 2 ? 120.0 : -120.0) / FX * x2[3 * i + 2];
            }
            place(k2, (i * 7 + 3) % N2, &x2[3 * i], oct[i], desc[i].data(), 3, g);
        }
        KeyFrame *pKF = make_kf(1 + c, k2, R2, t2, c == 0 ? 2000.f : 1.f);
        vector<MapPoint *> vpMatched12(N1, static_cast<MapPoint *>(NULL));
        for (int i = 0; i < NP; i++) {
            const int i2 = (i * 7 + 3) % N2;
            const double d = sqrt(x2[3 * i] * x2[3 * i] + x2[3 * i + 1] * x2[3 * i + 1] + x2[3 * i + 2] * x2[3 * i + 2]);
            const float mx = (float)(d * pow(1.2, oct[i])), mn = mx / (float)pow(1.2, 7);
            MapPoint *p2 = new MapPoint(to_world(R2, t2, &x2[3 * i]), pKF->mDescriptors.row(i2), 2, mn, mx);
            sc.owned.push_back(p2);
            pKF->AddMapPoint(p2, i2);
            if (i == 16) p2->SetBadFlag();
            if (i != 28) p2->AddObservation(pKF, i2);                    // 28: without an index in key frame 2 (:1114)
            if (i % 4 != 3) vpMatched12[i] = p2;                          // every fourth pair is left for SearchBySim3
        }
        sc.mvpEnoughConsistentCandidates.push_back(pKF);
        sc.vvpMapPointMatches.push_back(vpMatched12);
    }
    return sc;
}
static void free_scene(Scene &sc)
{
    for (KeyFrame *k : sc.mvpEnoughConsistentCandidates) delete k;
    delete sc.mpCurrentKF;
    for (MapPoint *p : sc.owned) delete p;
}

static vector<Sim3Solver *> make_solvers(Scene &sc, vector<Lcg> &sources, bool mbFixScale)
{
    vector<Sim3Solver *> vpSim3Solvers(sc.mvpEnoughConsistentCandidates.size());
    for (size_t i = 0; i < vpSim3Solvers.size(); i++) {
        Sim3Solver* pSolver = new Sim3Solver(sc.mpCurrentKF,sc.mvpEnoughConsistentCandidates[i],sc.vvpMapPointMatches[i],mbFixScale);
        pSolver->SetRansacParameters(0.99,20,300);
        sources[i].s = 1000u + (unsigned)i;
        pSolver->SetRand(lcg_next, &sources[i], 0x7fffffff);
        vpSim3Solvers[i] = pSolver;
    }
    return vpSim3Solvers;
}

struct Outcome {
    bool bMatch = false;
    KeyFrame *mpMatchedKF = nullptr;
    g2o::Sim3 gScm;
    vector<MapPoint *> mvpCurrentMatchedPoints;
    int nInliers = 0, rounds = 0, optimised = 0, found = 0;
};

// src/LoopClosing.cc:287-343 as written (matcher == NULL: without the SearchBySim3 line, for the run without a GPU)
static Outcome loop_reference(Scene &sc, vector<Sim3Solver *> &vpSim3Solvers, ORBmatcher *pMatcher, bool mbFixScale)
{
    Outcome out;
    KeyFrame *mpCurrentKF = sc.mpCurrentKF;
    vector<KeyFrame *> &mvpEnoughConsistentCandidates = sc.mvpEnoughConsistentCandidates;
    vector<vector<MapPoint *> > &vvpMapPointMatches = sc.vvpMapPointMatches;
    const int nInitialCandidates = (int)mvpEnoughConsistentCandidates.size();
    vector<bool> vbDiscarded(nInitialCandidates, false);
    int nCandidates = nInitialCandidates;
    bool bMatch = false;
    while(nCandidates>0 && !bMatch)
    {
        out.rounds++;
        for(int i=0; i<nInitialCandidates; i++)
        {
            if(vbDiscarded[i])
                continue;

            KeyFrame* pKF = mvpEnoughConsistentCandidates[i];

            // Perform 5 Ransac Iterations
            vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;

            Sim3Solver* pSolver = vpSim3Solvers[i];
            cv::Mat Scm  = pSolver->iterate(5,bNoMore,vbInliers,nInliers);

            // If Ransac reachs max. iterations discard keyframe
            if(bNoMore)
            {
                vbDiscarded[i]=true;
                nCandidates--;
            }

            // If RANSAC returns a Sim3, perform a guided matching and optimize with all correspondences
            if(!Scm.empty())
            {
                vector<MapPoint*> vpMapPointMatches(vvpMapPointMatches[i].size(), static_cast<MapPoint*>(NULL));
                for(size_t j=0, jend=vbInliers.size(); j<jend; j++)
                {
                    if(vbInliers[j])
                       vpMapPointMatches[j]=vvpMapPointMatches[i][j];
                }

                cv::Mat R = pSolver->GetEstimatedRotation();
                cv::Mat t = pSolver->GetEstimatedTranslation();
                const float s = pSolver->GetEstimatedScale();
                if (pMatcher) { ORBmatcher &matcher = *pMatcher; out.found +=
                matcher.SearchBySim3(mpCurrentKF,pKF,vpMapPointMatches,s,R,t,7.5);
                }

                g2o::Sim3 gScm(R,t,s);
                const int nInliers = Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale);
                out.optimised++;

                // If optimization is succesful stop ransacs and continue
                if(nInliers>=20)
                {
                    bMatch = true;
                    out.mpMatchedKF = pKF;
                    out.gScm = gScm;
                    out.nInliers = nInliers;
                    out.mvpCurrentMatchedPoints = vpMapPointMatches;
                    break;
                }
            }
        }
    }
    out.bMatch = bMatch;
    return out;
}

// the same loop round by round: iterate(5) for every live candidate, SearchBySim3 for those that returned a pose, ONE
// OptimizeSim3Batch, then the first candidate in order with nInliers >= 20 wins
static Outcome loop_batched(Scene &sc, vector<Sim3Solver *> &vpSim3Solvers, ORBmatcher &matcher, bool mbFixScale)
{
    Outcome out;
    KeyFrame *mpCurrentKF = sc.mpCurrentKF;
    vector<KeyFrame *> &mvpEnoughConsistentCandidates = sc.mvpEnoughConsistentCandidates;
    vector<vector<MapPoint *> > &vvpMapPointMatches = sc.vvpMapPointMatches;
    const int nInitialCandidates = (int)mvpEnoughConsistentCandidates.size();
    vector<bool> vbDiscarded(nInitialCandidates, false);
    int nCandidates = nInitialCandidates;
    bool bMatch = false;
    while(nCandidates>0 && !bMatch)
    {
        out.rounds++;
        vector<int> vnRound;                                    // the candidates of this round that returned a Scm, in order
        vector<vector<MapPoint*> > vvpRoundMatches;
        vector<g2o::Sim3> vgScm;
        for(int i=0; i<nInitialCandidates; i++)
        {
            if(vbDiscarded[i])
                continue;
            KeyFrame* pKF = mvpEnoughConsistentCandidates[i];
            vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;
            Sim3Solver* pSolver = vpSim3Solvers[i];
            cv::Mat Scm  = pSolver->iterate(5,bNoMore,vbInliers,nInliers);
            if(bNoMore)
            {
                vbDiscarded[i]=true;
                nCandidates--;
            }
            if(!Scm.empty())
            {
                vector<MapPoint*> vpMapPointMatches(vvpMapPointMatches[i].size(), static_cast<MapPoint*>(NULL));
                for(size_t j=0, jend=vbInliers.size(); j<jend; j++)
                {
                    if(vbInliers[j])
                       vpMapPointMatches[j]=vvpMapPointMatches[i][j];
                }
                cv::Mat R = pSolver->GetEstimatedRotation();
                cv::Mat t = pSolver->GetEstimatedTranslation();
                const float s = pSolver->GetEstimatedScale();
                out.found += matcher.SearchBySim3(mpCurrentKF,pKF,vpMapPointMatches,s,R,t,7.5);
                vnRound.push_back(i);
                vvpRoundMatches.push_back(vpMapPointMatches);
                vgScm.push_back(g2o::Sim3(R,t,s));
            }
        }
        vector<Optimizer::Sim3Problem> vProblems(vnRound.size());
        for(size_t k=0; k<vnRound.size(); k++)
            Optimizer::GatherSim3(mpCurrentKF, mvpEnoughConsistentCandidates[vnRound[k]], vvpRoundMatches[k], vgScm[k], 10, mbFixScale, vProblems[k]);
        std::string err;
        const int rc = Optimizer::OptimizeSim3Batch(matcher.Handle(), vProblems, &err);
        if (rc != ORBX_OK) { printf("OptimizeSim3Batch: %d %s\n", rc, err.c_str()); CHECK(rc == ORBX_OK); break; }
        out.optimised += (int)vnRound.size();
        for(size_t k=0; k<vnRound.size(); k++)
        {
            const int nInliers = Optimizer::ScatterSim3(vProblems[k], vvpRoundMatches[k], vgScm[k]);
            if(nInliers>=20)
            {
                bMatch = true;
                out.mpMatchedKF = mvpEnoughConsistentCandidates[vnRound[k]];
                out.gScm = vgScm[k];
                out.nInliers = nInliers;
                out.mvpCurrentMatchedPoints = vvpRoundMatches[k];
                break;
            }
        }
    }
    out.bMatch = bMatch;
    return out;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    const bool hostOnly = argc > 1 && !strcmp(argv[1], "host");
    double bars[3] = {0, 0, 0};
    if (!hostOnly) {
        if (argc < 4) { fprintf(stderr, "usage: %s compile-only | host | QBAR TBAR SBAR\n", argv[0]); return 2; }
        for (int k = 0; k < 3; k++) bars[k] = atof(argv[1 + k]);
    }
    Frame::mnMinX = 0.f; Frame::mnMaxX = W; Frame::mnMinY = 0.f; Frame::mnMaxY = H;
    Frame::mfGridElementWidthInv = 64.f / W; Frame::mfGridElementHeightInv = 48.f / H;
    for (int fix = 0; fix < 2; fix++) {
        const bool mbFixScale = fix != 0;
        Scene sc = make_scene(mbFixScale, 4242u + fix);
        vector<Lcg> srcA(3), srcB(3);
        if (hostOnly) {
            vector<Sim3Solver *> solvers = make_solvers(sc, srcA, mbFixScale);
            Outcome o = loop_reference(sc, solvers, nullptr, mbFixScale);
            CHECK(o.bMatch && o.mpMatchedKF == sc.mvpEnoughConsistentCandidates[1] && o.optimised == 2 && o.nInliers >= 40);
            CHECK(!mbFixScale || o.gScm[7] == 1.0);
            int kept = 0;
            for (size_t j = 0; j < o.mvpCurrentMatchedPoints.size(); j++)
                if (o.mvpCurrentMatchedPoints[j]) { kept++; CHECK(j % 6 != 5 && o.mvpCurrentMatchedPoints[j] == sc.vvpMapPointMatches[1][j]); }
            CHECK(kept == o.nInliers);
            printf("%s scale: host, candidate 1 after %d optimisations, nInliers %d\n", mbFixScale ? "fixed" : "free", o.optimised, o.nInliers);
            for (Sim3Solver *s : solvers) delete s;
        } else {
            ORBmatcher matcher(0.75,true);
            vector<Sim3Solver *> a = make_solvers(sc, srcA, mbFixScale), b = make_solvers(sc, srcB, mbFixScale);
            Outcome want = loop_reference(sc, a, &matcher, mbFixScale);
            Outcome got = loop_batched(sc, b, matcher, mbFixScale);
            CHECK(want.bMatch && want.mpMatchedKF == sc.mvpEnoughConsistentCandidates[1] && want.optimised == 2 && want.found > 10);
            CHECK(got.bMatch == want.bMatch && got.mpMatchedKF == want.mpMatchedKF && got.nInliers == want.nInliers && got.rounds == want.rounds);
            CHECK(got.mvpCurrentMatchedPoints == want.mvpCurrentMatchedPoints);
            int kept = 0, fromSearch = 0;
            for (size_t j = 0; j < want.mvpCurrentMatchedPoints.size(); j++)
                if (want.mvpCurrentMatchedPoints[j]) { kept++; fromSearch += j % 4 == 3; }
            // pairs SearchBySim3 added survive the optimisation; pair 28 can come back from it and is skipped by the gather (:1114)
            CHECK(kept - want.nInliers >= 0 && kept - want.nInliers <= 1 && fromSearch > 5);
            double d[3] = {0, 0, 0};
            for (int k = 0; k < 8; k++) d[k < 4 ? 0 : k < 7 ? 1 : 2] = max(d[k < 4 ? 0 : k < 7 ? 1 : 2], fabs(got.gScm[k] - want.gScm[k]));
            for (int k = 0; k < 3; k++) CHECK(d[k] <= bars[k]);
            CHECK(!mbFixScale || (got.gScm[7] == 1.0 && want.gScm[7] == 1.0));
            printf("%s scale: both loop forms, candidate 1, nInliers %d (%d from SearchBySim3), |d gScm| %.3g %.3g %.3g\n", mbFixScale ? "fixed" : "free",
                   want.nInliers, fromSearch, d[0], d[1], d[2]);
            for (Sim3Solver *s : a) delete s;
            for (Sim3Solver *s : b) delete s;
        }
        free_scene(sc);
    }
    if (g_fail) { printf("optimize_sim3_callsites: %d checks failed\n", g_fail); return 1; }
    printf("optimize_sim3_callsites ok\n");
    return 0;
}
