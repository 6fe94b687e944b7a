// PnPsolver.h / Optimizer -- the reference's pose-solver call shapes over include/orbp.h (host code inside liborbx.so).
// Reference: include/PnPsolver.h:66-78 (PnPsolver(const Frame&, const vector<MapPoint*>&), SetRansacParameters, find,
// iterate) and include/Optimizer.h (static int PoseOptimization(Frame*)).  Frame / MapPoint belong to the reference's
// object graph, so the constructor here takes what the reference constructor reads out of them
// (src/PnPsolver.cc:78-106); INTEGRATION.md 3d shows the five-line gather that keeps the original signature.
// Poses are row-major 4x4 float (the layout of the reference's CV_32F Tcw); an empty optional stands for the empty
// cv::Mat the reference returns.  PnPsolver::EvaluateAll is the one addition to the reference's interface: the EPnP
// hypotheses of all Relocalization candidates in one GPU call (orbm_pnp_hypotheses), replayed by iterate.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <mutex>
#include <optional>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/orbm.h"
#include "../../include/orbp.h"

namespace ORB_SLAM2 {

typedef std::array<float, 16> Pose;

class PnPsolver {
public:
    // p2d[i] = F.mvKeysUn[idx].pt, sigma2[i] = F.mvLevelSigma2[octave], p3d[i] = pMP->GetWorldPos(); keyPointIndices[i] = idx
    PnPsolver(const std::vector<float> &p2d, const std::vector<float> &sigma2, const std::vector<float> &p3d,
              const std::vector<size_t> &keyPointIndices, size_t nFrameFeatures, float fx, float fy, float cx, float cy)
        : mvKeyPointIndices(keyPointIndices), mnFrameFeatures(nFrameFeatures)
    {
        if (orbp_pnp_create(&s_, (int)sigma2.size(), p2d.data(), sigma2.data(), p3d.data(), fx, fy, cx, cy) < 0) { err_ = orbp_last_error(); s_ = nullptr; }
    }
    ~PnPsolver() { orbp_pnp_destroy(s_); }
    PnPsolver(const PnPsolver &) = delete;
    PnPsolver &operator=(const PnPsolver &) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4, float th2 = 5.991)
    {
        if (s_ && orbp_pnp_set_ransac_parameters(s_, probability, minInliers, maxIterations, minSet, epsilon, th2) < 0) err_ = orbp_last_error();
    }

    // the uniform source of the RANSAC draws (orbp_pnp_set_rand): fn(ctx) in [0, randMax]; NULL restores libc rand()
    void SetRand(int (*fn)(void *), void *ctx, int randMax) { if (s_) orbp_pnp_set_rand(s_, fn, ctx, randMax); }

    std::optional<Pose> find(std::vector<bool> &vbInliers, int &nInliers)
    {
        bool flag;
        int maxIts = 0;
        if (s_) orbp_pnp_get_ransac_state(s_, nullptr, &maxIts, nullptr, nullptr);
        return iterate(maxIts, flag, vbInliers, nInliers);
    }

    // vbInliers is indexed like the frame's features (src/PnPsolver.cc:226-231)
    std::optional<Pose> iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false; vbInliers.clear(); nInliers = 0;
        if (!s_) { bNoMore = true; return std::nullopt; }
        std::vector<uint8_t> inl(mvKeyPointIndices.size() + 1);
        Pose T;
        int noMore = 0;
        const int got = orbp_pnp_iterate(s_, nIterations, &noMore, inl.data(), &nInliers, T.data());
        bNoMore = noMore != 0;
        if (got <= 0) { if (got < 0) err_ = orbp_last_error(); return std::nullopt; }
        vbInliers.assign(mnFrameFeatures, false);
        for (size_t i = 0; i < mvKeyPointIndices.size(); i++)
            if (inl[i]) vbInliers[mvKeyPointIndices[i]] = true;
        return T;
    }

    // The batch step of Tracking::Relocalization, one line in front of `while(nCandidates>0 && !bMatch)` (src/Tracking.cc:1403):
    // every solver draws what its next iterate(nIterations) consumes (solver by solver, so the rand() stream is the one the
    // reference's first round of iterate calls consumes), all drawn sets are evaluated by ONE orbm_pnp_hypotheses call on the
    // matcher's handle, and the results are attached: the iterate calls that follow replay them.  NULL entries (discarded
    // candidates) and solvers with mRansacMinSet > 8 are skipped; the latter evaluate on the host as before.  Returns the ORBX
    // status; on failure (*err receives the text) the solvers keep their drawn sets and evaluate them on the host.
    static int EvaluateAll(const std::vector<PnPsolver *> &vpPnPsolvers, orbm_matcher *m, int nIterations = 5, std::string *err = nullptr)
    {
        return EvaluateAllWith(vpPnPsolvers, nIterations, err, [m](auto... a) { return orbm_pnp_hypotheses(m, a...); },
                               [] { return std::string(orbm_last_error()); });
    }
    // the same through ORBmatcher::PnPHypotheses (ORBmatcher.h), which owns the handle
    template <class Matcher>
    static int EvaluateAll(const std::vector<PnPsolver *> &vpPnPsolvers, Matcher &matcher, int nIterations = 5, std::string *err = nullptr)
    {
        return EvaluateAllWith(vpPnPsolvers, nIterations, err, [&matcher](auto... a) { return matcher.PnPHypotheses(a...); },
                               [&matcher] { return std::string(matcher.LastError()); });
    }

    bool Valid() const { return s_ != nullptr; }
    const std::string &LastError() const { return err_; }

private:
    template <class Call, class Text>
    static int EvaluateAllWith(const std::vector<PnPsolver *> &vpPnPsolvers, int nIterations, std::string *err, Call call, Text text)
    {
        std::vector<PnPsolver *> live;
        std::vector<int32_t> off(1, 0), hypOff(1, 0), samples;
        std::vector<int64_t> maskOff(1, 0);
        std::vector<float> p2d, p3d, maxErr;
        std::vector<orbm_pnp_camera> cams;
        std::vector<int32_t> sets;
        for (PnPsolver *p : vpPnPsolvers) {
            if (!p || !p->s_) continue;
            orbp_pnp *s = p->s_;
            const int n = (int)p->mvKeyPointIndices.size();
            const size_t c0 = maxErr.size();
            p2d.resize(2 * (c0 + n)); p3d.resize(3 * (c0 + n)); maxErr.resize(c0 + n);
            float K[4];
            int32_t minSet = 0;
            orbp_pnp_get_problem(s, p2d.data() + 2 * c0, p3d.data() + 3 * c0, maxErr.data() + c0, K, &minSet);
            if (minSet > ORBM_PNP_MAX_SET) { p2d.resize(2 * c0); p3d.resize(3 * c0); maxErr.resize(c0); continue; }
            orbp_pnp_draw(s, nIterations, nullptr);
            const int h = orbp_pnp_queued(s, nullptr);
            sets.resize((size_t)h * minSet + 1);
            orbp_pnp_queued(s, sets.data());
            const size_t s0 = samples.size();
            samples.resize(s0 + (size_t)ORBM_PNP_MAX_SET * h, -1);
            for (int k = 0; k < h; k++)
                for (int j = 0; j < minSet; j++) samples[s0 + (size_t)ORBM_PNP_MAX_SET * k + j] = sets[(size_t)k * minSet + j];
            cams.push_back({K[0], K[1], K[2], K[3], minSet});
            off.push_back(off.back() + n);
            hypOff.push_back(hypOff.back() + h);
            maskOff.push_back(maskOff.back() + (int64_t)h * ((n + 31) / 32));
            live.push_back(p);
        }
        const size_t H = (size_t)hypOff.back();
        std::vector<int32_t> counts(H + 1);
        std::vector<double> Rt(12 * H + 1);
        std::vector<uint32_t> masks((size_t)maskOff.back() + 1);
        samples.push_back(-1);       // never an empty vector's NULL data()
        const int rc = call((int)live.size(), (const int32_t *)off.data(), (const float *)p2d.data(), (const float *)p3d.data(),
                            (const float *)maxErr.data(), (const orbm_pnp_camera *)cams.data(), (const int32_t *)hypOff.data(),
                            (const int32_t *)samples.data(), (const int64_t *)maskOff.data(), counts.data(), Rt.data(), masks.data());
        if (rc != ORBX_OK) { if (err) *err = text(); return rc; }
        for (size_t k = 0; k < live.size(); k++)
            if (orbp_pnp_attach_results(live[k]->s_, hypOff[k + 1] - hypOff[k], counts.data() + hypOff[k], Rt.data() + 12 * (size_t)hypOff[k],
                                        masks.data() + maskOff[k]) < 0) {
                if (err) *err = orbp_last_error();
                return ORBX_E_INVALID;
            }
        return ORBX_OK;
    }
    orbp_pnp *s_ = nullptr;
    std::vector<size_t> mvKeyPointIndices;
    size_t mnFrameFeatures;
    std::string err_;
};

class Optimizer {
public:
    // Optimizer::PoseOptimization(Frame*) on the arrays it gathers (src/Optimizer.cc:277-355): one entry per feature with
    // a MapPoint.  Tcw is pFrame->mTcw in and the optimised pose out; outlier receives mvbOutlier for those features.
    static int PoseOptimization(const std::vector<float> &obs, const std::vector<float> &uRight, const std::vector<float> &invSigma2,
                                const std::vector<float> &Xw, float fx, float fy, float cx, float cy, float bf, Pose &Tcw,
                                std::vector<bool> &outlier)
    {
        const int n = (int)invSigma2.size();
        std::vector<uint8_t> o(n + 1);
        const int good = orbp_pose_optimization(n, obs.data(), uRight.empty() ? nullptr : uRight.data(), invSigma2.data(), Xw.data(),
                                                fx, fy, cx, cy, bf, Tcw.data(), o.data());
        outlier.assign(o.begin(), o.begin() + n);
        return good;
    }

    // One problem of PoseOptimizationBatch: the arguments of PoseOptimization above, and its results (outlier, nGood = the
    // return value).  uRight empty: every edge of this problem is monocular.
    struct PoseProblem {
        std::vector<float> obs, uRight, invSigma2, Xw;
        float fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;
        Pose Tcw{};
        std::vector<bool> outlier;
        int nGood = 0;
    };
    // PoseOptimization for every problem in one GPU launch (orbm_pose_optimization_batch, include/orbm.h): the frames of a step,
    // or the candidates of Tracking::Relocalization.  Returns the ORBX status; on failure no problem is
    // changed and *err receives orbm_last_error().
    static int PoseOptimizationBatch(orbm_matcher *matcher, std::vector<PoseProblem> &problems, std::string *err = nullptr)
    {
        const int B = (int)problems.size();
        std::vector<int32_t> off(B + 1, 0);
        bool anyStereo = false;
        for (int p = 0; p < B; p++) {
            off[p + 1] = off[p] + (int32_t)problems[p].invSigma2.size();
            anyStereo = anyStereo || !problems[p].uRight.empty();
        }
        const size_t N = (size_t)off[B];
        std::vector<float> obs, ur, s2, xw, T(16 * (size_t)B);
        std::vector<orbm_pose_camera> cams(B);
        obs.reserve(2 * N); s2.reserve(N); xw.reserve(3 * N);
        for (int p = 0; p < B; p++) {
            const PoseProblem &P = problems[p];
            const size_t n = P.invSigma2.size();
            if (P.obs.size() != 2 * n || P.Xw.size() != 3 * n || (!P.uRight.empty() && P.uRight.size() != n)) {
                if (err) *err = "PoseOptimizationBatch: array lengths of problem " + std::to_string(p) + " disagree";
                return ORBX_E_INVALID;
            }
            obs.insert(obs.end(), P.obs.begin(), P.obs.end());
            s2.insert(s2.end(), P.invSigma2.begin(), P.invSigma2.end());
            xw.insert(xw.end(), P.Xw.begin(), P.Xw.end());
            if (anyStereo) {
                if (P.uRight.empty()) ur.insert(ur.end(), n, -1.0f);
                else ur.insert(ur.end(), P.uRight.begin(), P.uRight.end());
            }
            cams[p] = {P.fx, P.fy, P.cx, P.cy, P.bf};
            for (int k = 0; k < 16; k++) T[16 * (size_t)p + k] = P.Tcw[k];
        }
        std::vector<uint8_t> o(N + 1);
        std::vector<int32_t> good(B + 1);
        const int rc = orbm_pose_optimization_batch(matcher, B, off.data(), obs.data(), anyStereo ? ur.data() : nullptr, s2.data(), xw.data(),
                                                    cams.data(), T.data(), o.data(), good.data());
        if (rc != ORBX_OK) { if (err) *err = orbm_last_error(); return rc; }
        for (int p = 0; p < B; p++) {
            PoseProblem &P = problems[p];
            for (int k = 0; k < 16; k++) P.Tcw[k] = T[16 * (size_t)p + k];
            P.outlier.assign(o.begin() + off[p], o.begin() + off[p + 1]);
            P.nGood = good[p];
        }
        return ORBX_OK;
    }

    // ---- Optimizer::OptimizeSim3 (include/Optimizer.h, src/Optimizer.cc:1046-1241; LoopClosing::ComputeSim3, src/LoopClosing.cc:327) ----
    // One problem: what the reference feeds to g2o (:1059-1178), and its results.  index[k] = vnIndexEdge[k], the slot of vpMatches1
    // correspondence k came from; S12 is g2oS12 in the order of g2o::Sim3::operator[] (qx, qy, qz, qw, tx, ty, tz, s), in and out.
    struct Sim3Problem {
        std::vector<float> x1c, x2c, obs1, obs2, invSigma2_1, invSigma2_2;
        std::vector<size_t> index;
        float K1[4] = {0, 0, 0, 0}, K2[4] = {0, 0, 0, 0};
        float th2 = 10.f;
        bool fixScale = true;
        double S12[8] = {0, 0, 0, 1, 0, 0, 0, 1};
        std::vector<bool> removed;          // per correspondence: the reference sets vpMatches1[index[k]] = NULL
        int nIn = 0;                        // the return value
    };
    // The gather of :1059-1178 with its skips (:1101, :1112-1136) and GetIndexInKeyFrame (:1110).  g2oS12 is read through operator[]
    // only.  The calibration is read from pKF->fx, fy, cx, cy (the entries of the mK the reference reads).
    template <class KeyFrameT, class MapPointT, class Sim3T>
    static void GatherSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatches1, const Sim3T &g2oS12, const float th2,
                           const bool bFixScale, Sim3Problem &P)
    {
        P = Sim3Problem();
        P.K1[0] = pKF1->fx; P.K1[1] = pKF1->fy; P.K1[2] = pKF1->cx; P.K1[3] = pKF1->cy;
        P.K2[0] = pKF2->fx; P.K2[1] = pKF2->fy; P.K2[2] = pKF2->cx; P.K2[3] = pKF2->cy;
        P.th2 = th2; P.fixScale = bFixScale;
        for (int k = 0; k < 8; k++) P.S12[k] = g2oS12[k];
        const auto R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation(), R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
        const int N = (int)vpMatches1.size();
        const std::vector<MapPointT *> vpMapPoints1 = pKF1->GetMapPointMatches();
        for (int i = 0; i < N; i++) {
            if (!vpMatches1[i]) continue;                                   // :1101
            MapPointT *pMP1 = vpMapPoints1[i];
            MapPointT *pMP2 = vpMatches1[i];
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);                  // :1110
            if (!(pMP1 && pMP2)) continue;                                  // :1112, :1135-1136
            if (!(!pMP1->isBad() && !pMP2->isBad() && i2 >= 0)) continue;   // :1114, :1132-1133
            sim3_to_camera(R1w, t1w, pMP1->GetWorldPos(), P.x1c);           // :1117-1119
            sim3_to_camera(R2w, t2w, pMP2->GetWorldPos(), P.x2c);           // :1125-1127
            const auto &kpUn1 = pKF1->mvKeysUn[i];
            P.obs1.push_back(kpUn1.pt.x); P.obs1.push_back(kpUn1.pt.y);
            P.invSigma2_1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
            const auto &kpUn2 = pKF2->mvKeysUn[i2];
            P.obs2.push_back(kpUn2.pt.x); P.obs2.push_back(kpUn2.pt.y);
            P.invSigma2_2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
            P.index.push_back((size_t)i);                                   // :1177
        }
    }
    // the results of a solved problem on the caller's objects: NULL into vpMatches1 from the flags (:1196, :1230), g2oS12 through
    // operator[] (:1238; a problem that returned at :1212 holds the S12 it came with)
    template <class MapPointT, class Sim3T>
    static int ScatterSim3(const Sim3Problem &P, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12)
    {
        for (size_t k = 0; k < P.index.size(); k++)
            if (P.removed[k]) vpMatches1[P.index[k]] = static_cast<MapPointT *>(NULL);
        for (int k = 0; k < 8; k++) g2oS12[k] = P.S12[k];
        return P.nIn;
    }
    // The reference's signature (MapPointT deduces to MapPoint), so src/LoopClosing.cc:327 compiles unchanged; on the host
    // (orbp_optimize_sim3), which is the faster call for one candidate (README).  < 0 on bad arguments (orbp_last_error()).
    template <class KeyFrameT, class MapPointT, class Sim3T>
    static int OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale)
    {
        Sim3Problem P;
        GatherSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, P);
        const int n = (int)P.index.size();
        std::vector<uint8_t> flags(n + 1);
        const int nIn = orbp_optimize_sim3(n, P.x1c.data(), P.x2c.data(), P.obs1.data(), P.obs2.data(), P.invSigma2_1.data(), P.invSigma2_2.data(),
                                           P.K1, P.K2, th2, bFixScale ? 1 : 0, P.S12, flags.data());
        if (nIn < 0) return nIn;
        P.removed.assign(flags.begin(), flags.begin() + n);
        P.nIn = nIn;
        return ScatterSim3(P, vpMatches1, g2oS12);
    }
    // OptimizeSim3 for every problem in one GPU launch (orbm_optimize_sim3_batch, include/orbm.h): the candidates of one round of
    // LoopClosing::ComputeSim3 that returned a Scm.  Returns the ORBX status; on failure no problem is changed and
    // *err receives the text.
    static int OptimizeSim3Batch(orbm_matcher *matcher, std::vector<Sim3Problem> &problems, std::string *err = nullptr)
    {
        const int B = (int)problems.size();
        std::vector<int32_t> off(B + 1, 0), fix(B + 1);
        for (int p = 0; p < B; p++) off[p + 1] = off[p] + (int32_t)problems[p].index.size();
        const size_t N = (size_t)off[B];
        std::vector<float> x1, x2, o1, o2, s1, s2, cams(8 * (size_t)B + 1), th2(B + 1);
        std::vector<double> S(8 * (size_t)B + 1);
        x1.reserve(3 * N + 1); x2.reserve(3 * N + 1); o1.reserve(2 * N + 1); o2.reserve(2 * N + 1); s1.reserve(N + 1); s2.reserve(N + 1);
        for (int p = 0; p < B; p++) {
            const Sim3Problem &P = problems[p];
            const size_t n = P.index.size();
            if (P.x1c.size() != 3 * n || P.x2c.size() != 3 * n || P.obs1.size() != 2 * n || P.obs2.size() != 2 * n || P.invSigma2_1.size() != n ||
                P.invSigma2_2.size() != n) {
                if (err) *err = "OptimizeSim3Batch: array lengths of problem " + std::to_string(p) + " disagree";
                return ORBX_E_INVALID;
            }
            x1.insert(x1.end(), P.x1c.begin(), P.x1c.end()); x2.insert(x2.end(), P.x2c.begin(), P.x2c.end());
            o1.insert(o1.end(), P.obs1.begin(), P.obs1.end()); o2.insert(o2.end(), P.obs2.begin(), P.obs2.end());
            s1.insert(s1.end(), P.invSigma2_1.begin(), P.invSigma2_1.end()); s2.insert(s2.end(), P.invSigma2_2.begin(), P.invSigma2_2.end());
            for (int k = 0; k < 4; k++) { cams[8 * (size_t)p + k] = P.K1[k]; cams[8 * (size_t)p + 4 + k] = P.K2[k]; }
            th2[p] = P.th2; fix[p] = P.fixScale ? 1 : 0;
            for (int k = 0; k < 8; k++) S[8 * (size_t)p + k] = P.S12[k];
        }
        x1.push_back(0.f); x2.push_back(0.f); o1.push_back(0.f); o2.push_back(0.f); s1.push_back(0.f); s2.push_back(0.f);      // never NULL
        std::vector<uint8_t> flags(N + 1);
        std::vector<int32_t> nIn(B + 1);
        const int rc = orbm_optimize_sim3_batch(matcher, B, off.data(), x1.data(), x2.data(), o1.data(), o2.data(), s1.data(), s2.data(), cams.data(),
                                                th2.data(), fix.data(), S.data(), flags.data(), nIn.data());
        if (rc != ORBX_OK) { if (err) *err = orbm_last_error(); return rc; }
        for (int p = 0; p < B; p++) {
            Sim3Problem &P = problems[p];
            for (int k = 0; k < 8; k++) P.S12[k] = S[8 * (size_t)p + k];
            P.removed.assign(flags.begin() + off[p], flags.begin() + off[p + 1]);
            P.nIn = nIn[p];
        }
        return ORBX_OK;
    }

    // ---- Optimizer::LocalBundleAdjustment (include/Optimizer.h, src/Optimizer.cc:453-778; LocalMapping::Run, src/LocalMapping.cc:82) ----
    // The flat problem of orbp_local_bundle_adjustment (include/orbp.h) and the objects its rows stand for.
    template <class KeyFrameT, class MapPointT>
    struct LbaProblem {
        std::vector<KeyFrameT *> local, fixed;              // lLocalKeyFrames, lFixedCameras
        std::vector<MapPointT *> points;                    // lLocalMapPoints
        std::vector<KeyFrameT *> edgeKF;                    // per edge: vpEdgeKFMono / vpEdgeKFStereo
        std::vector<uint8_t> localFixed;
        std::vector<float> Tcw, cam, xw, obs, uRight, invSigma2;
        std::vector<int32_t> edgeOff, edgeKf;
        // results
        std::vector<float> TcwLocal;
        std::vector<uint8_t> erase;
        orbp_lba_stats stats{};
        orbp_lba_problem flat() const
        {
            return {(int32_t)local.size(), (int32_t)fixed.size(), (int32_t)points.size(), localFixed.data(), Tcw.data(), cam.data(), edgeOff.data(),
                    edgeKf.data(), obs.data(), uRight.data(), invSigma2.data()};
        }
    };
    // The gather of :455-504 with its marks (mnBALocalForKF, mnBAFixedForKF) and isBad skips, and the edge walk :572-653
    template <class KeyFrameT, class MapPointT>
    static void GatherLocalBundleAdjustment(KeyFrameT *pKF, LbaProblem<KeyFrameT, MapPointT> &P)
    {
        P = LbaProblem<KeyFrameT, MapPointT>();
        P.local.push_back(pKF);                                             // :458-459
        pKF->mnBALocalForKF = pKF->mnId;
        const std::vector<KeyFrameT *> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
        for (int i = 0, iend = (int)vNeighKFs.size(); i < iend; i++) {      // :462-468
            KeyFrameT *pKFi = vNeighKFs[i];
            pKFi->mnBALocalForKF = pKF->mnId;
            if (!pKFi->isBad()) P.local.push_back(pKFi);
        }
        for (KeyFrameT *pKFi : P.local) {                                   // :472-486
            std::vector<MapPointT *> vpMPs = pKFi->GetMapPointMatches();
            for (MapPointT *pMP : vpMPs)
                if (pMP)
                    if (!pMP->isBad())
                        if (pMP->mnBALocalForKF != pKF->mnId) {
                            P.points.push_back(pMP);
                            pMP->mnBALocalForKF = pKF->mnId;
                        }
        }
        for (MapPointT *pMP : P.points) {                                   // :490-504
            auto observations = pMP->GetObservations();
            for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                KeyFrameT *pKFi = mit->first;
                if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                    pKFi->mnBAFixedForKF = pKF->mnId;
                    if (!pKFi->isBad()) P.fixed.push_back(pKFi);
                }
            }
        }
        std::map<KeyFrameT *, int32_t> index;                               // optimizer.vertex(pKFi->mnId)
        auto addKF = [&](KeyFrameT *pKFi) {                                 // :523-546
            index[pKFi] = (int32_t)index.size();
            const auto T = pKFi->GetPose();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) P.Tcw.push_back(T.template at<float>(r, c));
            P.cam.push_back(pKFi->fx); P.cam.push_back(pKFi->fy); P.cam.push_back(pKFi->cx); P.cam.push_back(pKFi->cy); P.cam.push_back(pKFi->mbf);
        };
        for (KeyFrameT *pKFi : P.local) { addKF(pKFi); P.localFixed.push_back(pKFi->mnId == 0 ? 1 : 0); }
        for (KeyFrameT *pKFi : P.fixed) addKF(pKFi);
        P.edgeOff.push_back(0);
        for (MapPointT *pMP : P.points) {                                   // :572-653
            const auto X = pMP->GetWorldPos();
            for (int r = 0; r < 3; r++) P.xw.push_back(X.template at<float>(r));
            const auto observations = pMP->GetObservations();
            for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                KeyFrameT *pKFi = mit->first;
                if (pKFi->isBad()) continue;                                // :589
                const auto it = index.find(pKFi);
                if (it == index.end()) continue;                            // a bad key frame at :500 that is good again: no vertex
                const auto &kpUn = pKFi->mvKeysUn[mit->second];
                P.edgeKf.push_back(it->second);
                P.edgeKF.push_back(pKFi);
                P.obs.push_back(kpUn.pt.x); P.obs.push_back(kpUn.pt.y);
                const float ur = pKFi->mvuRight[mit->second];
                P.uRight.push_back(ur < 0 ? -1.f : ur);                     // :594
                P.invSigma2.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
            }
            P.edgeOff.push_back((int32_t)P.edgeKf.size());
        }
        P.TcwLocal.assign(16 * P.local.size() + 1, 0.f);
        P.erase.assign(P.edgeKf.size() + 1, 0);
        P.Tcw.push_back(0.f); P.cam.push_back(0.f); P.xw.push_back(0.f); P.obs.push_back(0.f); P.uRight.push_back(0.f);       // never NULL
        P.invSigma2.push_back(0.f); P.edgeKf.push_back(0); P.localFixed.push_back(0);
    }
    // :745-777 in order, under pMap->mMutexMapUpdate: the erased pairs (points that turned bad during the solve are skipped as :720
    // and :735 do), SetPose, SetWorldPos and UpdateNormalAndDepth
    template <class KeyFrameT, class MapPointT, class MapT>
    static void ScatterLocalBundleAdjustment(const LbaProblem<KeyFrameT, MapPointT> &P, MapT *pMap)
    {
        std::vector<std::pair<KeyFrameT *, MapPointT *>> vToErase;
        for (int pass = 0; pass < 2; pass++)                                // the monocular edges first, then the stereo ones (:715-743)
            for (size_t p = 0; p < P.points.size(); p++) {
                if (P.points[p]->isBad()) continue;
                for (int32_t e = P.edgeOff[p]; e < P.edgeOff[p + 1]; e++)
                    if (P.erase[e] && (P.uRight[e] < 0) == (pass == 0)) vToErase.push_back(std::make_pair(P.edgeKF[e], P.points[p]));
            }
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);           // :746
        for (size_t i = 0; i < vToErase.size(); i++) {                      // :748-757
            vToErase[i].first->EraseMapPointMatch(vToErase[i].second);
            vToErase[i].second->EraseObservation(vToErase[i].first);
        }
        for (size_t k = 0; k < P.local.size(); k++) {                       // :762-768
            auto T = P.local[k]->GetPose().clone();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T.template at<float>(r, c) = P.TcwLocal[16 * k + 4 * r + c];
            P.local[k]->SetPose(T);
        }
        for (size_t p = 0; p < P.points.size(); p++) {                      // :771-777
            auto X = P.points[p]->GetWorldPos().clone();
            for (int r = 0; r < 3; r++) X.template at<float>(r) = P.xw[3 * p + r];
            P.points[p]->SetWorldPos(X);
            P.points[p]->UpdateNormalAndDepth();
        }
    }
    // The reference's signature, so src/LocalMapping.cc:82 compiles unchanged; on the host (orbp_local_bundle_adjustment): which
    // path is faster at which size is in README and INTEGRATION.md 3p.  pbStopFlag is read while the solver runs, as g2o reads it.
    template <class KeyFrameT, class MapT>
    static void LocalBundleAdjustment(KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap)
    {
        (void)LocalBundleAdjustment(static_cast<orbm_matcher *>(nullptr), pKF, pbStopFlag, pMap);
    }
    // The same through orbm_local_bundle_adjustment on the matcher's handle (NULL: the host path).  Returns ORBP_LBA_DONE,
    // ORBP_LBA_STOPPED (:655-657: nothing is written back) or the ORBX status; on failure nothing is changed and *err receives the text.
    template <class KeyFrameT, class MapT>
    static int LocalBundleAdjustment(orbm_matcher *matcher, KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap, std::string *err = nullptr,
                                     orbp_lba_stats *stats = nullptr)
    {
        typedef typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type MapPointT;
        static_assert(sizeof(bool) == 1, "pbStopFlag is read as a byte");
        LbaProblem<KeyFrameT, MapPointT> P;
        GatherLocalBundleAdjustment(pKF, P);
        const orbp_lba_problem flat = P.flat();
        const volatile uint8_t *stop = reinterpret_cast<const volatile uint8_t *>(pbStopFlag);
        const int rc = matcher ? orbm_local_bundle_adjustment(matcher, &flat, P.TcwLocal.data(), P.xw.data(), P.erase.data(), stop, &P.stats)
                               : orbp_local_bundle_adjustment(&flat, P.TcwLocal.data(), P.xw.data(), P.erase.data(), stop, &P.stats);
        if (rc < 0) { if (err) *err = matcher ? orbm_last_error() : orbp_last_error(); return rc; }
        if (stats) *stats = P.stats;
        if (rc == ORBP_LBA_DONE) ScatterLocalBundleAdjustment(P, pMap);
        return rc;
    }

    // ---- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (include/Optimizer.h:40-44, src/Optimizer.cc:41-237;
    // Tracking::CreateInitialMapMonocular, src/Tracking.cc:695; LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:651) ----
    // The flat problem of orbp_bundle_adjustment (include/orbp.h) and the objects its rows stand for.
    template <class KeyFrameT, class MapPointT>
    struct BaProblem {
        std::vector<KeyFrameT *> kfs;                       // the non-bad vpKFs: the vertices
        std::vector<MapPointT *> points;                    // the non-bad vpMP
        std::vector<uint8_t> included;                      // per point: !vbNotIncludedMP (nEdges > 0, :175-183)
        std::vector<uint8_t> localFixed;
        std::vector<float> Tcw, cam, xw, obs, uRight, invSigma2;
        std::vector<int32_t> edgeOff, edgeKf;
        std::vector<float> TcwOut;
        orbp_ba_stats stats{};
        orbp_lba_problem flat() const
        {
            return {(int32_t)kfs.size(), 0, (int32_t)points.size(), localFixed.data(), Tcw.data(), cam.data(), edgeOff.data(), edgeKf.data(),
                    obs.data(), uRight.data(), invSigma2.data()};
        }
    };
    // The walk of :71-184.  An observation counts towards nEdges unless its key frame is bad or has mnId > maxKFid (:109-112); it
    // becomes an edge only where that key frame is among the vertices (g2o's addEdge refuses an edge with a missing vertex).
    template <class KeyFrameT, class MapPointT>
    static void GatherBundleAdjustment(const std::vector<KeyFrameT *> &vpKFs, const std::vector<MapPointT *> &vpMP, BaProblem<KeyFrameT, MapPointT> &P)
    {
        P = BaProblem<KeyFrameT, MapPointT>();
        std::map<KeyFrameT *, int32_t> index;               // optimizer.vertex(pKF->mnId)
        long unsigned int maxKFid = 0;
        for (size_t i = 0; i < vpKFs.size(); i++) {         // :71-83
            KeyFrameT *pKF = vpKFs[i];
            if (pKF->isBad()) continue;
            index[pKF] = (int32_t)P.kfs.size();
            P.kfs.push_back(pKF);
            const auto T = pKF->GetPose();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) P.Tcw.push_back(T.template at<float>(r, c));
            P.cam.push_back(pKF->fx); P.cam.push_back(pKF->fy); P.cam.push_back(pKF->cx); P.cam.push_back(pKF->cy); P.cam.push_back(pKF->mbf);
            P.localFixed.push_back(pKF->mnId == 0 ? 1 : 0);
            if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
        }
        P.edgeOff.push_back(0);
        for (size_t i = 0; i < vpMP.size(); i++) {          // :89-184
            MapPointT *pMP = vpMP[i];
            if (pMP->isBad()) continue;
            P.points.push_back(pMP);
            const auto X = pMP->GetWorldPos();
            for (int r = 0; r < 3; r++) P.xw.push_back(X.template at<float>(r));
            const auto observations = pMP->GetObservations();
            int nEdges = 0;
            for (auto mit = observations.begin(); mit != observations.end(); mit++) {
                KeyFrameT *pKF = mit->first;
                if (pKF->isBad() || pKF->mnId > maxKFid) continue;
                nEdges++;
                const auto it = index.find(pKF);
                if (it == index.end()) continue;
                const auto &kpUn = pKF->mvKeysUn[mit->second];
                P.edgeKf.push_back(it->second);
                P.obs.push_back(kpUn.pt.x); P.obs.push_back(kpUn.pt.y);
                const float ur = pKF->mvuRight[mit->second];
                P.uRight.push_back(ur < 0 ? -1.f : ur);     // :116
                P.invSigma2.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
            }
            P.included.push_back(nEdges > 0 ? 1 : 0);
            P.edgeOff.push_back((int32_t)P.edgeKf.size());
        }
        P.TcwOut.assign(16 * P.kfs.size() + 1, 0.f);
        P.Tcw.push_back(0.f); P.cam.push_back(0.f); P.xw.push_back(0.f); P.obs.push_back(0.f); P.uRight.push_back(0.f);       // never NULL
        P.invSigma2.push_back(0.f); P.edgeKf.push_back(0); P.localFixed.push_back(0);
    }
    // :190-235: SetPose / SetWorldPos + UpdateNormalAndDepth when nLoopKF == 0, else mTcwGBA / mPosGBA and mnBAGlobalForKF.  Key
    // frames and points that turned bad during the solve are skipped, as :196 and :220 skip them.
    template <class KeyFrameT, class MapPointT>
    static void ScatterBundleAdjustment(const BaProblem<KeyFrameT, MapPointT> &P, const unsigned long nLoopKF)
    {
        for (size_t k = 0; k < P.kfs.size(); k++) {
            KeyFrameT *pKF = P.kfs[k];
            if (pKF->isBad()) continue;
            auto T = pKF->GetPose().clone();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T.template at<float>(r, c) = P.TcwOut[16 * k + 4 * r + c];
            if (nLoopKF == 0) pKF->SetPose(T);
            else {
                pKF->mTcwGBA = T;                               // :206-207: a 4 x 4 CV_32F matrix of its own (T is a clone)
                pKF->mnBAGlobalForKF = nLoopKF;
            }
        }
        for (size_t p = 0; p < P.points.size(); p++) {
            if (!P.included[p]) continue;
            MapPointT *pMP = P.points[p];
            if (pMP->isBad()) continue;
            auto X = pMP->GetWorldPos().clone();
            for (int r = 0; r < 3; r++) X.template at<float>(r) = P.xw[3 * p + r];
            if (nLoopKF == 0) {
                pMP->SetWorldPos(X);
                pMP->UpdateNormalAndDepth();
            } else {
                pMP->mPosGBA = X;                               // :231-232
                pMP->mnBAGlobalForKF = nLoopKF;
            }
        }
    }
    // Through orbm_bundle_adjustment on the matcher's handle (NULL: the host path, orbp_bundle_adjustment).  Returns 0 or the ORBX
    // status; on failure nothing is changed and *err receives the text.  Which path to call at which size: INTEGRATION.md 3q.
    template <class KeyFrameT, class MapPointT>
    static int BundleAdjustment(orbm_matcher *matcher, const std::vector<KeyFrameT *> &vpKFs, const std::vector<MapPointT *> &vpMP, std::string *err,
                                int nIterations = 5, bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true,
                                orbp_ba_stats *stats = nullptr)
    {
        static_assert(sizeof(bool) == 1, "pbStopFlag is read as a byte");
        BaProblem<KeyFrameT, MapPointT> P;
        GatherBundleAdjustment(vpKFs, vpMP, P);
        const orbp_lba_problem flat = P.flat();
        const volatile uint8_t *stop = reinterpret_cast<const volatile uint8_t *>(pbStopFlag);
        const int rc = matcher ? orbm_bundle_adjustment(matcher, &flat, nIterations, bRobust ? 1 : 0, P.TcwOut.data(), P.xw.data(), stop, &P.stats)
                               : orbp_bundle_adjustment(&flat, nIterations, bRobust ? 1 : 0, P.TcwOut.data(), P.xw.data(), stop, &P.stats);
        if (rc < 0) { if (err) *err = matcher ? orbm_last_error() : orbp_last_error(); return rc; }
        if (stats) *stats = P.stats;
        ScatterBundleAdjustment(P, nLoopKF);
        return rc;
    }
    template <class MapT>
    static int GlobalBundleAdjustemnt(orbm_matcher *matcher, MapT *pMap, std::string *err, int nIterations = 5, bool *pbStopFlag = NULL,
                                      const unsigned long nLoopKF = 0, const bool bRobust = true, orbp_ba_stats *stats = nullptr)
    {
        const auto vpKFs = pMap->GetAllKeyFrames();             // :43-45
        const auto vpMP = pMap->GetAllMapPoints();
        return BundleAdjustment(matcher, vpKFs, vpMP, err, nIterations, pbStopFlag, nLoopKF, bRobust, stats);
    }
    // The reference's signatures and defaults (include/Optimizer.h:40-44), so src/Tracking.cc:695 and src/LoopClosing.cc:651 compile
    // unchanged; on the host.
    template <class KeyFrameT, class MapPointT>
    static void BundleAdjustment(const std::vector<KeyFrameT *> &vpKF, const std::vector<MapPointT *> &vpMP, int nIterations = 5,
                                 bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true)
    {
        (void)BundleAdjustment(static_cast<orbm_matcher *>(nullptr), vpKF, vpMP, static_cast<std::string *>(nullptr), nIterations, pbStopFlag,
                               nLoopKF, bRobust);
    }
    template <class MapT>
    static void GlobalBundleAdjustemnt(MapT *pMap, int nIterations = 5, bool *pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                                       const bool bRobust = true)
    {
        (void)GlobalBundleAdjustemnt(static_cast<orbm_matcher *>(nullptr), pMap, static_cast<std::string *>(nullptr), nIterations, pbStopFlag,
                                     nLoopKF, bRobust);
    }

    // ---- Optimizer::OptimizeEssentialGraph (include/Optimizer.h, src/Optimizer.cc:781-1044; LoopClosing::CorrectLoop,
    // src/LoopClosing.cc:568) ----
    // The flat problem of orbp_optimize_essential_graph (include/orbp.h) and the objects its rows stand for.
    template <class KeyFrameT, class MapPointT>
    struct EgProblem {
        std::vector<KeyFrameT *> kfs;                       // the non-bad vpKFs by mnId ascending (g2o's hessianIndex order): the vertices
        std::vector<MapPointT *> points;                    // the non-bad vpMPs
        std::vector<double> Scw, Snc;
        std::vector<int32_t> edgeI, edgeJ, ref;
        std::vector<uint8_t> edgeCorrected;
        std::vector<float> xw, TcwOut;
        int32_t fixed = -1;
        bool fixScale = false;
        orbp_eg_stats stats{};
        orbp_eg_problem flat() const
        {
            return {(int32_t)kfs.size(), Scw.data(), Snc.data(), fixed, fixScale ? 1 : 0, (int32_t)(edgeI.size() - 1), edgeI.data(), edgeJ.data(),
                    edgeCorrected.data(), (int32_t)points.size(), ref.data()};
        }
    };
    // The walk of :797-983 and :1013-1029.  Sim3 values are read through operator[] only.  Two deviations (include/orbp.h): a bad key
    // frame gets no vertex and every edge or point that would touch a missing vertex is skipped (the reference dereferences a null
    // vertex there; GetAllKeyFrames returns no bad key frame in practice), and a point whose reference has no vertex gets ref = -1.
    template <class MapT, class KeyFrameT, class MapPointT, class PoseMapT, class ConnT>
    static void GatherEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const PoseMapT &NonCorrectedSim3,
                                     const PoseMapT &CorrectedSim3, const ConnT &LoopConnections, const bool bFixScale,
                                     EgProblem<KeyFrameT, MapPointT> &P)
    {
        P = EgProblem<KeyFrameT, MapPointT>();
        P.fixScale = bFixScale;
        const std::vector<KeyFrameT *> vpKFs = pMap->GetAllKeyFrames();
        const std::vector<MapPointT *> vpMPs = pMap->GetAllMapPoints();
        const int minFeat = 100;
        std::map<unsigned long, KeyFrameT *> byId;          // :809-844
        for (size_t i = 0; i < vpKFs.size(); i++)
            if (!vpKFs[i]->isBad()) byId[vpKFs[i]->mnId] = vpKFs[i];
        std::map<unsigned long, int32_t> index;             // optimizer.vertex(mnId)
        for (auto it = byId.begin(); it != byId.end(); it++) {
            KeyFrameT *pKF = it->second;
            index[it->first] = (int32_t)P.kfs.size();
            if (pKF == pLoopKF) P.fixed = (int32_t)P.kfs.size();
            P.kfs.push_back(pKF);
            double S[8];
            const auto itc = CorrectedSim3.find(pKF);
            if (itc != CorrectedSim3.end()) {
                for (int k = 0; k < 8; k++) S[k] = itc->second[k];
            } else {
                const auto R = pKF->GetRotation(), t = pKF->GetTranslation();
                float Rf[9], tf[3];
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) Rf[3 * r + c] = R.template at<float>(r, c);
                    tf[r] = t.template at<float>(r);
                }
                (void)orbp_sim3_from_rts(Rf, tf, 1.0f, S);
            }
            P.Scw.insert(P.Scw.end(), S, S + 8);
            const auto itn = NonCorrectedSim3.find(pKF);
            if (itn != NonCorrectedSim3.end())
                for (int k = 0; k < 8; k++) S[k] = itn->second[k];
            P.Snc.insert(P.Snc.end(), S, S + 8);
        }
        const auto vertex = [&index](KeyFrameT *pKF) {
            const auto it = index.find(pKF->mnId);
            return it == index.end() || pKF->isBad() ? (int32_t)-1 : it->second;
        };
        const auto add = [&P](int32_t i, int32_t j, uint8_t corrected) {
            P.edgeI.push_back(i); P.edgeJ.push_back(j); P.edgeCorrected.push_back(corrected);
        };
        std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
        for (auto mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {       // :852-880
            KeyFrameT *pKF = mit->first;
            const long unsigned int nIDi = pKF->mnId;
            for (auto sit = mit->second.begin(), send = mit->second.end(); sit != send; sit++) {
                const long unsigned int nIDj = (*sit)->mnId;
                if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
                const int32_t vi = vertex(pKF), vj = vertex(*sit);
                if (vi < 0 || vj < 0 || vi == vj) continue;
                add(vi, vj, 1);
                sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
            }
        }
        for (size_t i = 0; i < vpKFs.size(); i++) {         // :883-983
            KeyFrameT *pKF = vpKFs[i];
            const int32_t vi = vertex(pKF);
            if (vi < 0) continue;
            KeyFrameT *pParentKF = pKF->GetParent();
            if (pParentKF && vertex(pParentKF) >= 0 && vertex(pParentKF) != vi) add(vi, vertex(pParentKF), 0);     // :901-923
            const std::set<KeyFrameT *> sLoopEdges = pKF->GetLoopEdges();
            for (auto sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {                    // :926-949
                KeyFrameT *pLKF = *sit;
                if (pLKF->mnId < pKF->mnId && vertex(pLKF) >= 0) add(vi, vertex(pLKF), 0);
            }
            const std::vector<KeyFrameT *> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
            for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {                         // :952-982
                KeyFrameT *pKFn = *vit;
                if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                    if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                        if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                        if (vertex(pKFn) >= 0) add(vi, vertex(pKFn), 0);
                    }
                }
            }
        }
        for (size_t i = 0; i < vpMPs.size(); i++) {         // :1013-1036
            MapPointT *pMP = vpMPs[i];
            if (pMP->isBad()) continue;
            long unsigned int nIDr;
            if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
            else nIDr = pMP->GetReferenceKeyFrame()->mnId;
            const auto it = index.find(nIDr);
            P.points.push_back(pMP);
            P.ref.push_back(it == index.end() ? -1 : it->second);
            const auto X = pMP->GetWorldPos();
            for (int r = 0; r < 3; r++) P.xw.push_back(X.template at<float>(r));
        }
        P.TcwOut.assign(16 * P.kfs.size() + 1, 0.f);
        P.Scw.push_back(0.); P.Snc.push_back(0.); P.xw.push_back(0.f); P.ref.push_back(-1);      // never NULL
        add(0, 0, 0);                                       // flat() leaves this last entry out of n_edges
    }
    // :989-1043 under the map's update lock: SetPose for every vertex, SetWorldPos + UpdateNormalAndDepth for every non-bad point
    template <class MapT, class KeyFrameT, class MapPointT>
    static void ScatterEssentialGraph(const EgProblem<KeyFrameT, MapPointT> &P, MapT *pMap)
    {
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
        for (size_t k = 0; k < P.kfs.size(); k++) {
            auto T = P.kfs[k]->GetPose().clone();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T.template at<float>(r, c) = P.TcwOut[16 * k + 4 * r + c];
            P.kfs[k]->SetPose(T);
        }
        for (size_t p = 0; p < P.points.size(); p++) {
            MapPointT *pMP = P.points[p];
            if (pMP->isBad()) continue;
            auto X = pMP->GetWorldPos().clone();
            for (int r = 0; r < 3; r++) X.template at<float>(r) = P.xw[3 * p + r];
            pMP->SetWorldPos(X);
            pMP->UpdateNormalAndDepth();
        }
    }
    // Through orbm_optimize_essential_graph on the matcher's handle (NULL: the host path, orbp_optimize_essential_graph).  A map
    // beyond ORBM_EG_MAX_KFS key frames falls back to the host path, which has no cap; *err then holds the GPU call's reason.
    // Returns 0 or the ORBX status; on failure nothing is changed and *err receives the text.  Which path to call at which size:
    // INTEGRATION.md 3r.
    template <class MapT, class KeyFrameT, class PoseMapT, class ConnT>
    static int OptimizeEssentialGraph(orbm_matcher *matcher, MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const PoseMapT &NonCorrectedSim3,
                                      const PoseMapT &CorrectedSim3, const ConnT &LoopConnections, const bool &bFixScale,
                                      std::string *err = nullptr, orbp_eg_stats *stats = nullptr, int nIterations = 20)
    {
        typedef typename std::remove_pointer<typename decltype(pMap->GetAllMapPoints())::value_type>::type MapPointT;
        EgProblem<KeyFrameT, MapPointT> P;
        GatherEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale, P);
        const orbp_eg_problem flat = P.flat();
        int rc = ORBX_E_CAPACITY;
        if (matcher) {
            rc = orbm_optimize_essential_graph(matcher, &flat, nIterations, P.TcwOut.data(), P.xw.data(), nullptr, &P.stats);
            if (rc < 0 && err) *err = orbm_last_error();
        }
        if (rc == ORBX_E_CAPACITY) {
            rc = orbp_optimize_essential_graph(&flat, nIterations, P.TcwOut.data(), P.xw.data(), nullptr, &P.stats);
            if (rc < 0 && err) *err = orbp_last_error();
        }
        if (rc < 0) return rc;
        if (stats) *stats = P.stats;
        ScatterEssentialGraph(P, pMap);
        return rc;
    }
    // The reference's signature (include/Optimizer.h:47-51), so src/LoopClosing.cc:568 compiles unchanged; on the host.
    template <class MapT, class KeyFrameT, class PoseMapT, class ConnT>
    static void OptimizeEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const PoseMapT &NonCorrectedSim3,
                                       const PoseMapT &CorrectedSim3, const ConnT &LoopConnections, const bool &bFixScale)
    {
        (void)OptimizeEssentialGraph(static_cast<orbm_matcher *>(nullptr), pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
                                     bFixScale);
    }

private:
    // R*X+t as one cv::gemm evaluates it: three float products summed in float, the translation added in double (Sim3Solver.h)
    template <class MatT>
    static void sim3_to_camera(const MatT &R, const MatT &t, const MatT &X, std::vector<float> &out)
    {
        const float x = X.template at<float>(0), y = X.template at<float>(1), z = X.template at<float>(2);
        for (int r = 0; r < 3; r++) {
            const float t0 = R.template at<float>(r, 0) * x + R.template at<float>(r, 1) * y + R.template at<float>(r, 2) * z;
            out.push_back((float)((double)t0 + (double)t.template at<float>(r)));
        }
    }
};

}  // namespace ORB_SLAM2
