// PnPsolver.h / Optimizer -- the reference's pose-solver call shapes over include/orbp.h (host code inside liborbx.so).
// Reference: include/PnPsolver.h:66-78 (PnPsolver(const Frame&, const vector<MapPoint*>&), SetRansacParameters, find,
// iterate) and include/Optimizer.h (static int PoseOptimization(Frame*)).  Frame / MapPoint belong to the reference's
// object graph, so the constructor here takes what the reference constructor reads out of them
// (src/PnPsolver.cc:78-106); INTEGRATION.md 3d shows the five-line gather that keeps the original signature.
// Poses are row-major 4x4 float (the layout of the reference's CV_32F Tcw); an empty optional stands for the empty
// cv::Mat the reference returns.  PnPsolver::EvaluateAll is the one addition to the reference's interface: the EPnP
// hypotheses of all Relocalization candidates in one GPU call (orbm_pnp_hypotheses), replayed by iterate.
#pragma once
#include <array>
#include <cstdint>
#include <optional>
#include <string>
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
};

}  // namespace ORB_SLAM2
