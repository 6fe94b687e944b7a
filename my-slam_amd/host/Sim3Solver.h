// Sim3Solver.h -- ORB_SLAM2::Sim3Solver with the reference's interface (include/Sim3Solver.h:36-58) over include/orbp.h, and the
// batch step that evaluates the hypotheses of all loop candidates in one GPU call (include/orbm.h orbm_sim3_hypotheses).
//
// Same constructor (KeyFrame*, KeyFrame*, const vector<MapPoint*>&, bool bFixScale), SetRansacParameters, find, iterate and
// GetEstimatedRotation / Translation / Scale, so src/LoopClosing.cc:275-276, :301-302 and :321-323 compile unchanged.  The
// constructor does what src/Sim3Solver.cc:43-109 does: it skips NULL / bad MapPoints and those without an index in their key
// frame, moves the points into the two camera frames (Rcw*Xw+tcw as cv::gemm evaluates it), and keeps mvnIndices1, through which
// iterate() maps the inlier flags back to vpMatched12's indices.  The calibration is read from pKF->fx, fy, cx, cy (the entries
// of the mK the reference reads).
//
// LoopClosing::ComputeSim3 adds ONE line after its first loop:
//     Sim3Solver::EvaluateAll(vpSim3Solvers, matcher);
// which draws every solver's remaining triples, evaluates all of them in one launch and attaches the results; the while loop of
// :287-343 then runs as written and every iterate(5) is a replay.  A solver that was never passed to EvaluateAll (or whose GPU
// call failed) evaluates on the host, hypothesis by hypothesis, with the same bytes.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#else
#include "orbx_cv_compat.h"
#endif
#include "../../include/orbm.h"
#include "../../include/orbp.h"
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true)
    {
        std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation();
        const cv::Mat Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
        std::vector<float> x1, x2, s1, s2;
        for (int i1 = 0; i1 < mN1; i1++) {                  // src/Sim3Solver.cc:62-103
            if (!vpMatched12[i1]) continue;
            MapPoint *pMP1 = vpKeyFrameMP1[i1];
            MapPoint *pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
            const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            s1.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]);
            s2.push_back(pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave]);
            mvnIndices1.push_back((size_t)i1);
            to_camera(Rcw1, tcw1, pMP1->GetWorldPos(), x1);
            to_camera(Rcw2, tcw2, pMP2->GetWorldPos(), x2);
        }
        const float K1[4] = {pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy}, K2[4] = {pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy};
        if (orbp_sim3_create(&s_, (int)mvnIndices1.size(), x1.data(), x2.data(), s1.data(), s2.data(), K1, K2, bFixScale ? 1 : 0) < 0) {
            err_ = orbp_last_error();
            s_ = nullptr;
        }
    }
    ~Sim3Solver() { orbp_sim3_destroy(s_); }
    Sim3Solver(const Sim3Solver &) = delete;
    Sim3Solver &operator=(const Sim3Solver &) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        if (s_ && orbp_sim3_set_ransac_parameters(s_, probability, minInliers, maxIterations) < 0) err_ = orbp_last_error();
    }
    // a per-solver uniform source (fn(ctx) in [0, randMax]); without one the draws come from libc rand() as in the reference
    void SetRand(int (*fn)(void *), void *ctx, int randMax) { if (s_) orbp_sim3_set_rand(s_, fn, ctx, randMax); }

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        int maxIts = 0;
        if (s_) orbp_sim3_get_ransac_state(s_, nullptr, &maxIts, nullptr, nullptr, nullptr);
        return iterate(maxIts, bFlag, vbInliers12, nInliers);
    }

    // vbInliers is indexed like vpMatched12 (src/Sim3Solver.cc:143, :195-197); an empty cv::Mat when no pose is returned
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (!s_) { bNoMore = true; return cv::Mat(); }
        std::vector<uint8_t> inl(mvnIndices1.size() + 1);
        float T[16];
        int noMore = 0;
        const int got = orbp_sim3_iterate(s_, nIterations, &noMore, inl.data(), &nInliers, T);
        bNoMore = noMore != 0;
        if (got <= 0) { if (got < 0) err_ = orbp_last_error(); return cv::Mat(); }
        for (size_t i = 0; i < mvnIndices1.size(); i++)
            if (inl[i]) vbInliers[mvnIndices1[i]] = true;
        cv::Mat T12(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) T12.at<float>(r, c) = T[4 * r + c];
        return T12;
    }

    cv::Mat GetEstimatedRotation()
    {
        float R[9], t[3], s;
        if (!s_ || orbp_sim3_get_estimated(s_, R, t, &s) <= 0) return cv::Mat();
        cv::Mat m(3, 3, CV_32F);
        for (int i = 0; i < 9; i++) m.at<float>(i / 3, i % 3) = R[i];
        return m;
    }
    cv::Mat GetEstimatedTranslation()
    {
        float R[9], t[3], s;
        if (!s_ || orbp_sim3_get_estimated(s_, R, t, &s) <= 0) return cv::Mat();
        cv::Mat m(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) m.at<float>(i) = t[i];
        return m;
    }
    float GetEstimatedScale()
    {
        float R[9], t[3], s = 0.f;
        if (s_) orbp_sim3_get_estimated(s_, R, t, &s);
        return s;
    }

    // The batch step of LoopClosing::ComputeSim3: every non-NULL solver's remaining triples are drawn (solver by solver), all of
    // them are evaluated by ONE orbm_sim3_hypotheses call on the matcher's handle, and the results are attached.  Returns the
    // ORBX status; on failure (*err receives the text) the solvers keep their drawn triples and evaluate them on the host.
    static int EvaluateAll(const std::vector<Sim3Solver *> &vpSolvers, ORBmatcher &matcher, std::string *err = nullptr)
    {
        std::vector<Sim3Solver *> live;
        std::vector<int32_t> off(1, 0), hypOff(1, 0), triples;
        std::vector<int64_t> maskOff(1, 0);
        std::vector<float> x1, x2, e1, e2;
        std::vector<orbm_sim3_camera> cams;
        for (Sim3Solver *p : vpSolvers) {
            if (!p || !p->s_) continue;
            orbp_sim3 *s = p->s_;
            int maxIts = 0;
            orbp_sim3_get_ransac_state(s, nullptr, &maxIts, nullptr, nullptr, nullptr);
            orbp_sim3_draw(s, maxIts, nullptr);
            const int h = orbp_sim3_queued(s, nullptr), n = (int)p->mvnIndices1.size();
            const size_t t0 = triples.size(), c0 = e1.size();
            triples.resize(t0 + 3 * (size_t)h);
            orbp_sim3_queued(s, triples.data() + t0);
            x1.resize(3 * (c0 + n)); x2.resize(3 * (c0 + n)); e1.resize(c0 + n); e2.resize(c0 + n);
            orbm_sim3_camera &cam = cams.emplace_back();
            orbp_sim3_get_problem(s, x1.data() + 3 * c0, x2.data() + 3 * c0, e1.data() + c0, e2.data() + c0, cam.K1, cam.K2, &cam.fix_scale);
            off.push_back(off.back() + n);
            hypOff.push_back(hypOff.back() + h);
            maskOff.push_back(maskOff.back() + (int64_t)h * ((n + 31) / 32));
            live.push_back(p);
        }
        const size_t H = (size_t)hypOff.back();
        std::vector<int32_t> counts(H + 1);
        std::vector<float> sRt(13 * H + 1);
        std::vector<uint32_t> masks((size_t)maskOff.back() + 1);
        const int rc = matcher.Sim3Hypotheses((int)live.size(), off.data(), x1.data(), x2.data(), e1.data(), e2.data(), cams.data(), hypOff.data(),
                                              triples.data(), maskOff.data(), counts.data(), sRt.data(), masks.data());
        if (rc != ORBX_OK) { if (err) *err = matcher.LastError(); return rc; }
        for (size_t k = 0; k < live.size(); k++)
            if (orbp_sim3_attach_results(live[k]->s_, hypOff[k + 1] - hypOff[k], counts.data() + hypOff[k], sRt.data() + 13 * (size_t)hypOff[k],
                                         masks.data() + maskOff[k]) < 0) {
                if (err) *err = orbp_last_error();
                return ORBX_E_INVALID;
            }
        return ORBX_OK;
    }

    bool Valid() const { return s_ != nullptr; }
    const std::string &LastError() const { return err_; }
    const std::vector<size_t> &Indices1() const { return mvnIndices1; }      // mvnIndices1: correspondence -> index in vpMatched12

private:
    // Rcw*Xw+tcw: one cv::gemm, three float products summed in float, the translation added in double (csrc/orbm_internal.h gemm3)
    static void to_camera(const cv::Mat &R, const cv::Mat &t, const cv::Mat &X, std::vector<float> &out)
    {
        const float x = X.at<float>(0), y = X.at<float>(1), z = X.at<float>(2);
        for (int r = 0; r < 3; r++) {
            const float t0 = R.at<float>(r, 0) * x + R.at<float>(r, 1) * y + R.at<float>(r, 2) * z;
            out.push_back((float)((double)t0 + (double)t.at<float>(r)));
        }
    }
    orbp_sim3 *s_ = nullptr;
    int mN1 = 0;
    std::vector<size_t> mvnIndices1;
    std::string err_;
};

}  // namespace ORB_SLAM2
