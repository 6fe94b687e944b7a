// Initializer.h -- ORB_SLAM2::Initializer with the reference's interface (include/Initializer.h:32-40) over include/orbp.h, the
// 2 * mMaxIterations hypotheses of FindHomography / FindFundamental in one GPU call and the 4 or 8 CheckRT passes in another
// (include/orbm.h orbm_init_hypotheses, orbm_init_check_rt).
//
// Same constructor (const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200) and the same
// Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D,
// vector<bool> &vbTriangulated), so src/Tracking.cc:589 and :623 compile unchanged.  Of a frame it reads mK and mvKeysUn only
// (both are templates on the frame type for that reason: any class with these two members does).
//
// Initialize runs: the draws (orbp_init_draw), one orbm_init_hypotheses on a pooled matcher handle (orbm_pool.h), the two walks on
// the host, the candidate motions, one orbm_init_check_rt, the acceptance rules (orbp_init_initialize).  Where no handle is to be
// had, a GPU call fails or SetUseGpu(false) was called, the host evaluates the same hypotheses with the same text
// (csrc/orbp_init_body.h): every output byte is the same, and LastError() says what happened.  The default of SetUseGpu is
// kDefaultUseGpu below; INTEGRATION.md 3n has the measurement behind it.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#else
#include "orbx_cv_compat.h"
#endif
#include "../../include/orbm.h"
#include "../../include/orbp.h"
#include "orbm_pool.h"

namespace ORB_SLAM2 {

class Initializer {
public:
    static constexpr bool kDefaultUseGpu = true;

    // Fix the reference frame (src/Initializer.cc:33-42)
    template <class FrameT>
    Initializer(const FrameT &ReferenceFrame, float sigma = 1.0, int iterations = 200)
    {
        const cv::Mat &K = ReferenceFrame.mK;
        std::vector<float> keys1;
        pack_keys(ReferenceFrame.mvKeysUn, keys1);
        mN1 = (int)ReferenceFrame.mvKeysUn.size();
        if (K.empty() || orbp_init_create(&s_, keys1.data(), mN1, K.at<float>(0, 0), K.at<float>(1, 1),
                                          K.at<float>(0, 2), K.at<float>(1, 2), sigma, iterations) < 0) {
            err_ = K.empty() ? "Initializer: the reference frame has no mK" : orbp_last_error();
            s_ = nullptr;
        }
    }
    ~Initializer() { orbp_init_destroy(s_); }
    Initializer(const Initializer &) = delete;
    Initializer &operator=(const Initializer &) = delete;

    // a per-object uniform source (fn(ctx) in [0, randMax]); without one the draws come from libc rand() after SeedRandOnce(0)
    void SetRand(int (*fn)(void *), void *ctx, int randMax) { if (s_) orbp_init_set_rand(s_, fn, ctx, randMax); }
    void SetUseGpu(bool on) { useGpu_ = on; }
    bool Valid() const { return s_ != nullptr; }
    const std::string &LastError() const { return err_; }
    bool LastUsedGpu() const { return usedGpu_; }       // the last Initialize took both GPU calls (or needed none of the second)

    // Computes in parallel a fundamental matrix and a homography, selects a model and tries to recover the motion and the
    // structure from motion (src/Initializer.cc:44-121)
    template <class FrameT>
    bool Initialize(const FrameT &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                    std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated)
    {
        usedGpu_ = false;
        err_.clear();
        if (!s_) { err_ = "Initializer: no solver"; return false; }
        if ((int)vMatches12.size() != mN1) { err_ = "Initializer: vMatches12 does not have one entry per reference key"; return false; }
        std::vector<float> keys2;
        pack_keys(CurrentFrame.mvKeysUn, keys2);
        std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
        const int N = orbp_init_set_current(s_, keys2.data(), (int)CurrentFrame.mvKeysUn.size(), m12.data());
        if (N < 0 || orbp_init_draw(s_, nullptr) < 0) { err_ = orbp_last_error(); return false; }      // fewer than 8 matches: refused
        int model = -1;
        if (useGpu_) usedGpu_ = evaluate_on_gpu(N, model);
        std::vector<float> p3d(3 * (size_t)mN1 + 3);
        std::vector<uint8_t> tri((size_t)mN1 + 1);
        float R[9], t[3];
        const int ok = orbp_init_initialize(s_, R, t, p3d.data(), tri.data());
        if (ok < 0) err_ = orbp_last_error();
        if (ok <= 0) {
            if (model_of_last_plan() == 1) { R21 = cv::Mat(); t21 = cv::Mat(); }                       // ReconstructF :501-502
            return false;
        }
        R21 = cv::Mat(3, 3, CV_32F);
        t21 = cv::Mat(3, 1, CV_32F);
        for (int i = 0; i < 9; i++) R21.at<float>(i / 3, i % 3) = R[i];
        for (int i = 0; i < 3; i++) t21.at<float>(i) = t[i];
        vP3D.resize(mN1);
        vbTriangulated.assign(mN1, false);
        for (int i = 0; i < mN1; i++) {
            vP3D[i] = cv::Point3f(p3d[3 * (size_t)i], p3d[3 * (size_t)i + 1], p3d[3 * (size_t)i + 2]);
            vbTriangulated[i] = tri[i] != 0;
        }
        return true;
    }

private:
    static void pack_keys(const std::vector<cv::KeyPoint> &keys, std::vector<float> &out)
    {
        out.resize(2 * keys.size() + 2);
        for (size_t i = 0; i < keys.size(); i++) { out[2 * i] = keys[i].pt.x; out[2 * i + 1] = keys[i].pt.y; }
    }
    int model_of_last_plan()
    {
        int model = -1, n = 0;
        float M[9], Rt[12 * ORBM_INIT_MAX_MOTIONS];
        int N = 0;
        orbp_init_get_sizes(s_, nullptr, nullptr, &N, nullptr, nullptr);
        std::vector<uint8_t> inl((size_t)N + 1);
        if (orbp_init_plan_check_rt(s_, &model, M, inl.data(), Rt, &n) < 0) return -1;
        return model;
    }
    // both GPU calls of one Initialize; false (and err_) where the host has to evaluate instead
    bool evaluate_on_gpu(int N, int &model)
    {
        orbm_detail::Lease lease;
        if (!lease.ready(&err_)) return false;
        int its = 0;
        orbp_init_get_sizes(s_, nullptr, nullptr, nullptr, &its, nullptr);
        const size_t n = (size_t)N, H = 2 * (size_t)its, W = (n + 31) / 32;
        std::vector<float> uv(4 * n + 4), pn(4 * n + 4), scoreM(10 * H + 1);
        std::vector<int32_t> sets(8 * H + 8), models(H + 1), counts(H + 1);
        std::vector<uint32_t> masks(W * H + 1);
        float params[24];
        orbp_init_get_problem(s_, uv.data(), pn.data(), params, sets.data(), nullptr, nullptr);
        for (size_t k = 0; k < (size_t)its; k++) {                 // the H of every set, then the F (orbp_init_attach_results)
            memcpy(&sets[8 * ((size_t)its + k)], &sets[8 * k], 8 * sizeof(int32_t));
            models[k] = 0; models[(size_t)its + k] = 1;
        }
        orbm_init_params par;
        memcpy(&par, params, sizeof par);
        const int32_t off[2] = {0, N}, hypOff[2] = {0, (int32_t)H};
        const int64_t maskOff[2] = {0, (int64_t)(W * H)};
        if (orbm_init_hypotheses(lease.h.m, 1, off, uv.data(), pn.data(), &par, hypOff, sets.data(), models.data(), maskOff, scoreM.data(),
                                 counts.data(), masks.data()) != ORBX_OK) {
            err_ = orbm_last_error();
            return false;
        }
        if (orbp_init_attach_results(s_, (int)H, scoreM.data(), counts.data(), masks.data()) < 0) { err_ = orbp_last_error(); return false; }
        float M[9], Rt[12 * ORBM_INIT_MAX_MOTIONS];
        std::vector<uint8_t> inl(n + 1);
        int nMotions = 0;
        if (orbp_init_plan_check_rt(s_, &model, M, inl.data(), Rt, &nMotions) < 0) { err_ = orbp_last_error(); return false; }
        if (nMotions == 0) return true;                            // Initialize returns false before any CheckRT
        const size_t pairs = n * (size_t)nMotions;
        std::vector<uint8_t> status(pairs + 1);
        std::vector<float> cosp(pairs + 1), p3d(3 * pairs + 3);
        if (orbm_init_check_rt(lease.h.m, N, uv.data(), inl.data(), params + 19, params[23], nMotions, Rt, status.data(), cosp.data(),
                               p3d.data()) != ORBX_OK) {
            err_ = orbm_last_error();
            return false;
        }
        if (orbp_init_attach_check_rt(s_, nMotions, Rt, inl.data(), status.data(), cosp.data(), p3d.data()) < 0) { err_ = orbp_last_error(); return false; }
        return true;
    }
    orbp_init *s_ = nullptr;
    int mN1 = 0;
    bool useGpu_ = kDefaultUseGpu, usedGpu_ = false;
    std::string err_;
};

}  // namespace ORB_SLAM2
