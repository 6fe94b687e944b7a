// NewMapPoints.h -- the per-match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:288-434 of WChen09/My-SLAM) for
// all matches of one neighbour in ONE GPU call (orbm_triangulate_matches, include/orbm.h).
//
//     int ORB_SLAM2::TriangulateMatches(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<std::pair<size_t,size_t> > &vMatchedIndices,
//                                       std::vector<unsigned char> &status, std::vector<cv::Mat> &x3D, std::string *err);
//
// pKF1 is mpCurrentKeyFrame, pKF2 the neighbour, vMatchedIndices what SearchForTriangulation returned (:270).  status[k] names the
// line that decided match k (orbm_tri_status); x3D[k] is the 3x1 CV_32F position of the new MapPoint for the accepted ones
// (status[k] <= ORBM_TRI_STEREO2) and an empty matrix otherwise.  The object-graph work of :436-451 stays with the caller, over the
// accepted matches in match order.  Returns the number of accepted matches, or -1 when the GPU call failed
// (text in *err); status and x3D are empty then.
// Per key frame the function reads what the reference's loop reads, under the same getters:
//   :219-233, :272-284   GetRotation(), GetTranslation(), GetCameraCenter(), fx, fy, cx, cy, invfx, invfy, mfScaleFactor
//   :293-298             mvKeysUn, mvuRight
//   :314-316, :344, :348 mb, mvDepth, and through UnprojectStereo mvKeys (src/KeyFrame.cc:615-631)
//   :365, :382, :392, :428   mvLevelSigma2, mbf, mvScaleFactors
// It is its own header because it needs members (mvDepth, mb, mvKeys, invfx) that the matcher adapter does not; like
// MapPointDescriptors.h it includes the tree's own "KeyFrame.h".  The GPU handle is the pooled thread-local one (orbm_pool.h).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#else
#include "orbx_cv_compat.h"
#endif
#include "../../include/orbm.h"
#include "orbm_pool.h"

#include "KeyFrame.h"

namespace ORB_SLAM2 {
namespace orbm_detail {
template <class KeyFrameT> bool FillCamera(KeyFrameT *pKF, orbm_camera &c, std::string *err)
{
    const cv::Mat Rcw = pKF->GetRotation(), tcw = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) c.Rcw[3 * r + k] = Rcw.template at<float>(r, k);
        c.tcw[r] = tcw.template at<float>(r);
        c.Ow[r] = Ow.template at<float>(r);
    }
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy; c.invfx = pKF->invfx; c.invfy = pKF->invfy;
    c.mb = pKF->mb; c.mbf = pKF->mbf; c.scale_factor = pKF->mfScaleFactor;
    const size_t nl = pKF->mvScaleFactors.size();
    if (nl < 1 || nl > ORBX_MAX_LEVELS || pKF->mvLevelSigma2.size() != nl) {
        if (err) *err = "key frame with " + std::to_string(nl) + " pyramid levels";
        return false;
    }
    c.nlevels = (int32_t)nl;
    for (size_t l = 0; l < ORBX_MAX_LEVELS; l++) {
        c.scale_factors[l] = l < nl ? pKF->mvScaleFactors[l] : 0.f;
        c.level_sigma2[l] = l < nl ? pKF->mvLevelSigma2[l] : 0.f;
    }
    return true;
}
template <class KeyFrameT> void FillFeatures(KeyFrameT *pKF, std::vector<orbx_keypoint> &kp, std::vector<float> &xy, std::vector<float> &ur,
                                             std::vector<float> &depth)
{
    const size_t n = pKF->mvKeysUn.size();
    kp.resize(n); xy.resize(2 * n); ur.resize(n); depth.resize(n);
    for (size_t i = 0; i < n; i++) {
        const cv::KeyPoint &k = pKF->mvKeysUn[i];
        kp[i].x = k.pt.x; kp[i].y = k.pt.y; kp[i].size = k.size; kp[i].angle = k.angle; kp[i].response = k.response;
        kp[i].octave = k.octave; kp[i].class_id = k.class_id;
        xy[2 * i] = pKF->mvKeys[i].pt.x; xy[2 * i + 1] = pKF->mvKeys[i].pt.y;
        ur[i] = pKF->mvuRight[i]; depth[i] = pKF->mvDepth[i];
    }
}
}  // namespace orbm_detail

template <class KeyFrameT>
int TriangulateMatches(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<std::pair<size_t, size_t> > &vMatchedIndices,
                       std::vector<unsigned char> &status, std::vector<cv::Mat> &x3D, std::string *err = nullptr)
{
    status.clear(); x3D.clear();
    const int n = (int)vMatchedIndices.size();
    if (n == 0) return 0;
    orbm_detail::Lease lease;
    if (!lease.ready(err)) return -1;
    orbm_detail::Scratch &S = *lease.h.s;
    orbm_camera cam1, cam2;
    if (!orbm_detail::FillCamera(pKF1, cam1, err) || !orbm_detail::FillCamera(pKF2, cam2, err)) return -1;
    orbm_detail::FillFeatures(pKF1, S.kp_, S.f0_, S.f1_, S.f2_);
    orbm_detail::FillFeatures(pKF2, S.kp2_, S.f3_, S.f4_, S.f5_);
    S.i0_.resize(3 * (size_t)n);
    for (int k = 0; k < n; k++) {
        S.i0_[3 * (size_t)k] = (int32_t)vMatchedIndices[k].first; S.i0_[3 * (size_t)k + 1] = (int32_t)vMatchedIndices[k].second; S.i0_[3 * (size_t)k + 2] = 0;
    }
    const int32_t off2[2] = {0, (int32_t)S.kp2_.size()};
    S.u8_.assign(n, 0); S.g0_.assign(3 * (size_t)n, 0.f);
    if (orbm_triangulate_matches(lease.h.m, &cam1, S.kp_.data(), S.f0_.data(), S.f1_.data(), S.f2_.data(), (int)S.kp_.size(), &cam2, 1, off2,
                                 S.kp2_.data(), S.f3_.data(), S.f4_.data(), S.f5_.data(), S.i0_.data(), n, S.u8_.data(), S.g0_.data()) != ORBX_OK) {
        if (err) *err = orbm_last_error();
        return -1;
    }
    status.assign(S.u8_.begin(), S.u8_.end());
    x3D.resize(n);
    int accepted = 0;
    for (int k = 0; k < n; k++) {
        if (status[k] > ORBM_TRI_STEREO2) continue;
        cv::Mat p(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) p.template at<float>(r) = S.g0_[3 * (size_t)k + r];
        x3D[k] = p;
        accepted++;
    }
    return accepted;
}

}  // namespace ORB_SLAM2
