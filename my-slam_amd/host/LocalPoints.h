// LocalPoints.h -- the second half of Tracking::SearchLocalPoints (src/Tracking.cc:1174-1199 of WChen09/My-SLAM) in ONE GPU call
// (orbm_search_local_points, include/orbm.h): Frame::isInFrustum for every local MapPoint and, when one is in view,
// ORBmatcher::SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th).
//
//     int ORB_SLAM2::SearchLocalPoints(Frame &F, const std::vector<MapPoint*> &vpLocalMapPoints, float th, float nnratio,
//                                      std::string *err);
//
// F is mCurrentFrame after the first loop of the function (:1153-1169), th and nnratio what :1191-1197 choose.  The call gathers
// under the reference's getters, makes one library call and replays on the objects what the two loops write:
//   every MapPoint the loop reaches (:1177-1180 passed)   mbTrackInView (src/Frame.cc:271, :317)
//   every MapPoint in view                                mTrackProjX, mTrackProjXR, mTrackProjY, mnTrackScaleLevel, mTrackViewCos
//                                                         (src/Frame.cc:318-322), IncreaseVisible() (:1184)
//   every match                                           F.mvpMapPoints[idx] = pMP (src/ORBmatcher.cc:120)
// Returns the number of matches (what SearchByProjection returns; 0 when nothing is in view), or -1 when the GPU call failed
// (text in *err); no object has been written then.
// Reads: F.mTcw (mRcw and mtcw are its blocks, src/Frame.cc:263-265), F.GetCameraCenter(), fx, fy, cx, cy, mbf, mnMinX .. mnMaxY,
// mfLogScaleFactor, mnScaleLevels, mvScaleFactors, mvKeysUn, mDescriptors, mvuRight, mvpMapPoints[i]->Observations(), mnId;
// pMP->mnLastFrameSeen, isBad(), GetWorldPos(), GetNormal(), GetDescriptor(), Observations() and the one accessor the reference's
// MapPoint lacks: the raw mfMaxDistance / mfMinDistance, which MapPoint::PredictScale and the two
// *DistanceInvariance getters read under mMutexPos --
//     void MapPoint::GetDistanceRange(float &mfMax, float &mfMin) { unique_lock<mutex> lock(mMutexPos); mfMax = mfMaxDistance; mfMin = mfMinDistance; }
// Templated like NewMapPoints.h, on the tree's own "Frame.h" / "MapPoint.h"; the GPU handle is the pooled thread-local one.
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
#include "orbm_pool.h"

#include "MapPoint.h"
#include "Frame.h"

namespace ORB_SLAM2 {
namespace orbm_detail {
template <class FrameT> bool FillFrameView(FrameT &F, orbm_frame_view &v, std::string *err)
{
    const cv::Mat Ow = F.GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) v.Rcw[3 * r + k] = F.mTcw.template at<float>(r, k);
        v.tcw[r] = F.mTcw.template at<float>(r, 3);
        v.Ow[r] = Ow.template at<float>(r);
    }
    v.fx = F.fx; v.fy = F.fy; v.cx = F.cx; v.cy = F.cy; v.mbf = F.mbf;
    v.bounds[0] = (float)F.mnMinX; v.bounds[1] = (float)F.mnMaxX; v.bounds[2] = (float)F.mnMinY; v.bounds[3] = (float)F.mnMaxY;
    v.log_scale_factor = F.mfLogScaleFactor;
    const size_t nl = F.mvScaleFactors.size();
    if (nl < 1 || nl > ORBX_MAX_LEVELS || (int)nl != F.mnScaleLevels) {
        if (err) *err = "frame with " + std::to_string(nl) + " scale factors and " + std::to_string(F.mnScaleLevels) + " levels";
        return false;
    }
    v.nlevels = (int32_t)nl;
    for (size_t l = 0; l < ORBX_MAX_LEVELS; l++) v.scale_factors[l] = l < nl ? F.mvScaleFactors[l] : 0.f;
    return true;
}
// Frame::AssignFeaturesToGrid of the searched frame, on the GPU; skipped while the pooled handle still holds this frame's grid
template <class FrameT> bool EnsureFrameGrid(PooledHandle &h, const FrameT &F, std::string *err)
{
    const int n = (int)F.mvKeysUn.size();
    if (h.gridKind == 0 && h.gridFrame == (unsigned long)F.mnId && h.gridKeys == (const void *)F.mvKeysUn.data() && h.gridN == n &&
        orbm_grid_count(h.m) == n) return true;
    h.gridN = -1;
    if (orbm_grid_build(h.m, reinterpret_cast<const orbx_keypoint *>(F.mvKeysUn.data()), n, (float)F.mnMinX, (float)F.mnMaxX, (float)F.mnMinY,
                        (float)F.mnMaxY) != ORBX_OK) {
        if (err) *err = orbm_last_error();
        return false;
    }
    h.gridKind = 0; h.gridFrame = (unsigned long)F.mnId; h.gridKeys = (const void *)F.mvKeysUn.data(); h.gridN = n;
    return true;
}
}  // namespace orbm_detail

template <class FrameT, class MapPointT>
int SearchLocalPoints(FrameT &F, const std::vector<MapPointT *> &vpLocalMapPoints, float th, float nnratio, std::string *err = nullptr)
{
    const int n = (int)vpLocalMapPoints.size(), nc = (int)F.mvKeysUn.size();
    if (n == 0) return 0;
    orbm_detail::Lease lease;
    if (!lease.ready(err)) return -1;
    orbm_detail::Scratch &S = *lease.h.s;
    orbm_frame_view view;
    if (!orbm_detail::FillFrameView(F, view, err)) return -1;
    if (nc > 0 && !orbm_detail::EnsureFrameGrid(lease.h, F, err)) return -1;
    S.u8_.assign(n, 0); S.f0_.assign((size_t)n * 3, 0.f); S.f1_.assign((size_t)n * 3, 0.f); S.f2_.assign(n, 0.f); S.f3_.assign(n, 0.f);
    S.i1_.assign(n, 0); S.desc_.assign((size_t)n * 32, 0);
    for (int i = 0; i < n; i++) {
        MapPointT *pMP = vpLocalMapPoints[i];
        if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) { S.u8_[i] = 1; continue; }            // :1177-1180
        const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
        for (int k = 0; k < 3; k++) { S.f0_[(size_t)3 * i + k] = P.template at<float>(k); S.f1_[(size_t)3 * i + k] = Pn.template at<float>(k); }
        pMP->GetDistanceRange(S.f2_[i], S.f3_[i]);
        S.i1_[i] = pMP->Observations();
        const cv::Mat d = pMP->GetDescriptor();
        memcpy(&S.desc_[(size_t)i * 32], d.template ptr<unsigned char>(), 32);
    }
    S.obs_.assign(nc, -1);                          // -1 = NULL slot, else the point's Observations() (src/ORBmatcher.cc:85-87)
    for (int i = 0; i < nc; i++)
        if (F.mvpMapPoints[i]) S.obs_[i] = F.mvpMapPoints[i]->Observations();
    S.match_.assign(nc, -1);
    S.v8_.assign(n, 0); S.g0_.assign(n, 0.f); S.g1_.assign(n, 0.f); S.g2_.assign(n, 0.f); S.g3_.assign(n, 0.f); S.i0_.assign(n, 0);
    const bool stereo = (int)F.mvuRight.size() == nc && nc > 0 && F.mbf > 0;
    int nToMatch = 0, nmatches = 0;
    if (orbm_search_local_points(lease.h.m, &view, n, S.u8_.data(), S.f0_.data(), S.f1_.data(), S.f2_.data(), S.f3_.data(), 0.5f, S.desc_.data(),
                                 S.i1_.data(), reinterpret_cast<const orbx_keypoint *>(F.mvKeysUn.data()),
                                 nc > 0 ? F.mDescriptors.template ptr<unsigned char>() : nullptr, stereo ? F.mvuRight.data() : nullptr, nc, th,
                                 nnratio, S.v8_.data(), S.g0_.data(), S.g1_.data(), S.g2_.data(), S.i0_.data(), S.g3_.data(), &nToMatch,
                                 S.obs_.data(), S.match_.data(), &nmatches) != ORBX_OK) {
        if (err) *err = orbm_last_error();
        return -1;
    }
    for (int i = 0; i < n; i++) {
        if (S.v8_[i] == ORBM_FRUSTUM_SKIPPED) continue;
        MapPointT *pMP = vpLocalMapPoints[i];
        pMP->mbTrackInView = S.v8_[i] == ORBM_FRUSTUM_IN_VIEW;                                      // src/Frame.cc:271, :317
        if (!pMP->mbTrackInView) continue;
        pMP->mTrackProjX = S.g0_[i]; pMP->mTrackProjXR = S.g2_[i]; pMP->mTrackProjY = S.g1_[i];     // :318-320
        pMP->mnTrackScaleLevel = S.i0_[i]; pMP->mTrackViewCos = S.g3_[i];                           // :321-322
        pMP->IncreaseVisible();                                                                     // src/Tracking.cc:1184
    }
    for (int i2 = 0; i2 < nc; i2++)
        if (S.match_[i2] >= 0) F.mvpMapPoints[i2] = vpLocalMapPoints[S.match_[i2]];                 // src/ORBmatcher.cc:120
    return nmatches;
}

}  // namespace ORB_SLAM2
