// MapPointDescriptors.h -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307 of WChen09/My-SLAM) for a whole
// list of MapPoints in ONE GPU call (orbm_distinctive_descriptors, include/orbm.h).
//
//     int ORB_SLAM2::ComputeDistinctiveDescriptors(const std::vector<MapPoint*> &vpMPs);
//
// The reference calls the method once per MapPoint inside loops over all MapPoints of a key frame (src/LocalMapping.cc:141-163,
// :444, :519-532, src/LoopClosing.cc:533, src/Tracking.cc:541, 677, 1124); the loop keeps everything else and the descriptor
// calls become one call after it.  Per MapPoint the function does what the reference's body does:
//   reads:  pMP->isBad() (:251), pMP->GetObservations() (the copy :253 takes, under the point's own lock),
//           pKF->isBad() (:265), pKF->mDescriptors.row(idx) (:266) in the map's iteration order
//   writes: pMP->SetDescriptor(row) -- the reference has no setter for the protected mDescriptor, so the integrator adds
//               void MapPoint::SetDescriptor(const cv::Mat &d) { unique_lock<mutex> lock(mMutexFeatures); mDescriptor = d.clone(); }
//           which is :303-306.  NULL and bad points, points without observations and points whose key frames are all bad keep
//           their descriptor (:251, :256, :269).
// Returns the number of MapPoints whose descriptor was set, or -1 when the GPU call failed (text in *err); no descriptor is
// touched then.  It is its own header because it needs members (GetObservations, SetDescriptor, KeyFrame::isBad) that the
// matcher adapter does not; like ORBmatcher.h it includes the tree's own "MapPoint.h" and "KeyFrame.h".  The GPU handle is the
// pooled thread-local one of ORBmatcher.h (orbm_pool.h).
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
#include "KeyFrame.h"

namespace ORB_SLAM2 {

template <class MapPointT> int ComputeDistinctiveDescriptors(const std::vector<MapPointT *> &vpMPs, std::string *err = nullptr)
{
    orbm_detail::Lease lease;
    if (!lease.ready(err)) return -1;
    orbm_detail::Scratch &S = *lease.h.s;
    std::vector<MapPointT *> pts;                  // the points that reach :272, in list order
    S.i0_.assign(1, 0); S.desc_.clear();
    for (MapPointT *pMP : vpMPs) {
        if (!pMP || pMP->isBad()) continue;                                     // :251
        const auto observations = pMP->GetObservations();                       // :253
        if (observations.empty()) continue;                                     // :256
        const size_t before = S.desc_.size();
        for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {     // :261
            auto *pKF = mit->first;
            if (pKF->isBad()) continue;                                         // :265
            S.desc_.resize(S.desc_.size() + 32);
            memcpy(&S.desc_[S.desc_.size() - 32], pKF->mDescriptors.template ptr<unsigned char>((int)mit->second), 32);   // :266
        }
        if (S.desc_.size() == before) continue;                                 // :269
        S.i0_.push_back((int32_t)(S.desc_.size() / 32));
        pts.push_back(pMP);
    }
    const int n = (int)pts.size();
    if (n == 0) return 0;
    S.i1_.assign(n, -1);
    if (orbm_distinctive_descriptors(lease.h.m, n, S.i0_.data(), S.desc_.data(), S.i1_.data(), nullptr) != ORBX_OK) {
        if (err) *err = orbm_last_error();
        return -1;
    }
    for (int p = 0; p < n; p++) {
        const cv::Mat row(1, 32, CV_8U, &S.desc_[((size_t)S.i0_[p] + S.i1_[p]) * 32]);     // a header over the gathered bytes
        pts[p]->SetDescriptor(row);                                             // :303-306 (clones)
    }
    return n;
}

}  // namespace ORB_SLAM2
