// MapPoint.h -- repo-authored minimal MapPoint for tests/cxx/fuse_views_callsites.cc (names and signatures as in the reference's
// include/MapPoint.h, bodies written here).  Beyond tests/cxx/slam_shims/MapPoint.h it has what the Fuse overload over a list of key
// frames reads and what makes the loop of LocalMapping::SearchInNeighbors order-dependent: GetDistanceRange (the accessor of
// INTEGRATION.md section 3i), and a Replace that ends with ComputeDistinctiveDescriptors on the survivor (src/MapPoint.cc:177-215,
// :242-307), so a MapPoint's descriptor can change between two key frames of the loop.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <vector>
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#else
#include "../../../my-slam_amd/host/orbx_cv_compat.h"
#endif

namespace ORB_SLAM2 {
class KeyFrame;
class Frame;

class MapPoint {
public:
    MapPoint(const cv::Mat &Pos, const cv::Mat &normal, const cv::Mat &descriptor, float minDistance, float maxDistance)
        : mTrackProjX(0), mTrackProjY(0), mTrackProjXR(-1), mbTrackInView(false), mnTrackScaleLevel(0), mTrackViewCos(1), mnFuseCandidateForKF(0),
          mnId(nNextId++), mWorldPos(Pos.clone()), mDescriptor(descriptor.clone()), mNormalVector(normal.clone()), nObs(0), mbBad(false),
          mfMinDistance(minDistance), mfMaxDistance(maxDistance), mpReplaced(nullptr) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    int Observations() { return nObs; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    bool isBad() { return mbBad; }
    void SetBadFlag() { mbBad = true; mObservations.clear(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    void GetDistanceRange(float &mfMax, float &mfMin) { mfMax = mfMaxDistance; mfMin = mfMinDistance; }
    int PredictScale(const float &currentDist, Frame *pF);      // defined in Frame.h (needs the complete Frame)
    int PredictScale(const float &currentDist, KeyFrame *pKF);  // defined in KeyFrame.h
    void AddObservation(KeyFrame *pKF, size_t idx);             // defined in KeyFrame.h (reads pKF->mvuRight)
    int GetIndexInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }
    void Replace(MapPoint *pMP);                                // defined in KeyFrame.h
    void ComputeDistinctiveDescriptors();                       // defined in KeyFrame.h
    MapPoint *GetReplaced() { return mpReplaced; }

    float mTrackProjX, mTrackProjY, mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;
    long unsigned int mnFuseCandidateForKF;
    long unsigned int mnId;
    inline static long unsigned int nNextId = 0;

protected:
    cv::Mat mWorldPos, mDescriptor, mNormalVector;
    std::map<KeyFrame *, size_t> mObservations;
    int nObs;
    bool mbBad;
    float mfMinDistance, mfMaxDistance;
    MapPoint *mpReplaced;
};
}  // namespace ORB_SLAM2
