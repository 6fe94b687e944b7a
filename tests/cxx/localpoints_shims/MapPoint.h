// MapPoint.h -- repo-authored minimal MapPoint for tests/cxx/localpoints_callsites.cc: the members Tracking::SearchLocalPoints,
// Frame::isInFrustum and ORBmatcher::SearchByProjection(F, vpMapPoints, th) read or write (names and signatures as in the
// reference's include/MapPoint.h, bodies written here), plus the accessor INTEGRATION.md 3i adds.
#pragma once
#include <cmath>
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#else
#include "../../../my-slam_amd/host/orbx_cv_compat.h"
#endif

namespace ORB_SLAM2 {
class Frame;

class MapPoint {
public:
    MapPoint(const float P[3], const float normal[3], const unsigned char desc[32], int observations, float maxDistance, float minDistance)
        : mTrackProjX(-1), mTrackProjY(-1), mTrackProjXR(-1), mbTrackInView(false), mnTrackScaleLevel(-1), mTrackViewCos(-1),
          mnLastFrameSeen(0), mnVisible(1), mWorldPos(3, 1, CV_32F), mNormalVector(3, 1, CV_32F), mDescriptor(1, 32, CV_8U), nObs(observations),
          mbBad(false), mfMinDistance(minDistance), mfMaxDistance(maxDistance)
    {
        for (int k = 0; k < 3; k++) { mWorldPos.at<float>(k) = P[k]; mNormalVector.at<float>(k) = normal[k]; }
        for (int k = 0; k < 32; k++) mDescriptor.ptr<unsigned char>()[k] = desc[k];
    }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    void SetBadFlag() { mbBad = true; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    int PredictScale(const float &currentDist, Frame *pF);      // defined in Frame.h (needs the complete Frame)
    // the accessor of INTEGRATION.md 3i (in the reference's tree it takes mMutexPos)
    void GetDistanceRange(float &mfMax, float &mfMin) { mfMax = mfMaxDistance; mfMin = mfMinDistance; }

    // Variables used by the tracking (public in the reference too)
    float mTrackProjX, mTrackProjY, mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;
    long unsigned int mnLastFrameSeen;
    int mnVisible;                                               // protected in the reference; the test compares it

protected:
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    int nObs;
    bool mbBad;
    float mfMinDistance, mfMaxDistance;
};
}  // namespace ORB_SLAM2
