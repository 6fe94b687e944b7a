// MapPoint.h -- repo-authored minimal MapPoint for the test of my-slam_amd/host/MapPointDescriptors.h: only the members that
// MapPoint::ComputeDistinctiveDescriptors reads or writes (names and signatures as in the reference's include/MapPoint.h:40-150,
// bodies written here), plus SetDescriptor, the one member the integrator adds.
#pragma once
#include <map>
#include <mutex>
#if __has_include(<opencv2/core/core.hpp>)
#include <opencv2/core/core.hpp>
#else
#include "../../../my-slam_amd/host/orbx_cv_compat.h"
#endif

namespace ORB_SLAM2 {
class KeyFrame;

class MapPoint {
public:
    MapPoint(long unsigned int id, const cv::Mat &descriptor) : mnId(id), mDescriptor(descriptor.clone()), mbBad(false) {}
    void AddObservation(KeyFrame *pKF, size_t idx)
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        if (mObservations.count(pKF)) return;
        mObservations[pKF] = idx;
    }
    std::map<KeyFrame *, size_t> GetObservations()             // include/MapPoint.h:51, src/MapPoint.cc:111-115
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        return mObservations;
    }
    bool isBad()
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        return mbBad;
    }
    void SetBadFlag() { std::unique_lock<std::mutex> lock(mMutexFeatures); mbBad = true; }
    cv::Mat GetDescriptor()
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        return mDescriptor.clone();
    }
    void SetDescriptor(const cv::Mat &d)                        // the added member: src/MapPoint.cc:303-306
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        mDescriptor = d.clone();
    }
    void ComputeDistinctiveDescriptors();                       // the single-point method, rewritten over the batched call by the caller

    long unsigned int mnId;
protected:
    cv::Mat mDescriptor;
    std::map<KeyFrame *, size_t> mObservations;
    bool mbBad;
    std::mutex mMutexFeatures;
};
}  // namespace ORB_SLAM2
