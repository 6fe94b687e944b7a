// MapPoint.h -- repo-authored minimal MapPoint for the test of my-slam_amd/host/NewMapPoints.h: the members that
// LocalMapping::CreateNewMapPoints' bookkeeping (src/LocalMapping.cc:436-451) and the batched descriptor call touch (names and
// signatures as in the reference's include/MapPoint.h, bodies written here), plus SetDescriptor.
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
class Map;

class MapPoint {
public:
    MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : mnId(nNextId++), mpRefKF(pRefKF), mpMap(pMap), mWorldPos(Pos.clone()), mbBad(false), nNormalUpdates(0) {}
    void AddObservation(KeyFrame *pKF, size_t idx)
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        if (mObservations.count(pKF)) return;
        mObservations[pKF] = idx;
    }
    std::map<KeyFrame *, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mObservations; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mbBad; }
    cv::Mat GetDescriptor() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mDescriptor.clone(); }
    void SetDescriptor(const cv::Mat &d) { std::unique_lock<std::mutex> lock(mMutexFeatures); mDescriptor = d.clone(); }
    void UpdateNormalAndDepth() { nNormalUpdates++; }           // counted, not computed: not part of what is under test

    long unsigned int mnId;
    static long unsigned int nNextId;
    int nNormalUpdatesDone() const { return nNormalUpdates; }
protected:
    KeyFrame *mpRefKF;
    Map *mpMap;
    cv::Mat mWorldPos, mDescriptor;
    std::map<KeyFrame *, size_t> mObservations;
    bool mbBad;
    int nNormalUpdates;
    std::mutex mMutexFeatures;
};
}  // namespace ORB_SLAM2
