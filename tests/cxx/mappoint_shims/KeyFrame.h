// KeyFrame.h -- repo-authored minimal KeyFrame for the test of my-slam_amd/host/MapPointDescriptors.h (member names and types as
// in the reference's include/KeyFrame.h; only what MapPoint::ComputeDistinctiveDescriptors and its callers in
// src/LocalMapping.cc:141-163, :519-532 read or call).
#pragma once
#include <vector>
#include "MapPoint.h"

namespace ORB_SLAM2 {
class KeyFrame {
public:
    KeyFrame(long unsigned int id, const cv::Mat &descriptors) : mnId(id), mDescriptors(descriptors.clone()), mbBad(false) {}
    bool isBad() { return mbBad; }
    void SetBadFlag() { mbBad = true; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    void AddMapPoint(MapPoint *pMP) { mvpMapPoints.push_back(pMP); }

    long unsigned int mnId;
    const cv::Mat mDescriptors;
protected:
    bool mbBad;
    std::vector<MapPoint *> mvpMapPoints;
};
}  // namespace ORB_SLAM2
