// Frame.h -- repo-authored minimal Frame for tests/cxx/fuse_views_callsites.cc: the members my-slam_amd/host/ORBmatcher.h names
// (as in the reference's include/Frame.h:100-190), so that the header compiles; the Fuse tests make no Frame.  The static image
// origin (mnMinX, mnMinY) is what a key frame's grid cells were assigned with (src/Frame.cc:382-392).
#pragma once
#include <cmath>
#include <vector>
#include "KeyFrame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {
class Frame {
public:
    Frame() : mbf(0), mb(0), N(0), mnId(0), mnScaleLevels(0), mfScaleFactor(1), mfLogScaleFactor(0) {}
    inline static float fx = 0, fy = 0, cx = 0, cy = 0;
    float mbf, mb;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors, mDescriptorsRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw;
    long unsigned int mnId;
    int mnScaleLevels;
    float mfScaleFactor, mfLogScaleFactor;
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    inline static float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    inline static float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
};

// MapPoint::PredictScale(dist, Frame*) with the reference's arithmetic (src/MapPoint.cc:402-417)
inline int MapPoint::PredictScale(const float &currentDist, Frame *pF)
{
    float ratio = mfMaxDistance / currentDist;
    int nScale = (int)std::ceil(std::log(ratio) / pF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pF->mnScaleLevels) nScale = pF->mnScaleLevels - 1;
    return nScale;
}
}  // namespace ORB_SLAM2
