// KeyFrame.h, MapPoint and Map -- repo-authored minimal classes for the BundleAdjustment adapter test (member names and types as in
// the reference's include/KeyFrame.h, include/MapPoint.h and include/Map.h; only what Optimizer::BundleAdjustment and
// GlobalBundleAdjustemnt read or call, bodies written here).
#pragma once
#include <map>
#include <vector>
#include "orbx_cv_compat.h"

namespace ORB_SLAM2 {
class KeyFrame;

class MapPoint {
public:
    MapPoint(long unsigned int id, const cv::Mat &Pos) : mnId(id), mnBAGlobalForKF(0), mWorldPos(Pos.clone()) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); nSetWorldPos++; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    void UpdateNormalAndDepth() { nUpdateNormalAndDepth++; }
    bool isBad() { return mbBad; }

    long unsigned int mnId;
    cv::Mat mPosGBA;
    long unsigned int mnBAGlobalForKF;
    bool mbBad = false;
    int nSetWorldPos = 0, nUpdateNormalAndDepth = 0;            // what the test counts
protected:
    cv::Mat mWorldPos;
    std::map<KeyFrame *, size_t> mObservations;
};

class KeyFrame {
public:
    KeyFrame(long unsigned int id, float fx_, float fy_, float cx_, float cy_, float bf, const cv::Mat &Tcw_, const std::vector<float> &invLevelSigma2)
        : mnId(id), mnBAGlobalForKF(0), fx(fx_), fy(fy_), cx(cx_), cy(cy_), mbf(bf), mvInvLevelSigma2(invLevelSigma2), Tcw(Tcw_.clone()) {}
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); nSetPose++; }
    bool isBad() { return mbBad; }
    size_t AddFeature(const cv::KeyPoint &kp, float uRight)     // the test's builder
    {
        mvKeysUn.push_back(kp); mvuRight.push_back(uRight);
        return mvKeysUn.size() - 1;
    }

    long unsigned int mnId;
    cv::Mat mTcwGBA;
    long unsigned int mnBAGlobalForKF;
    const float fx, fy, cx, cy, mbf;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    const std::vector<float> mvInvLevelSigma2;
    bool mbBad = false;
    int nSetPose = 0;
protected:
    cv::Mat Tcw;
};

class Map {
public:
    void AddKeyFrame(KeyFrame *pKF) { mspKeyFrames.push_back(pKF); }
    void AddMapPoint(MapPoint *pMP) { mspMapPoints.push_back(pMP); }
    std::vector<KeyFrame *> GetAllKeyFrames() { return mspKeyFrames; }
    std::vector<MapPoint *> GetAllMapPoints() { return mspMapPoints; }
    long unsigned int MapPointsInMap() { return mspMapPoints.size(); }
protected:
    std::vector<KeyFrame *> mspKeyFrames;                       // the reference keeps std::set; the order here is the test's
    std::vector<MapPoint *> mspMapPoints;
};
}   // namespace ORB_SLAM2
