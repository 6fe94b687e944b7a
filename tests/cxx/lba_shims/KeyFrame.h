// KeyFrame.h, MapPoint and Map -- repo-authored minimal classes for the LocalBundleAdjustment adapter test (member names and types
// as in the reference's include/KeyFrame.h, include/MapPoint.h and include/Map.h; only what Optimizer::LocalBundleAdjustment reads
// or calls, bodies written here).
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>
#include "orbx_cv_compat.h"

namespace ORB_SLAM2 {
class KeyFrame;

class MapPoint {
public:
    MapPoint(long unsigned int id, const cv::Mat &Pos) : mnId(id), mnBALocalForKF(0), mWorldPos(Pos.clone()) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); nSetWorldPos++; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    void EraseObservation(KeyFrame *pKF) { mObservations.erase(pKF); nEraseObservation++; }
    void UpdateNormalAndDepth() { nUpdateNormalAndDepth++; }
    bool isBad() { return mbBad; }

    long unsigned int mnId;
    long unsigned int mnBALocalForKF;
    bool mbBad = false;
    int nSetWorldPos = 0, nEraseObservation = 0, nUpdateNormalAndDepth = 0;     // what the test counts
protected:
    cv::Mat mWorldPos;
    std::map<KeyFrame *, size_t> mObservations;
};

class KeyFrame {
public:
    KeyFrame(long unsigned int id, float fx_, float fy_, float cx_, float cy_, float bf, const cv::Mat &Tcw_, const std::vector<float> &invLevelSigma2)
        : mnId(id), mnBALocalForKF(0), mnBAFixedForKF(0), fx(fx_), fy(fy_), cx(cx_), cy(cy_), mbf(bf), mvInvLevelSigma2(invLevelSigma2), Tcw(Tcw_.clone()) {}
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); nSetPose++; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    void EraseMapPointMatch(MapPoint *pMP)                  // src/KeyFrame.cc:226-231
    {
        const auto it = pMP->GetObservations().find(this);
        (void)it;
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] == pMP) mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
        nEraseMapPointMatch++;
    }
    bool isBad() { return mbBad; }
    // the test's builder: feature idx of this key frame observes pMP
    size_t AddFeature(const cv::KeyPoint &kp, float uRight, MapPoint *pMP)
    {
        mvKeysUn.push_back(kp); mvuRight.push_back(uRight); mvpMapPoints.push_back(pMP);
        return mvKeysUn.size() - 1;
    }

    long unsigned int mnId;
    long unsigned int mnBALocalForKF, mnBAFixedForKF;
    const float fx, fy, cx, cy, mbf;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    const std::vector<float> mvInvLevelSigma2;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    bool mbBad = false;
    int nSetPose = 0, nEraseMapPointMatch = 0;
protected:
    cv::Mat Tcw;
    std::vector<MapPoint *> mvpMapPoints;
};

class Map {
public:
    std::mutex mMutexMapUpdate;
};
}   // namespace ORB_SLAM2
