// KeyFrame.h, MapPoint and Map -- repo-authored minimal classes for the OptimizeEssentialGraph adapter test (member names and types
// as in the reference's include/KeyFrame.h, include/MapPoint.h and include/Map.h; only what Optimizer::OptimizeEssentialGraph reads
// or calls, bodies written here).
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include "orbx_cv_compat.h"

namespace ORB_SLAM2 {
class KeyFrame;

class MapPoint {
public:
    MapPoint(long unsigned int id, const cv::Mat &Pos, KeyFrame *pRefKF) : mnId(id), mWorldPos(Pos.clone()), mpRefKF(pRefKF) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); nSetWorldPos++; }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    void UpdateNormalAndDepth() { nUpdateNormalAndDepth++; }
    bool isBad() { return mbBad; }

    long unsigned int mnId;
    long unsigned int mnCorrectedByKF = 0;
    long unsigned int mnCorrectedReference = 0;
    bool mbBad = false;
    int nSetWorldPos = 0, nUpdateNormalAndDepth = 0;            // what the test counts
protected:
    cv::Mat mWorldPos;
    KeyFrame *mpRefKF;
};

class KeyFrame {
public:
    KeyFrame(long unsigned int id, const cv::Mat &Tcw_) : mnId(id), Tcw(Tcw_.clone()) {}
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); nSetPose++; }
    cv::Mat GetRotation()
    {
        cv::Mat R(3, 3, CV_32F);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c);
        return R;
    }
    cv::Mat GetTranslation()
    {
        cv::Mat t(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) t.at<float>(r) = Tcw.at<float>(r, 3);
        return t;
    }
    bool isBad() { return mbBad; }
    int GetWeight(KeyFrame *pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    KeyFrame *GetParent() { return mpParent; }
    bool hasChild(KeyFrame *pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame *> GetLoopEdges() { return mspLoopEdges; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w)
    {
        nAskedWeight = w;
        return mvpOrderedConnectedKeyFrames;
    }

    long unsigned int mnId;
    bool mbBad = false;
    int nSetPose = 0, nAskedWeight = -1;
    // the test's builder writes these directly
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;       // what GetCovisiblesByWeight(100) hands back, a NULL included
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens, mspLoopEdges;
protected:
    cv::Mat Tcw;
};

class Map {
public:
    void AddKeyFrame(KeyFrame *pKF) { mspKeyFrames.push_back(pKF); }
    void AddMapPoint(MapPoint *pMP) { mspMapPoints.push_back(pMP); }
    std::vector<KeyFrame *> GetAllKeyFrames() { return mspKeyFrames; }
    std::vector<MapPoint *> GetAllMapPoints() { return mspMapPoints; }
    long unsigned int GetMaxKFid()
    {
        long unsigned int m = 0;
        for (KeyFrame *pKF : mspKeyFrames) m = std::max(m, pKF->mnId);
        return m;
    }
    std::mutex mMutexMapUpdate;
protected:
    std::vector<KeyFrame *> mspKeyFrames;                       // the reference keeps std::set; the order here is the test's
    std::vector<MapPoint *> mspMapPoints;
};
}   // namespace ORB_SLAM2
