// KeyFrame.h -- repo-authored minimal KeyFrame for the test of my-slam_amd/host/NewMapPoints.h (member names and types as in
// the reference's include/KeyFrame.h; only what LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:209-454, and
// MapPoint::ComputeDistinctiveDescriptors read or call).
#pragma once
#include <vector>
#include "MapPoint.h"

namespace ORB_SLAM2 {
class KeyFrame {
public:
    KeyFrame(long unsigned int id, size_t n) : mnId(id), fx(0), fy(0), cx(0), cy(0), invfx(0), invfy(0), mbf(0), mb(0), mfScaleFactor(0),
                                               mbBad(false), mvpMapPoints(n, static_cast<MapPoint *>(nullptr)) {}
    void SetPose(const float *Rcw_, const float *tcw_, const float *Ow_)
    {
        Rcw = cv::Mat(3, 3, CV_32F); tcw = cv::Mat(3, 1, CV_32F); Ow = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Rcw.at<float>(r, c) = Rcw_[3 * r + c];
            tcw.at<float>(r) = tcw_[r]; Ow.at<float>(r) = Ow_[r];
        }
    }
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    bool isBad() { return mbBad; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }

    long unsigned int mnId;
    float fx, fy, cx, cy, invfx, invfy, mbf, mb;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors;
    float mfScaleFactor;
    std::vector<float> mvScaleFactors, mvLevelSigma2;
protected:
    cv::Mat Rcw, tcw, Ow;
    bool mbBad;
    std::vector<MapPoint *> mvpMapPoints;
};
}  // namespace ORB_SLAM2
