// Frame.h -- repo-authored minimal Frame for tests/cxx/localpoints_callsites.cc (member names as in the reference's
// include/Frame.h): what Tracking::SearchLocalPoints reads of mCurrentFrame, and Frame::isInFrustum written out with the
// arithmetic OpenCV 3.1.0 gives the reference's expressions (src/Frame.cc:269-325): mRcw*P+mtcw through
// cv::gemm's small-matrix path, cv::norm and Mat::dot accumulating in double.  Compile with -ffp-contract=off.
#pragma once
#include <cmath>
#include <vector>
#include "MapPoint.h"

namespace ORB_SLAM2 {
class Frame {
public:
    Frame() : mbf(0), mnId(0), mnScaleLevels(0), mfLogScaleFactor(0) {}
    // the blocks of mTcw and the camera centre, as Frame::UpdatePoseMatrices leaves them (src/Frame.cc:261-266); mOw is given
    void SetPose(const float Rcw[9], const float tcw[3], const float Ow[3])
    {
        mTcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) mTcw.at<float>(r, c) = r == c ? 1.f : 0.f;
        mOw = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) mTcw.at<float>(r, c) = Rcw[3 * r + c];
            mTcw.at<float>(r, 3) = tcw[r];
            mOw.at<float>(r) = Ow[r];
        }
    }
    cv::Mat GetCameraCenter() { return mOw.clone(); }

    bool isInFrustum(MapPoint *pMP, float viewingCosLimit)
    {
        pMP->mbTrackInView = false;
        const cv::Mat P = pMP->GetWorldPos();
        const float p[3] = {P.at<float>(0), P.at<float>(1), P.at<float>(2)};
        float Pc[3];
        for (int r = 0; r < 3; r++) {           // mRcw*P+mtcw
            const float t0 = mTcw.at<float>(r, 0) * p[0] + mTcw.at<float>(r, 1) * p[1] + mTcw.at<float>(r, 2) * p[2];
            Pc[r] = (float)((double)t0 * 1.0 + (double)mTcw.at<float>(r, 3) * 1.0);
        }
        const float &PcX = Pc[0], &PcY = Pc[1], &PcZ = Pc[2];
        if (PcZ < 0.0f)
            return false;
        const float invz = 1.0f / PcZ;
        const float u = fx * PcX * invz + cx;
        const float v = fy * PcY * invz + cy;
        if (u < mnMinX || u > mnMaxX)
            return false;
        if (v < mnMinY || v > mnMaxY)
            return false;
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        float PO[3];
        double nn = 0, dot = 0;
        const cv::Mat Pn = pMP->GetNormal();
        for (int k = 0; k < 3; k++) {
            PO[k] = p[k] - mOw.at<float>(k);
            nn += (double)PO[k] * (double)PO[k];
            dot += (double)PO[k] * (double)Pn.at<float>(k);
        }
        const float dist = (float)std::sqrt(nn);
        if (dist < minDistance || dist > maxDistance)
            return false;
        const float viewCos = (float)(dot / dist);
        if (viewCos < viewingCosLimit)
            return false;
        const int nPredictedLevel = pMP->PredictScale(dist, this);
        pMP->mbTrackInView = true;
        pMP->mTrackProjX = u;
        pMP->mTrackProjXR = u - mbf * invz;
        pMP->mTrackProjY = v;
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;
        return true;
    }

    inline static float fx = 0, fy = 0, cx = 0, cy = 0;
    float mbf;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat mTcw;
    long unsigned int mnId;
    int mnScaleLevels;
    float mfLogScaleFactor;
    std::vector<float> mvScaleFactors;
    inline static float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;

private:
    cv::Mat mOw;
};

// MapPoint::PredictScale(dist, Frame*) with the reference's arithmetic (src/MapPoint.cc:402-417): float ratio, log of a float, ceil
inline int MapPoint::PredictScale(const float &currentDist, Frame *pF)
{
    float ratio = mfMaxDistance / currentDist;
    int nScale = (int)std::ceil(std::log(ratio) / pF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pF->mnScaleLevels) nScale = pF->mnScaleLevels - 1;
    return nScale;
}
}  // namespace ORB_SLAM2
