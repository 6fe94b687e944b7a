// KeyFrame.h -- repo-authored minimal KeyFrame for tests/cxx/fuse_views_callsites.cc (member names and types as in the reference's
// include/KeyFrame.h; bodies written here).  Beyond tests/cxx/slam_shims/KeyFrame.h it has the grid: the cells are filled the way
// Frame::AssignFeaturesToGrid does with the frame's float image origin (src/Frame.cc:230-245, :382-392; a key frame copies that grid,
// src/KeyFrame.cc:48-54), and GetFeaturesInArea walks them as src/KeyFrame.cc:569-606 does with the key frame's int origin: cell
// column by cell column, row by row, push_back order, |dx| < r && |dy| < r.
#pragma once
#include <cmath>
#include <map>
#include <set>
#include <vector>
#include "MapPoint.h"

#ifndef ORBX_SHIM_DBOW2
#define ORBX_SHIM_DBOW2
namespace DBoW2 {              // Thirdparty/DBoW2/DBoW2/FeatureVector.h: a std::map<NodeId, std::vector<unsigned int>>
typedef unsigned int NodeId;
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
}
#endif

namespace ORB_SLAM2 {
class KeyFrame {
public:
    static const int GRID_COLS = 64, GRID_ROWS = 48;          // FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:37-38
    // what KeyFrame::KeyFrame(Frame&, ...) copies from the frame (src/KeyFrame.cc:30-57); frameMinX / frameMinY are the frame's float
    // mnMinX / mnMinY, truncated to int by the member initialisers mnMinX(F.mnMinX) ... as in the reference
    KeyFrame(long unsigned int id, const std::vector<cv::KeyPoint> &keysUn, const std::vector<float> &uRight, const cv::Mat &descriptors,
             float fx_, float fy_, float cx_, float cy_, float bf, float gridWInv, float gridHInv, float frameMinX, float frameMinY, float frameMaxX,
             float frameMaxY, const std::vector<float> &scaleFactors, const std::vector<float> &invLevelSigma2, float logScaleFactor)
        : mnId(id), mnFuseTargetForKF(0), mfGridElementWidthInv(gridWInv), mfGridElementHeightInv(gridHInv), fx(fx_), fy(fy_), cx(cx_), cy(cy_), mbf(bf),
          N((int)keysUn.size()), mvKeysUn(keysUn), mvuRight(uRight), mDescriptors(descriptors.clone()), mnScaleLevels((int)scaleFactors.size()),
          mfLogScaleFactor(logScaleFactor), mvScaleFactors(scaleFactors), mvInvLevelSigma2(invLevelSigma2), mnMinX(frameMinX), mnMinY(frameMinY),
          mnMaxX(frameMaxX), mnMaxY(frameMaxY), mvpMapPoints(keysUn.size(), static_cast<MapPoint *>(NULL)), mbBad(false)
    {
        mGrid.resize(GRID_COLS);
        for (int i = 0; i < GRID_COLS; i++) mGrid[i].resize(GRID_ROWS);
        for (int i = 0; i < N; i++) {                          // Frame::AssignFeaturesToGrid / PosInGrid
            const cv::KeyPoint &kp = mvKeysUn[i];
            const int posX = (int)round((kp.pt.x - frameMinX) * mfGridElementWidthInv);
            const int posY = (int)round((kp.pt.y - frameMinY) * mfGridElementHeightInv);
            if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) continue;
            mGrid[posX][posY].push_back(i);
        }
    }

    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); }
    void SetCameraCenter(const cv::Mat &Ow_) { Ow = Ow_.clone(); }    // Ow = -Rwc*tcw is a cv::Mat product: the test passes it in
    cv::Mat GetRotation() { cv::Mat R(3, 3, CV_32F); for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    cv::Mat GetTranslation() { cv::Mat t(3, 1, CV_32F); for (int r = 0; r < 3; r++) t.at<float>(r) = Tcw.at<float>(r, 3); return t; }
    cv::Mat GetCameraCenter() { return Ow.clone(); }

    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    std::set<MapPoint *> GetMapPoints()
    {
        std::set<MapPoint *> s;
        for (MapPoint *p : mvpMapPoints) if (p && !p->isBad()) s.insert(p);
        return s;
    }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(NULL); }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    bool IsInImage(const float &x, const float &y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    bool isBad() { return mbBad; }

    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const
    {
        std::vector<size_t> vIndices;
        vIndices.reserve(N);
        const int nMinCellX = std::max(0, (int)floor((x - mnMinX - r) * mfGridElementWidthInv));
        if (nMinCellX >= GRID_COLS) return vIndices;
        const int nMaxCellX = std::min((int)GRID_COLS - 1, (int)ceil((x - mnMinX + r) * mfGridElementWidthInv));
        if (nMaxCellX < 0) return vIndices;
        const int nMinCellY = std::max(0, (int)floor((y - mnMinY - r) * mfGridElementHeightInv));
        if (nMinCellY >= GRID_ROWS) return vIndices;
        const int nMaxCellY = std::min((int)GRID_ROWS - 1, (int)ceil((y - mnMinY + r) * mfGridElementHeightInv));
        if (nMaxCellY < 0) return vIndices;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t> &vCell = mGrid[ix][iy];
                for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
                    const cv::KeyPoint &kpUn = mvKeysUn[vCell[j]];
                    const float distx = kpUn.pt.x - x;
                    const float disty = kpUn.pt.y - y;
                    if (fabs(distx) < r && fabs(disty) < r) vIndices.push_back(vCell[j]);
                }
            }
        }
        return vIndices;
    }

    long unsigned int mnId;
    long unsigned int mnFuseTargetForKF;
    const float mfGridElementWidthInv, mfGridElementHeightInv;
    const float fx, fy, cx, cy, mbf;
    const int N;
    const std::vector<cv::KeyPoint> mvKeysUn;
    const std::vector<float> mvuRight;
    const cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    const int mnScaleLevels;
    const float mfLogScaleFactor;
    const std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    const int mnMinX, mnMinY, mnMaxX, mnMaxY;
protected:
    cv::Mat Tcw, Ow;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    bool mbBad;
};

// MapPoint::PredictScale(dist, KeyFrame*) with the reference's arithmetic (src/MapPoint.cc:385-400)
inline int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF)
{
    float ratio = mfMaxDistance / currentDist;
    int nScale = (int)std::ceil(std::log(ratio) / pKF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
    return nScale;
}
inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx)      // src/MapPoint.cc:98-109
{
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2; else nObs++;
}
inline void MapPoint::ComputeDistinctiveDescriptors()                 // src/MapPoint.cc:242-307
{
    if (mbBad || mObservations.empty()) return;
    std::vector<cv::Mat> vDescriptors;
    for (auto &o : mObservations)
        if (!o.first->isBad()) vDescriptors.push_back(o.first->mDescriptors.row((int)o.second));
    if (vDescriptors.empty()) return;
    const size_t N = vDescriptors.size();
    std::vector<std::vector<int> > Distances(N, std::vector<int>(N, 0));
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) {
            int d = 0;
            const unsigned char *a = vDescriptors[i].ptr<unsigned char>(), *b = vDescriptors[j].ptr<unsigned char>();
            for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
            Distances[i][j] = d; Distances[j][i] = d;
        }
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances[i]);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (N - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    mDescriptor = vDescriptors[BestIdx].clone();
}
inline void MapPoint::Replace(MapPoint *pMP)                          // src/MapPoint.cc:177-215 without the Map and the found / visible counters
{
    if (pMP->mnId == this->mnId) return;
    std::map<KeyFrame *, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    mpReplaced = pMP;
    for (auto &o : obs) {
        KeyFrame *pKF = o.first;
        if (!pMP->IsInKeyFrame(pKF)) { pKF->ReplaceMapPointMatch(o.second, pMP); pMP->AddObservation(pKF, o.second); }
        else pKF->EraseMapPointMatch(o.second);
    }
    pMP->ComputeDistinctiveDescriptors();
}
}  // namespace ORB_SLAM2
