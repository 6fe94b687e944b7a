/*
 * matcher_standin.h -- force-included (-include) in front of the reference's own src/ORBmatcher.cc, which is compiled unmodified
 * and in place for oracle/_ref/ref_matcher, and in front of the driver oracle/ref/ref_matcher.cc.  TEST INFRASTRUCTURE ONLY.
 *
 * include/ORBmatcher.h includes "MapPoint.h", "KeyFrame.h" and "Frame.h", which drag in the whole system with g2o and Eigen.  This
 * header predefines their include guards (FRAME_H, KEYFRAME_H, MAPPOINT_H), so the real headers are found and their bodies
 * skipped, and declares stand-in ORB_SLAM2::Frame, KeyFrame and MapPoint with the members src/ORBmatcher.cc touches (the list is
 * `grep -o` of its `->` and `.` members), under the reference's names and types.  It selects the linear-algebra layer of the OpenCV
 * shim (CV_SHIM_LINALG, cv_shim/cv_linalg.hpp); the Makefile selects its arithmetic variant.
 *
 * The reference's own text.  Seven members decide results and are NOT restated: the driver includes their text, sliced out of the
 * reference at build time (oracle/_ref/*.inc, never committed), after these classes:
 *     Frame::AssignFeaturesToGrid, Frame::GetFeaturesInArea, Frame::PosInGrid        src/Frame.cc:230, :327, :382
 *     KeyFrame::GetFeaturesInArea, KeyFrame::IsInImage                               src/KeyFrame.cc:569, :610
 *     MapPoint::PredictScale(float, KeyFrame*), MapPoint::PredictScale(float, Frame*)   src/MapPoint.cc:385, :402
 * Four of them are compiled under another name (`#define IsInImage IsInImage_ref` around the slice, in the driver) so that the
 * member of the reference's name can be a wrapper that logs the call and then runs the reference's text.
 *
 * What the stand-in restates, with the line it restates:
 *     FRAME_GRID_ROWS 48, FRAME_GRID_COLS 64                   include/Frame.h:37-38
 *     MapPoint::isBad, Observations                           src/MapPoint.cc:217-222, :145-149 (the stored flag / count)
 *     MapPoint::GetMin / GetMaxDistanceInvariance              src/MapPoint.cc:373-383 return 0.8f*mfMinDistance / 1.2f*mfMaxDistance;
 *                                                              here the request carries the returned value itself, as oracle_lib does
 *     MapPoint::IsInKeyFrame, GetIndexInKeyFrame               src/MapPoint.cc:315-328 (lookup in mObservations)
 *     MapPoint::AddObservation                                 src/MapPoint.cc:98-109 (no second entry per key frame; nObs += 2 for a
 *                                                              stereo feature, += 1 otherwise)
 *     MapPoint::Replace                                        src/MapPoint.cc:177-215 (same id returns; the observations are taken,
 *                                                              the point turns bad, every key frame that does not hold pMP gets
 *                                                              ReplaceMapPointMatch + pMP->AddObservation, the others
 *                                                              EraseMapPointMatch(idx); found / visible counts, the distinctive
 *                                                              descriptor and the Map are not modelled: nothing in ORBmatcher.cc reads
 *                                                              them within one call)
 *     KeyFrame::AddMapPoint, GetMapPoint, GetMapPointMatches, GetMapPoints, ReplaceMapPointMatch, EraseMapPointMatch
 *                                                              src/KeyFrame.cc:210-214, :283-287, :277-281, :235-248, :230-233, :216-220
 *     KeyFrame::GetRotation, GetTranslation, GetCameraCenter   src/KeyFrame.cc:86-108 (clones of the stored matrices; the driver stores
 *                                                              what the request gives, Ow included)
 * Together they give, on the one key frame of a Fuse call, the effect src/MapPoint.cc and src/KeyFrame.cc give: Fuse reads
 * pKF->GetMapPoint(bestIdx) (:954, :1084) after earlier slots of the same call have written to the key frame.
 *
 * The call log.  Every stand-in member appends (call, MapPoint id, argument) to ref_matcher_log(); the driver dumps it.  The
 * MapPoint id of a KeyFrame / Frame member is the MapPoint whose member was called last.  The last entry made on behalf of a
 * MapPoint tells the line at which the reference left the loop body; GetMapPoint(bestIdx) at :954 / :1084, Replace,
 * AddObservation and AddMapPoint give Fuse's best_idx per slot and its mutation sequence.
 */
#ifndef REF_MATCHER_STANDIN_H
#define REF_MATCHER_STANDIN_H

#define CV_SHIM_LINALG
#define FRAME_H
#define KEYFRAME_H
#define MAPPOINT_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"

using namespace std;

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

enum ref_matcher_call {
    RML_IS_BAD = 1, RML_OBSERVATIONS = 2, RML_GET_DESCRIPTOR = 3, RML_GET_WORLD_POS = 4, RML_IS_IN_IMAGE = 5, RML_MAX_DISTANCE = 6,
    RML_MIN_DISTANCE = 7, RML_GET_NORMAL = 8, RML_PREDICT_SCALE = 9, RML_FEATURES_IN_AREA = 10, RML_IS_IN_KEYFRAME = 11,
    RML_INDEX_IN_KEYFRAME = 12, RML_GET_MAP_POINT = 13, RML_REPLACE = 14, RML_ADD_OBSERVATION = 15, RML_ADD_MAP_POINT = 16
};

inline std::vector<int32_t> &ref_matcher_log()
{
    static std::vector<int32_t> log;
    return log;
}
inline int &ref_matcher_current()
{
    static int id = -1;
    return id;
}
inline void ref_matcher_note(int call, int id, int arg)
{
    std::vector<int32_t> &l = ref_matcher_log();
    l.push_back(call);
    l.push_back(id);
    l.push_back(arg);
}

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class MapPoint {
public:
    MapPoint(int id_) : mTrackProjX(0), mTrackProjY(0), mTrackProjXR(0), mbTrackInView(false), mnTrackScaleLevel(0), mTrackViewCos(0),
                        id(id_), mfMinDistanceInvariance(0), mfMaxDistanceInvariance(0), mbBad(false), nObs(0), mfMaxDistance(0) {}

    cv::Mat GetWorldPos() { note(RML_GET_WORLD_POS); return mWorldPos.clone(); }
    cv::Mat GetNormal() { note(RML_GET_NORMAL); return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { note(RML_GET_DESCRIPTOR); return mDescriptor.clone(); }
    bool isBad() { note(RML_IS_BAD, mbBad); return mbBad; }
    int Observations() { note(RML_OBSERVATIONS, nObs); return nObs; }
    float GetMinDistanceInvariance() { note(RML_MIN_DISTANCE); return mfMinDistanceInvariance; }
    float GetMaxDistanceInvariance() { note(RML_MAX_DISTANCE); return mfMaxDistanceInvariance; }
    bool IsInKeyFrame(KeyFrame *pKF) { note(RML_IS_IN_KEYFRAME, (int)mObservations.count(pKF)); return mObservations.count(pKF); }
    int GetIndexInKeyFrame(KeyFrame *pKF)
    {
        int idx = mObservations.count(pKF) ? (int)mObservations[pKF] : -1;
        note(RML_INDEX_IN_KEYFRAME, idx);
        return idx;
    }
    inline void AddObservation(KeyFrame *pKF, size_t idx);
    inline void Replace(MapPoint *pMP);
    int PredictScale(const float &currentDist, KeyFrame *pKF)
    {
        int level = PredictScale_ref(currentDist, pKF);
        note(RML_PREDICT_SCALE, level);
        return level;
    }
    int PredictScale(const float &currentDist, Frame *pF)
    {
        int level = PredictScale_ref(currentDist, pF);
        note(RML_PREDICT_SCALE, level);
        return level;
    }
    int PredictScale_ref(const float &currentDist, KeyFrame *pKF);      /* the reference's text, src/MapPoint.cc:385 */
    int PredictScale_ref(const float &currentDist, Frame *pF);          /* the reference's text, src/MapPoint.cc:402 */

    /* Variables used by the tracking (include/MapPoint.h:88-94) */
    float mTrackProjX;
    float mTrackProjY;
    float mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;

    /* filled by the driver */
    int id;
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistanceInvariance, mfMaxDistanceInvariance;
    bool mbBad;
    int nObs;
    std::map<KeyFrame *, size_t> mObservations;
    float mfMaxDistance;
    std::mutex mMutexPos;

private:
    void note(int call, int arg = 0)
    {
        ref_matcher_current() = id;
        ref_matcher_note(call, id, arg);
    }
};

class KeyFrame {
public:
    KeyFrame(int n, float fx_, float fy_, float cx_, float cy_, float mbf_, const float grid[6], const float bounds[4], int levels, float logsf)
        : mnGridCols(FRAME_GRID_COLS), mnGridRows(FRAME_GRID_ROWS), mfGridElementWidthInv(grid[2]), mfGridElementHeightInv(grid[3]),
          fx(fx_), fy(fy_), cx(cx_), cy(cy_), mbf(mbf_), N(n), mnScaleLevels(levels), mfLogScaleFactor(logsf),
          mnMinX((int)bounds[0]), mnMinY((int)bounds[2]), mnMaxX((int)bounds[1]), mnMaxY((int)bounds[3]), mvpMapPoints(n, (MapPoint *)0) {}

    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::set<MapPoint *> GetMapPoints()
    {
        std::set<MapPoint *> s;
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] && !mvpMapPoints[i]->mbBad) s.insert(mvpMapPoints[i]);
        return s;
    }
    MapPoint *GetMapPoint(const size_t &idx)
    {
        ref_matcher_note(RML_GET_MAP_POINT, ref_matcher_current(), (int)idx);
        return mvpMapPoints[idx];
    }
    void AddMapPoint(MapPoint *pMP, const size_t &idx)
    {
        ref_matcher_note(RML_ADD_MAP_POINT, pMP->id, (int)idx);
        mvpMapPoints[idx] = pMP;
    }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(NULL); }

    bool IsInImage(const float &x, const float &y) const
    {
        bool in = IsInImage_ref(x, y);
        ref_matcher_note(RML_IS_IN_IMAGE, ref_matcher_current(), in);
        return in;
    }
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const
    {
        std::vector<size_t> v = GetFeaturesInArea_ref(x, y, r);
        ref_matcher_note(RML_FEATURES_IN_AREA, ref_matcher_current(), (int)v.size());
        return v;
    }
    bool IsInImage_ref(const float &x, const float &y) const;                                   /* the reference's text, src/KeyFrame.cc:610 */
    std::vector<size_t> GetFeaturesInArea_ref(const float &x, const float &y, const float &r) const;    /* src/KeyFrame.cc:569 */

    /* Grid (to speed up feature matching), include/KeyFrame.h:130-133 */
    const int mnGridCols;
    const int mnGridRows;
    const float mfGridElementWidthInv;
    const float mfGridElementHeightInv;

    const float fx, fy, cx, cy, mbf;                        /* include/KeyFrame.h:154 */
    const int N;                                            /* :160 */
    std::vector<cv::KeyPoint> mvKeysUn;                     /* :164-167; const in the reference, filled by the driver here */
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;                          /* :171 */
    const int mnScaleLevels;                                /* :177-182 */
    const float mfLogScaleFactor;
    std::vector<float> mvScaleFactors;
    std::vector<float> mvLevelSigma2;
    std::vector<float> mvInvLevelSigma2;
    const int mnMinX;                                       /* :185-188 */
    const int mnMinY;
    const int mnMaxX;
    const int mnMaxY;

    std::vector<MapPoint *> mvpMapPoints;                   /* :202 */
    std::vector<std::vector<std::vector<size_t> > > mGrid;  /* :210 */
    cv::Mat Rcw, tcw, Ow;                                   /* filled by the driver */
};

class Frame {
public:
    Frame() : N(0), mb(0), mbf(0), mnScaleLevels(0), mfLogScaleFactor(0) {}

    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const
    {
        std::vector<size_t> v = GetFeaturesInArea_ref(x, y, r, minLevel, maxLevel);
        ref_matcher_note(RML_FEATURES_IN_AREA, ref_matcher_current(), (int)v.size());
        return v;
    }
    std::vector<size_t> GetFeaturesInArea_ref(const float &x, const float &y, const float &r, const int minLevel, const int maxLevel) const;   /* src/Frame.cc:327 */
    bool PosInGrid(const cv::KeyPoint &kp, int &posX, int &posY);      /* the reference's text, src/Frame.cc:382 */
    void AssignFeaturesToGrid();                                        /* the reference's text, src/Frame.cc:230 */

    static float fx;                                        /* include/Frame.h:113-116 */
    static float fy;
    static float cx;
    static float cy;
    float mbf;                                              /* :121 */
    float mb;                                               /* :124 */
    int N;                                                  /* :132 */
    std::vector<cv::KeyPoint> mvKeys;                       /* :138-139 */
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;                            /* :143 */
    DBoW2::FeatureVector mFeatVec;                          /* :148 */
    cv::Mat mDescriptors;                                   /* :151 */
    std::vector<MapPoint *> mvpMapPoints;                   /* :154 */
    std::vector<bool> mvbOutlier;                           /* :157 */
    static float mfGridElementWidthInv;                     /* :159-161 */
    static float mfGridElementHeightInv;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    cv::Mat mTcw;                                           /* :164 */
    int mnScaleLevels;                                      /* :174-178 */
    float mfLogScaleFactor;
    std::vector<float> mvScaleFactors;
    static float mnMinX;                                    /* :183-186 */
    static float mnMaxX;
    static float mnMinY;
    static float mnMaxY;
};

inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx)
{
    ref_matcher_note(RML_ADD_OBSERVATION, id, (int)idx);
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2;
    else nObs++;
}

inline void MapPoint::Replace(MapPoint *pMP)
{
    ref_matcher_note(RML_REPLACE, id, pMP->id);
    if (pMP->id == this->id) return;
    std::map<KeyFrame *, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    for (std::map<KeyFrame *, size_t>::iterator mit = obs.begin(), mend = obs.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        if (!pMP->mObservations.count(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else {
            pKF->EraseMapPointMatch(mit->second);
        }
    }
}

}
#endif
