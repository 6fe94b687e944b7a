/*
 * mapping_standin.h -- force-included (-include) in front of the reference's own src/MapPoint.cc, which is compiled unmodified and
 * in place for oracle/_ref/ref_mapping, and in front of the driver oracle/ref/ref_mapping.cc.  TEST INFRASTRUCTURE ONLY.
 *
 * include/MapPoint.h includes "KeyFrame.h", "Frame.h" and "Map.h", which drag in the whole system with g2o and Eigen.  This header
 * predefines their include guards (FRAME_H, KEYFRAME_H, MAP_H), so the real headers are found and their bodies skipped, and declares
 * stand-in ORB_SLAM2::Map, KeyFrame and Frame with the members that src/MapPoint.cc and the slices below touch, under the
 * reference's names and types.  MapPoint is the reference's own class (include/MapPoint.h, src/MapPoint.cc); include/ORBmatcher.h
 * is the reference's own too.  It selects the linear-algebra layer of the OpenCV shim (CV_SHIM_LINALG, cv_shim/cv_linalg.hpp); the
 * Makefile selects its arithmetic variant.
 *
 * The reference's own text.  These decide results and are NOT restated: the whole of src/MapPoint.cc, and the slices the driver
 * includes, cut out of the reference at build time (oracle/_ref/*.inc, never committed):
 *     Frame::isInFrustum                                                  src/Frame.cc:269
 *     KeyFrame::UnprojectStereo, KeyFrame::ComputeSceneMedianDepth        src/KeyFrame.cc:615, :633
 *     LocalMapping::CreateNewMapPoints, ComputeF12, SkewSymmetricMatrix   src/LocalMapping.cc:209, :538, :700
 *     ORBmatcher::DescriptorDistance                                      src/ORBmatcher.cc:1647
 * KeyFrame::UnprojectStereo is compiled under another name (`#define UnprojectStereo UnprojectStereo_ref` around the slice, in the
 * driver) so that the member of the reference's name can note the call (and a feature without depth) before it runs the reference's text.
 *
 * What the stand-in restates, with the line it restates:
 *     Map::EraseMapPoint, AddMapPoint                        src/Map.cc:43-57 (the set of points; AddMapPoint also logs the new point)
 *     KeyFrame::AddMapPoint, GetMapPoint                     src/KeyFrame.cc:210-214, :283-287
 *     KeyFrame::EraseMapPointMatch, ReplaceMapPointMatch     src/KeyFrame.cc:216-220, :230-233
 *     KeyFrame::GetRotation, GetTranslation, GetCameraCenter src/KeyFrame.cc:86-108 (clones of the stored matrices; the driver stores
 *                                                            what the request gives, Ow and Twc included)
 *     KeyFrame::isBad                                        src/KeyFrame.cc:520-524 (the stored flag)
 *     KeyFrame::GetBestCovisibilityKeyFrames                 src/KeyFrame.cc:164-172: here it returns the request's list
 *     Frame::GetCameraCenter                                 include/Frame.h:81-83
 *     KeyFrame::GetMapPointMatches                           src/KeyFrame.cc:277-281
 * For the whole-loop build (oracle/_ref/ref_newpoints, which links src/ORBmatcher.cc unmodified for its SearchForTriangulation) the two
 * classes also carry the members the other searches of that file name; KeyFrame::GetMapPoints, IsInImage and both GetFeaturesInArea
 * are declared only, and the driver defines them to stop the run: CreateNewMapPoints reaches none of them.
 *
 * cos / atan2 / log.  src/LocalMapping.cc:314-316 calls cos and atan2 of floats and src/MapPoint.cc:393, :410 log of a float, from
 * inside namespace ORB_SLAM2.  Declaring ORB_SLAM2::cos(float), atan2(float, float) and log(float) here makes unqualified lookup
 * stop in that namespace (the precedent of ref_sincos.h), so the calls bind to the driver's definitions: the correctly rounded
 * float values the project takes as canonical, or glibc's cosf / atan2f / logf with -DREF_LIBM_MATH (measure).
 */
#ifndef REF_MAPPING_STANDIN_H
#define REF_MAPPING_STANDIN_H

#define CV_SHIM_LINALG
#define FRAME_H
#define KEYFRAME_H
#define MAP_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"

using namespace std;

namespace ORB_SLAM2 {

float cos(float x);
float atan2(float y, float x);
float log(float x);

class MapPoint;
class KeyFrame;
class Frame;

void ref_mapping_new_point(MapPoint *pMP);          /* the driver's: reads the new point's position and observations */
void ref_mapping_unproject(KeyFrame *pKF, int i);   /* the driver's: notes the call; leaves the loop where the depth is not > 0 */

class Map {
public:
    void AddMapPoint(MapPoint *pMP)
    {
        mspMapPoints.insert(pMP);
        ref_mapping_new_point(pMP);
    }
    void EraseMapPoint(MapPoint *pMP) { mspMapPoints.erase(pMP); }

    std::mutex mMutexPointCreation;                         /* include/Map.h:62 */
    std::set<MapPoint *> mspMapPoints;                      /* :65 */
};

class KeyFrame {
public:
    KeyFrame() : mnId(0), mnFrameId(0), fx(0), fy(0), cx(0), cy(0), invfx(0), invfy(0), mbf(0), mb(0), N(0), mnScaleLevels(0),
                 mfScaleFactor(0), mfLogScaleFactor(0), mbBad(false) {}

    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    bool isBad() { return mbBad; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(NULL); }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &) { return mvpNeighbours; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    /* declared for the searches of src/ORBmatcher.cc that the whole-loop build (ref_newpoints) links but never calls; the driver
       defines them to stop the run */
    std::set<MapPoint *> GetMapPoints();
    bool IsInImage(const float &x, const float &y) const;
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const;

    cv::Mat UnprojectStereo(int i)
    {
        ref_mapping_unproject(this, i);
        return UnprojectStereo_ref(i);
    }
    cv::Mat UnprojectStereo_ref(int i);                     /* the reference's text, src/KeyFrame.cc:615 */
    float ComputeSceneMedianDepth(const int q);             /* the reference's text, src/KeyFrame.cc:633 */

    long unsigned int mnId;                                 /* include/KeyFrame.h:122-123 */
    long unsigned int mnFrameId;
    float fx, fy, cx, cy, invfx, invfy, mbf, mb;            /* :154; const in the reference, filled by the driver here */
    int N;                                                  /* :160 */
    std::vector<cv::KeyPoint> mvKeys;                       /* :164-169 */
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<float> mvDepth;
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;                          /* :171 */
    int mnScaleLevels;                                      /* :177-182 */
    float mfScaleFactor;
    float mfLogScaleFactor;
    std::vector<float> mvScaleFactors;
    std::vector<float> mvLevelSigma2;
    std::vector<float> mvInvLevelSigma2;
    cv::Mat mK;                                             /* :189 */
    cv::Mat Tcw, Twc, Ow;                                   /* :196-199 */
    std::vector<MapPoint *> mvpMapPoints;                   /* :202 */
    std::mutex mMutexPose;                                  /* :230, :232 */
    std::mutex mMutexFeatures;

    /* filled by the driver */
    bool mbBad;
    std::vector<KeyFrame *> mvpNeighbours;
};

class Frame {
public:
    Frame() : mbf(0), mb(0), N(0), mnId(0), mnScaleLevels(0), mfLogScaleFactor(0) {}

    bool isInFrustum(MapPoint *pMP, float viewingCosLimit);     /* the reference's text, src/Frame.cc:269 */
    cv::Mat GetCameraCenter() { return mOw.clone(); }
    /* as KeyFrame's: linked by ref_newpoints, never called */
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const;

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
    cv::Mat mTcw;                                           /* :164 */
    long unsigned int mnId;                                 /* :168 */
    int mnScaleLevels;                                      /* :174-178 */
    float mfLogScaleFactor;
    std::vector<float> mvScaleFactors;
    static float mnMinX;                                    /* :183-186 */
    static float mnMaxX;
    static float mnMinY;
    static float mnMaxY;
    cv::Mat mRcw, mtcw, mOw;                                /* :202-205; filled by the driver */
};

}
#endif
