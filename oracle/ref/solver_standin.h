/*
 * solver_standin.h -- force-included (-include) in front of the reference's own src/Sim3Solver.cc, src/PnPsolver.cc and
 * src/Initializer.cc, which are compiled unmodified and in place for oracle/_ref/ref_sim3, ref_pnp and ref_init.
 * TEST INFRASTRUCTURE ONLY.
 *
 * The three files include "Frame.h", "KeyFrame.h", "MapPoint.h", "ORBmatcher.h" and (Initializer.cc) "Optimizer.h", which drag in
 * the whole system with g2o and Eigen.  This header predefines their include guards (FRAME_H, KEYFRAME_H, MAPPOINT_H,
 * ORBMATCHER_H, OPTIMIZER_H), so the real headers are found and their bodies skipped, and declares stand-in ORB_SLAM2::Frame,
 * KeyFrame and MapPoint with exactly the members the three .cc files touch, under the reference's names and types:
 *   KeyFrame   GetRotation / GetTranslation (include/KeyFrame.h:54-55), GetMapPointMatches (:89), mvKeysUn (:164),
 *              mvLevelSigma2 (:181), mK (:189)                                   -- src/Sim3Solver.cc:43-106
 *   MapPoint   GetWorldPos (include/MapPoint.h:46), GetIndexInKeyFrame (:57), isBad (:61)
 *                                                                               -- src/Sim3Solver.cc:72-97, src/PnPsolver.cc:85-92
 *   Frame      mK (include/Frame.h:112), fx, fy, cx, cy (:113-116, static), mvKeysUn (:138), mvpMapPoints (:153),
 *              mvLevelSigma2 (:179)                    -- src/PnPsolver.cc:72-107, src/Initializer.cc:35-37, :49
 * It also selects the linear-algebra layer of the OpenCV shim (CV_SHIM_LINALG, cv_shim/cv_linalg.hpp).
 *
 * The stand-ins are plain data that a driver fills.  The reference's members are const in KeyFrame; the driver fills them through
 * the constructor.  A MapPoint knows its index in each key frame through a small table (the reference looks it up in
 * mObservations).  The real headers bring `using namespace std` into every file that includes them; the three .cc files and
 * their headers rely on it (vector, pair, isfinite, thread, ref), so it is here too.
 */
#ifndef REF_SOLVER_STANDIN_H
#define REF_SOLVER_STANDIN_H

#define CV_SHIM_LINALG
#define FRAME_H
#define KEYFRAME_H
#define MAPPOINT_H
#define ORBMATCHER_H
#define OPTIMIZER_H

#include <cmath>
#include <functional>
#include <map>
#include <thread>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>

using namespace std;

namespace ORB_SLAM2 {

class KeyFrame;

class MapPoint {
public:
    MapPoint(const cv::Mat &pos, bool bad = false) : mWorldPos(pos.clone()), mbBad(bad) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame *pKF)
    {
        std::map<KeyFrame *, int>::const_iterator it = index.find(pKF);
        return it == index.end() ? -1 : it->second;
    }

    std::map<KeyFrame *, int> index;         /* filled by the driver */

private:
    cv::Mat mWorldPos;
    bool mbBad;
};

class KeyFrame {
public:
    KeyFrame(const std::vector<cv::KeyPoint> &keys, const std::vector<float> &sigma2, const cv::Mat &K, const cv::Mat &Rcw, const cv::Mat &tcw)
        : mvKeysUn(keys), mvLevelSigma2(sigma2), mK(K), R(Rcw), t(tcw) {}
    cv::Mat GetRotation() { return R.clone(); }
    cv::Mat GetTranslation() { return t.clone(); }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }

    const std::vector<cv::KeyPoint> mvKeysUn;
    const std::vector<float> mvLevelSigma2;
    const cv::Mat mK;

    std::vector<MapPoint *> mvpMapPoints;    /* filled by the driver */

private:
    cv::Mat R, t;
};

class Frame {
public:
    cv::Mat mK;
    static float fx;
    static float fy;
    static float cx;
    static float cy;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint *> mvpMapPoints;
    vector<float> mvLevelSigma2;
};

}
#endif
