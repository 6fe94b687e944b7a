// kfdb_include_order.cc -- host/KeyFrameDatabase.h under the reference's circular include graph (tests/cxx/kfdb_shims/):
// a translation unit whose first project include is KeyFrame.h (-DFIRST_KEYFRAME, as src/KeyFrame.cc), Frame.h
// (-DFIRST_FRAME, as src/Frame.cc) or MapPoint.h (-DFIRST_MAPPOINT, as src/MapPoint.cc) must compile the adapter's call
// expressions.  Compiled with -fsyntax-only by tests/test_kfdb_cpu.py.
#if defined(FIRST_KEYFRAME)
#include "KeyFrame.h"
#elif defined(FIRST_FRAME)
#include "Frame.h"
#elif defined(FIRST_MAPPOINT)
#include "MapPoint.h"
#else
#error "define FIRST_KEYFRAME, FIRST_FRAME or FIRST_MAPPOINT"
#endif
#include "KeyFrameDatabase.h"

namespace ORB_SLAM2 {
size_t callsites(KeyFrameDatabase *mpKeyFrameDB, Frame &mCurrentFrame, KeyFrame *mpCurrentKF, KeyFrame *pKF, float minScore)
{
    mpKeyFrameDB->add(pKF);
    std::vector<KeyFrame *> a = mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame);
    std::vector<KeyFrame *> b = mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore);
    mpKeyFrameDB->erase(pKF);
    mpKeyFrameDB->clear();
    return a.size() + b.size();
}
}
