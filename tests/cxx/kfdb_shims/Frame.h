// Frame.h -- repo-authored minimal Frame for the KeyFrameDatabase adapter tests (member names as in the reference's
// include/Frame.h: the id and the BowVector DetectRelocalizationCandidates reads).  Includes as include/Frame.h:26-30.
#pragma once
#include "MapPoint.h"
#include "ORBVocabulary.h"
#include "KeyFrame.h"

namespace ORB_SLAM2 {
class MapPoint;
class KeyFrame;

class Frame {
public:
    Frame() : mnId(0) {}
    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
};
}
