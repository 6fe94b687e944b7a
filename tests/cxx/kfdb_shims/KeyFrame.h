// KeyFrame.h -- repo-authored minimal KeyFrame for the KeyFrameDatabase adapter tests (member names and types as in the
// reference's include/KeyFrame.h; only what ORB_SLAM2::KeyFrameDatabase reads, bodies written here).  The covisibility order
// is set by the test: GetBestCovisibilityKeyFrames(N) returns the first N of it, as src/KeyFrame.cc does.  The includes
// are the reference's (include/KeyFrame.h:24-30): MapPoint.h, Frame.h and KeyFrameDatabase.h come before the class, and
// MapPoint.h and Frame.h include this header in turn, so whichever of them a translation unit includes first, the others
// are parsed while KeyFrame is still incomplete.
#pragma once
#include <map>
#include <set>
#include <vector>
#include "MapPoint.h"
#include "ORBVocabulary.h"
#include "Frame.h"
#include "KeyFrameDatabase.h"

namespace ORB_SLAM2 {
class MapPoint;
class Frame;
class KeyFrameDatabase;

class KeyFrame {
public:
    explicit KeyFrame(long unsigned int id) : mnId(id) {}

    std::set<KeyFrame *> GetConnectedKeyFrames()
    {
        std::set<KeyFrame *> s;
        for (auto &kv : mConnectedKeyFrameWeights) s.insert(kv.first);
        return s;
    }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }

    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
};
}
