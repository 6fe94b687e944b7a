// LoopClosing.h -- repo-authored: LoopClosing::KeyFrameAndPose (include/LoopClosing.h:50-51) over a stand-in g2o::Sim3 that holds
// the eight numbers of g2o::Sim3::operator[] (qx qy qz qw tx ty tz s) and offers nothing else: the adapter may read a Sim3 through
// operator[] only.
#pragma once
#include <map>
#include "KeyFrame.h"

namespace g2o {
struct Sim3 {
    double v[8] = {0, 0, 0, 1, 0, 0, 0, 1};
    double operator[](int i) const { return v[i]; }
    double &operator[](int i) { return v[i]; }
};
}   // namespace g2o

namespace ORB_SLAM2 {
class LoopClosing {
public:
    typedef std::map<KeyFrame *, g2o::Sim3, std::less<KeyFrame *>> KeyFrameAndPose;
};
}   // namespace ORB_SLAM2
