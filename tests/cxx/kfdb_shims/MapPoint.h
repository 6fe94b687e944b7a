// MapPoint.h -- repo-authored stand-in that only reproduces the reference's include order (include/MapPoint.h:24-25:
// KeyFrame.h, then Frame.h) for the KeyFrameDatabase adapter tests; the adapter reads no MapPoint member.
#pragma once
#include "KeyFrame.h"
#include "Frame.h"

namespace ORB_SLAM2 {
class KeyFrame;
class Frame;

class MapPoint {
};
}
