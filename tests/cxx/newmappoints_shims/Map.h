// Map.h -- repo-authored minimal Map: AddMapPoint (src/Map.cc:37-41) in insertion order, which is what the test compares.
#pragma once
#include <vector>
#include "MapPoint.h"

namespace ORB_SLAM2 {
class Map {
public:
    void AddMapPoint(MapPoint *pMP) { mvpMapPoints.push_back(pMP); }
    std::vector<MapPoint *> mvpMapPoints;
};
}  // namespace ORB_SLAM2
