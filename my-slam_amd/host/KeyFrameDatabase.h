// KeyFrameDatabase.h -- drop-in replacement for the reference's include/KeyFrameDatabase.h (WChen09/My-SLAM); the method
// bodies are in KeyFrameDatabase.cc beside it, which replaces src/KeyFrameDatabase.cc in the build.
//
// Same namespace, class name, constructor and public methods as include/KeyFrameDatabase.h:44-58, so the call sites
// src/Tracking.cc:1355 (DetectRelocalizationCandidates), src/LoopClosing.cc:142 (DetectLoopCandidates) and the add / erase /
// clear calls of LocalMapping, KeyFrame::SetBadFlag and System::Reset compile unchanged:
//     KeyFrameDatabase(const ORBVocabulary &voc)                                   :44
//     void add(KeyFrame* pKF) / void erase(KeyFrame* pKF) / void clear()          :46-50
//     std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore)  :53
//     std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)             :56
// Like the reference header it includes "KeyFrame.h", "Frame.h" and "ORBVocabulary.h" and only declares: the reference's
// include graph is circular (KeyFrame.h includes Frame.h and this header before it defines KeyFrame), so KeyFrame and Frame
// may still be incomplete here.  In an ORB-SLAM2 tree those headers are the tree's own; this repo's tests supply minimal
// classes with the same member names and the same include order (tests/cxx/kfdb_shims/).
#pragma once
#include <cstdint>
#include <list>
#include <mutex>
#include <set>
#include <unordered_map>
#include <vector>

#include "../../include/orbk.h"

#include "KeyFrame.h"
#include "Frame.h"
#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary &voc, int device = 0);
    ~KeyFrameDatabase();
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    void add(KeyFrame *pKF);

    void erase(KeyFrame *pKF);

    void clear();

    // Loop Detection
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);

    // Relocalization
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);

protected:
    std::vector<KeyFrame *> Query(int kind, uint64_t qid, const std::vector<int32_t> &ids, const std::vector<double> &vals,
                                  const std::vector<uint64_t> &conn, float minScore);

    // The GPU handle of include/orbk.h: the BowVectors live in its device arena, and so does the reference's per-keyframe
    // query state (mnLoopQuery .. mRelocScore); no KeyFrame member is written.
    orbk_database *mpDB = nullptr;
    // every keyframe ever added, by mnId (a re-add replaces the entry).  Never cleared: an erase or clear() on another
    // thread between the two phases of a query must not orphan a scored id, and ORB-SLAM2 keeps KeyFrame objects alive
    // until System::Reset, whose re-added keyframes replace their entries.
    std::unordered_map<uint64_t, KeyFrame *> mKeyFrames;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2
