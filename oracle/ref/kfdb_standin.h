/*
 * kfdb_standin.h -- force-included (-include) in front of the reference's own src/KeyFrameDatabase.cc, which is compiled
 * unmodified and in place for oracle/_ref/ref_kfdb.  TEST INFRASTRUCTURE ONLY.
 *
 * The reference's include/KeyFrameDatabase.h includes "KeyFrame.h" and "Frame.h"; both drag in OpenCV, Eigen, g2o and the
 * rest of the system.  This header predefines their include guards (KEYFRAME_H, FRAME_H), so the real headers are found
 * and their bodies skipped, and declares stand-in ORB_SLAM2::KeyFrame and ORB_SLAM2::Frame with exactly the members
 * src/KeyFrameDatabase.cc touches, under the reference's names and types (include/KeyFrame.h:65-67, :124, :144-149, :170;
 * include/Frame.h:146, :168).  The reference's include/ORBVocabulary.h and Thirdparty/DBoW2 are the real ones.
 *
 * Two conventions, both the driver's and not the reference's:
 *   - The reference's KeyFrame constructor (src/KeyFrame.cc:34) sets mnLoopQuery, mnLoopWords, mnRelocQuery and
 *     mnRelocWords to 0 and never initialises mLoopScore / mRelocScore, so reading one before its first write is undefined
 *     there.  The stand-in sets both to 0, as include/orbk.h documents for the library and tests/kfdb_oracle.py does.
 *   - GetConnectedKeyFrames() and GetBestCovisibilityKeyFrames(N) return what the driver's script filled in: a set, and the
 *     first N of an ordered list (src/KeyFrame.cc returns the first N of mvpOrderedConnectedKeyFrames in the same way).
 *     GetBestCovisibilityKeyFrames is defined in ref_kfdb.cc, where it also logs the call.
 */
#ifndef REF_KFDB_STANDIN_H
#define REF_KFDB_STANDIN_H

#define KEYFRAME_H
#define FRAME_H

#include <list>
#include <set>
#include <vector>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

using namespace std;       /* include/KeyFrameDatabase.h:66 writes list<KeyFrame*> unqualified; the real headers bring this in */

namespace ORB_SLAM2 {

class KeyFrame {
public:
    explicit KeyFrame(long unsigned int id)
        : mnId(id), mnLoopQuery(0), mnLoopWords(0), mLoopScore(0.0f), mnRelocQuery(0), mnRelocWords(0), mRelocScore(0.0f) {}

    std::set<KeyFrame *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N);      /* ref_kfdb.cc */

    long unsigned int mnId;
    long unsigned int mnLoopQuery;
    int mnLoopWords;
    float mLoopScore;
    long unsigned int mnRelocQuery;
    int mnRelocWords;
    float mRelocScore;
    DBoW2::BowVector mBowVec;

    std::set<KeyFrame *> connected;          /* filled by the driver ("conn") */
    std::vector<KeyFrame *> covisible;       /* filled by the driver ("covis"), best first */
};

class Frame {
public:
    Frame() : mnId(0) {}
    DBoW2::BowVector mBowVec;
    long unsigned int mnId;
};

}
#endif
