// KeyFrameDatabase.cc -- the adapter's method bodies; replaces the reference's src/KeyFrameDatabase.cc in the build (see
// KeyFrameDatabase.h).  A query gathers mBowVec, mnId and GetConnectedKeyFrames(), calls orbk_query_begin, reads
// GetBestCovisibilityKeyFrames(10) of the scored keyframes (only those, only then, as the reference does), calls
// orbk_query_end and maps the candidate ids back to KeyFrame*.  A library error (no GPU, out of device memory) throws
// std::runtime_error: there is no CPU path.
#include "KeyFrameDatabase.h"

#include "KeyFrame.h"

#include <stdexcept>
#include <string>

namespace ORB_SLAM2 {

namespace {
void check(int rc)
{
    if (rc != ORBX_OK) throw std::runtime_error(std::string("KeyFrameDatabase: ") + orbk_last_error());
}

template <class BowVector>
void gather(const BowVector &v, std::vector<int32_t> &ids, std::vector<double> &vals)
{
    for (typename BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
        ids.push_back((int32_t)it->first);
        vals.push_back((double)it->second);
    }
}
}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc, int device)
{
    check(orbk_create(&mpDB, device, (int)voc.size(), (int)voc.getScoringType(), 1024, 1 << 20));
}

KeyFrameDatabase::~KeyFrameDatabase() { orbk_destroy(mpDB); }

void KeyFrameDatabase::add(KeyFrame *pKF)
{
    std::vector<int32_t> ids;
    std::vector<double> vals;
    gather(pKF->mBowVec, ids, vals);
    {
        std::lock_guard<std::mutex> lk(mMutex);
        mKeyFrames[(uint64_t)pKF->mnId] = pKF;
    }
    check(orbk_add(mpDB, (uint64_t)pKF->mnId, ids.data(), vals.data(), (int)ids.size()));
}

void KeyFrameDatabase::erase(KeyFrame *pKF) { check(orbk_erase(mpDB, (uint64_t)pKF->mnId)); }

void KeyFrameDatabase::clear() { check(orbk_clear(mpDB)); }

std::vector<KeyFrame *> KeyFrameDatabase::DetectLoopCandidates(KeyFrame *pKF, float minScore)
{
    std::set<KeyFrame *> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::vector<uint64_t> conn;
    for (KeyFrame *k : spConnectedKeyFrames) conn.push_back((uint64_t)k->mnId);
    std::vector<int32_t> ids;
    std::vector<double> vals;
    gather(pKF->mBowVec, ids, vals);
    return Query(ORBK_LOOP, (uint64_t)pKF->mnId, ids, vals, conn, minScore);
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)
{
    std::vector<int32_t> ids;
    std::vector<double> vals;
    gather(F->mBowVec, ids, vals);
    return Query(ORBK_RELOC, (uint64_t)F->mnId, ids, vals, std::vector<uint64_t>(), 0.0f);
}

std::vector<KeyFrame *> KeyFrameDatabase::Query(int kind, uint64_t qid, const std::vector<int32_t> &ids, const std::vector<double> &vals,
                                                const std::vector<uint64_t> &conn, float minScore)
{
    int n = orbk_size(mpDB) + 1, rc;
    std::vector<uint64_t> scored;
    std::vector<float> si;
    do {            // another thread may add keyframes meanwhile; a capacity error changes no state
        scored.resize(n); si.resize(n);
        rc = orbk_query_begin(mpDB, kind, qid, ids.data(), vals.data(), (int)ids.size(), conn.data(), (int)conn.size(), minScore,
                              scored.data(), si.data(), (int)scored.size(), &n);
    } while (rc == ORBX_E_CAPACITY);
    check(rc);
    // id -> KeyFrame*: the scored keyframes were in the database at orbk_query_begin; a neighbour can be any keyframe
    std::unordered_map<uint64_t, KeyFrame *> ptr;
    std::vector<int32_t> off(1, 0);
    std::vector<uint64_t> nb;
    {
        std::lock_guard<std::mutex> lk(mMutex);
        for (int i = 0; i < n; i++) ptr[scored[i]] = mKeyFrames.at(scored[i]);
    }
    for (int i = 0; i < n; i++) {
        std::vector<KeyFrame *> vpNeighs = ptr[scored[i]]->GetBestCovisibilityKeyFrames(10);
        for (KeyFrame *k : vpNeighs) { nb.push_back((uint64_t)k->mnId); ptr[(uint64_t)k->mnId] = k; }
        off.push_back((int32_t)nb.size());
    }
    std::vector<uint64_t> cand(n + 1);
    int nc = 0;
    check(orbk_query_end(mpDB, kind, off.data(), nb.data(), cand.data(), (int)cand.size(), &nc));
    std::vector<KeyFrame *> out;
    out.reserve(nc);
    for (int i = 0; i < nc; i++) out.push_back(ptr.at(cand[i]));
    return out;
}

}  // namespace ORB_SLAM2
