/*
 * ref_kfdb.cc -- driver that runs the reference's own src/KeyFrameDatabase.cc (compiled unmodified and in place, behind the
 * stand-in KeyFrame / Frame of kfdb_standin.h, with the reference's include/ORBVocabulary.h and Thirdparty/DBoW2) on a
 * script, for tests/test_reference_pin_kfdb_*.py.
 *
 *   ref_kfdb < SCRIPT > OUTPUT
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable: it keeps the reference's code out of the test process.
 *
 * The script is the language of tests/cxx/kfdb_callsites.cc, one command per line, plus "dump":
 *     words <N>                            the vocabulary size; first, once
 *     kf <id> <n> <word> <value> ...       a KeyFrame with that BowVector (values as %.17g)
 *     covis <id> <k> <id> ...              its covisibility order (GetBestCovisibilityKeyFrames takes the first N of it)
 *     conn <id> <k> <id> ...               its connected keyframes
 *     add <id> | erase <id> | clear
 *     reloc <frame id> <n> <word> <value> ...
 *     loop <id> <minScore>
 *     dump
 * Output, per query two lines and per dump one line per keyframe known so far (ascending id) and an end line:
 *     C <id> ...                           the candidates, in the reference's order
 *     L <id>:<bits> ...                    lScoreAndMatch: ids and the float score's bits in hex (see below)
 *     D <id> <mnLoopQuery> <mnLoopWords> <mLoopScore bits> <mnRelocQuery> <mnRelocWords> <mRelocScore bits>
 *     E
 *
 * The call log.  The reference calls pKFi->GetBestCovisibilityKeyFrames(10) once per entry of lScoreAndMatch, in list
 * order (src/KeyFrameDatabase.cc:148-151, :262-265), and by then it has written that entry's score into pKFi->mLoopScore
 * (:135) or mRelocScore (:250).  That function is the driver's, so it records (this->mnId, the bits of that score) at
 * every call: the record of one query is the reference's own lScoreAndMatch, read without editing the reference.
 *
 * The vocabulary.  KeyFrameDatabase needs an ORBVocabulary only for size() (the length of the inverted file) and for
 * score().  The driver uses a probe subclass that sizes the protected word table to N null entries (size() returns
 * m_words.size() and nothing here dereferences a word); the default constructor already makes the L1 scoring object
 * (TemplatedVocabulary.h: TF_IDF, L1_NORM).  A word id >= N would index past mvInvertedFile in the reference; the driver
 * refuses it (status 2), and no test case holds one.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "KeyFrameDatabase.h"          // the reference's; KeyFrame.h and Frame.h in it are skipped by kfdb_standin.h

using namespace ORB_SLAM2;

class ProbeVocabulary : public ORBVocabulary {
public:
    explicit ProbeVocabulary(unsigned int nwords) { m_words.resize(nwords, nullptr); }
};

static bool g_loop = false;
static std::vector<std::pair<unsigned long, uint32_t>> g_log;

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

std::vector<KeyFrame *> KeyFrame::GetBestCovisibilityKeyFrames(const int &N)
{
    g_log.push_back(std::make_pair(mnId, bits(g_loop ? mLoopScore : mRelocScore)));
    if ((int)covisible.size() < N) return covisible;
    return std::vector<KeyFrame *>(covisible.begin(), covisible.begin() + N);
}

static void fail(const char *m) { std::fprintf(stderr, "ref_kfdb: %s\n", m); std::exit(2); }

static void read_bow(std::istringstream &ss, DBoW2::BowVector &v, unsigned int nwords)
{
    int n = 0;
    ss >> n;
    v.clear();
    for (int i = 0; i < n; i++) {
        unsigned int w = 0;
        std::string val;
        ss >> w >> val;
        if (!ss) fail("truncated BowVector");
        if (w >= nwords) fail("word id beyond the vocabulary");
        v[w] = std::strtod(val.c_str(), nullptr);
    }
}

int main()
{
    std::map<unsigned long, std::unique_ptr<KeyFrame>> kfs;
    auto get = [&](unsigned long id) -> KeyFrame * {
        std::unique_ptr<KeyFrame> &p = kfs[id];
        if (!p) p.reset(new KeyFrame(id));
        return p.get();
    };
    std::unique_ptr<ProbeVocabulary> voc;
    std::unique_ptr<KeyFrameDatabase> db;
    unsigned int nwords = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string cmd;
        ss >> cmd;
        if (cmd.empty()) continue;
        if (cmd == "words") {
            if (db) fail("words given twice");
            ss >> nwords;
            voc.reset(new ProbeVocabulary(nwords));
            if (voc->size() != nwords) fail("vocabulary size");
            db.reset(new KeyFrameDatabase(*voc));
            continue;
        }
        if (!db) fail("no words command");
        if (cmd == "kf") {
            unsigned long id = 0;
            ss >> id;
            read_bow(ss, get(id)->mBowVec, nwords);
        } else if (cmd == "covis" || cmd == "conn") {
            unsigned long id = 0;
            int k = 0;
            ss >> id >> k;
            KeyFrame *pKF = get(id);
            std::vector<KeyFrame *> v;
            for (int i = 0; i < k; i++) {
                unsigned long j = 0;
                ss >> j;
                v.push_back(get(j));
            }
            if (!ss) fail("truncated id list");
            if (cmd == "covis") pKF->covisible = v;
            else pKF->connected = std::set<KeyFrame *>(v.begin(), v.end());
        } else if (cmd == "add" || cmd == "erase") {
            unsigned long id = 0;
            ss >> id;
            if (cmd == "add") db->add(get(id));
            else db->erase(get(id));
        } else if (cmd == "clear") {
            db->clear();
        } else if (cmd == "reloc" || cmd == "loop") {
            std::vector<KeyFrame *> cand;
            g_log.clear();
            g_loop = cmd == "loop";
            if (g_loop) {
                unsigned long id = 0;
                std::string ms;
                ss >> id >> ms;
                cand = db->DetectLoopCandidates(get(id), std::strtof(ms.c_str(), nullptr));
            } else {
                Frame F;
                ss >> F.mnId;
                read_bow(ss, F.mBowVec, nwords);
                cand = db->DetectRelocalizationCandidates(&F);
            }
            std::printf("C");
            for (KeyFrame *k : cand) std::printf(" %lu", k->mnId);
            std::printf("\nL");
            for (const auto &e : g_log) std::printf(" %lu:%08x", e.first, e.second);
            std::printf("\n");
        } else if (cmd == "dump") {
            for (const auto &kv : kfs) {
                const KeyFrame &k = *kv.second;
                std::printf("D %lu %lu %d %08x %lu %d %08x\n", k.mnId, k.mnLoopQuery, k.mnLoopWords, bits(k.mLoopScore),
                            k.mnRelocQuery, k.mnRelocWords, bits(k.mRelocScore));
            }
            std::printf("E\n");
        } else {
            fail("unknown command");
        }
    }
    return std::fflush(stdout) == 0 ? 0 : 2;
}
