// kfdb_callsites.cc -- the reference's KeyFrameDatabase call expressions over host/KeyFrameDatabase.h (+ .cc):
//     mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame)        src/Tracking.cc:1355
//     mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore)          src/LoopClosing.cc:142
//     mpKeyFrameDB->add(pKF), ->erase(pKF), ->clear()
// Run with "compile-only" it exits at once.  Otherwise it reads a script on stdin, one command per line, and prints the
// candidate mnIds of every query on a line of its own:
//     kf <id> <n> <word> <value> ...       a KeyFrame with that BowVector (values as %.17g)
//     covis <id> <k> <id> ...              its covisibility order (GetBestCovisibilityKeyFrames takes the first 10)
//     conn <id> <k> <id> ...               its connected keyframes
//     add <id> | erase <id> | clear
//     reloc <frame id> <n> <word> <value> ...
//     loop <id> <minScore>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

#include "KeyFrame.h"                  // first, as in src/KeyFrame.cc: KeyFrameDatabase.h is parsed before KeyFrame is complete
#include "KeyFrameDatabase.h"

using namespace ORB_SLAM2;

static void read_bow(std::istringstream &ss, DBoW2::BowVector &v)
{
    int n = 0;
    ss >> n;
    v.clear();
    for (int i = 0; i < n; i++) {
        unsigned int w = 0;
        std::string val;
        ss >> w >> val;
        v[w] = strtod(val.c_str(), nullptr);
    }
}

static int run()
{
    std::map<unsigned long, std::unique_ptr<KeyFrame>> kfs;
    auto get = [&](unsigned long id) -> KeyFrame * {
        std::unique_ptr<KeyFrame> &p = kfs[id];
        if (!p) p.reset(new KeyFrame(id));
        return p.get();
    };
    std::unique_ptr<ORBVocabulary> voc;
    std::unique_ptr<KeyFrameDatabase> db;
    KeyFrameDatabase *mpKeyFrameDB = nullptr;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string cmd;
        ss >> cmd;
        if (cmd == "words") {
            unsigned int nwords = 0;
            ss >> nwords;
            voc.reset(new ORBVocabulary(nwords, DBoW2::L1_NORM));
            db.reset(new KeyFrameDatabase(*voc));
            mpKeyFrameDB = db.get();
        } else if (cmd == "kf") {
            unsigned long id = 0;
            ss >> id;
            read_bow(ss, get(id)->mBowVec);
        } else if (cmd == "covis" || cmd == "conn") {
            unsigned long id = 0;
            int k = 0;
            ss >> id >> k;
            KeyFrame *pKF = get(id);
            if (cmd == "conn") pKF->mConnectedKeyFrameWeights.clear();
            std::vector<KeyFrame *> v;
            for (int i = 0; i < k; i++) {
                unsigned long j = 0;
                ss >> j;
                v.push_back(get(j));
            }
            if (cmd == "covis") pKF->mvpOrderedConnectedKeyFrames = v;
            else for (KeyFrame *c : v) pKF->mConnectedKeyFrameWeights[c] = 1;
        } else if (cmd == "add" || cmd == "erase") {
            unsigned long id = 0;
            ss >> id;
            KeyFrame *pKF = get(id);
            if (cmd == "add") mpKeyFrameDB->add(pKF);
            else mpKeyFrameDB->erase(pKF);
        } else if (cmd == "clear") {
            mpKeyFrameDB->clear();
        } else if (cmd == "reloc" || cmd == "loop") {
            std::vector<KeyFrame *> vpCandidateKFs;
            if (cmd == "reloc") {
                Frame mCurrentFrame;
                ss >> mCurrentFrame.mnId;
                read_bow(ss, mCurrentFrame.mBowVec);
                vpCandidateKFs = mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame);
            } else {
                unsigned long id = 0;
                std::string ms;
                ss >> id >> ms;
                KeyFrame *mpCurrentKF = get(id);
                const float minScore = strtof(ms.c_str(), nullptr);
                vpCandidateKFs = mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore);
            }
            for (size_t i = 0; i < vpCandidateKFs.size(); i++) printf(i ? " %lu" : "%lu", vpCandidateKFs[i]->mnId);
            printf("\n");
        } else if (!cmd.empty()) {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    try {
        return run();
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
