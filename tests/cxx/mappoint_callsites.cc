// mappoint_callsites.cc -- the reference's call expressions around MapPoint::ComputeDistinctiveDescriptors over
// host/MapPointDescriptors.h:
//     const vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();     src/LocalMapping.cc:142, :520
//     if(pMP) if(!pMP->isBad()) ... pMP->ComputeDistinctiveDescriptors();                        :147-155, :524-528
// with the descriptor calls of the loop replaced by ONE ComputeDistinctiveDescriptors(vpMapPointMatches) after it, and the
// reference's single-point method rewritten as a call of the batched one.
// Run with "compile-only" it exits at once.  Otherwise it reads a script on stdin, one command per line:
//     kfs <K>                                  the number of key frames (they live in one array, so the iteration order of
//                                              std::map<KeyFrame*, size_t> is the order of their ids 0..K-1)
//     kf <bad> <rows> <hex of rows x 32 bytes> the next key frame's mDescriptors
//     mp <bad> <hex of 32 bytes> <n> <kf> <idx> ...    a MapPoint of mpCurrentKeyFrame: its descriptor, then its observations
//     null                                     a NULL slot of mpCurrentKeyFrame
//     batch                                    the rewritten loop; prints "set <n>"
//     single <i>                               slot i's rewritten single-point method
//     dump                                     one line per slot: "null", or the hex of GetDescriptor()
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "MapPointDescriptors.h"

using namespace ORB_SLAM2;
using namespace std;

// src/MapPoint.cc:242, rewritten: the body is the batched call on a list of one
void MapPoint::ComputeDistinctiveDescriptors()
{
    ORB_SLAM2::ComputeDistinctiveDescriptors(vector<MapPoint*>(1, this));
}

static cv::Mat from_hex(const string &hex, int rows)
{
    cv::Mat m(rows, 32, CV_8U);
    for (int i = 0; i < rows * 32; i++) {
        unsigned v = 0;
        sscanf(hex.c_str() + 2 * i, "%2x", &v);
        m.ptr<unsigned char>(i / 32)[i % 32] = (unsigned char)v;
    }
    return m;
}

static int run()
{
    vector<KeyFrame> kfs;
    vector<unique_ptr<MapPoint>> mps;
    unique_ptr<KeyFrame> current;
    KeyFrame *mpCurrentKeyFrame = nullptr;
    string line;
    while (getline(cin, line)) {
        istringstream ss(line);
        string cmd;
        ss >> cmd;
        if (cmd == "kfs") {
            size_t K = 0;
            ss >> K;
            kfs.reserve(K);
            current.reset(new KeyFrame(K, cv::Mat(0, 32, CV_8U)));
            mpCurrentKeyFrame = current.get();
        } else if (cmd == "kf") {
            int bad = 0, rows = 0;
            string hex;
            ss >> bad >> rows >> hex;
            if (kfs.size() == kfs.capacity() || (int)hex.size() != rows * 64) return 2;
            kfs.emplace_back(kfs.size(), from_hex(hex, rows));
            if (bad) kfs.back().SetBadFlag();
        } else if (cmd == "mp") {
            int bad = 0, n = 0;
            string hex;
            ss >> bad >> hex >> n;
            if (hex.size() != 64 || !mpCurrentKeyFrame) return 2;
            mps.emplace_back(new MapPoint(mps.size(), from_hex(hex, 1)));
            MapPoint *pMP = mps.back().get();
            for (int i = 0; i < n; i++) {
                size_t kf = 0, idx = 0;
                ss >> kf >> idx;
                if (kf >= kfs.size() || (int)idx >= kfs[kf].mDescriptors.rows) return 2;
                pMP->AddObservation(&kfs[kf], idx);
            }
            if (bad) pMP->SetBadFlag();
            mpCurrentKeyFrame->AddMapPoint(pMP);
        } else if (cmd == "null") {
            mpCurrentKeyFrame->AddMapPoint(static_cast<MapPoint*>(NULL));
        } else if (cmd == "batch") {
            const vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
            for(size_t i=0; i<vpMapPointMatches.size(); i++)
            {
                MapPoint* pMP = vpMapPointMatches[i];
                if(pMP)
                {
                    if(!pMP->isBad())
                    {
                        // pMP->UpdateNormalAndDepth() stays here; pMP->ComputeDistinctiveDescriptors() left the loop
                    }
                }
            }
            string err;
            const int n = ComputeDistinctiveDescriptors(vpMapPointMatches, &err);
            if (n < 0) { fprintf(stderr, "ComputeDistinctiveDescriptors: %s\n", err.c_str()); return 3; }
            printf("set %d\n", n);
        } else if (cmd == "single") {
            size_t i = 0;
            ss >> i;
            const vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
            if (i >= vpMapPointMatches.size()) return 2;
            MapPoint* pMP = vpMapPointMatches[i];
            if(pMP)
                if(!pMP->isBad())
                    pMP->ComputeDistinctiveDescriptors();
        } else if (cmd == "dump") {
            const vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
            for (MapPoint *pMP : vpMapPointMatches) {
                if (!pMP) { printf("null\n"); continue; }
                const cv::Mat d = pMP->GetDescriptor();
                for (int k = 0; k < 32; k++) printf("%02x", d.ptr<unsigned char>()[k]);
                printf("\n");
            }
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    return run();
}
