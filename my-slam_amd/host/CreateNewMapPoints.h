// CreateNewMapPoints.h -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:209-454 of WChen09/My-SLAM) with every neighbour's
// SearchForTriangulation (:270) and per-match loop (:288-434) in ONE GPU call (orbm_create_new_map_points, include/orbm.h).
//
//     ORB_SLAM2::NewMapPointsBatch<KeyFrame> batch;
//     batch.Search(mpCurrentKeyFrame, vpKF2, vF12, bOnlyStereo);          // before the loop: the snapshot and the one call
//     batch.Neighbour(i, vMatchedIndices, status, x3D);                   // at neighbour i's turn, in place of :270 and :288-434
//
// Search() takes the neighbours that passed the baseline gate (:246-263), in the reference's order, with vF12[i] =
// ComputeF12(mpCurrentKeyFrame, vpKF2[i]); :241's CheckNewKeyFrames() exit, ComputeF12 and the object-graph work of :436-451 stay
// with the caller.
//
// The replay rule.  Neighbour(i, ...) returns exactly what SearchForTriangulation(pKF1, vpKF2[i], vF12[i], ...) followed by
// TriangulateMatches (NewMapPoints.h) would return at that moment: the pairs (idx1, idx2) the search found for neighbour i on the
// snapshot, in ascending idx1, kept only where pKF1->GetMapPoint(idx1) is NULL when Neighbour() is called -- it reads the live
// key frame, so a feature that an earlier neighbour's turn gave a MapPoint drops out (src/ORBmatcher.cc:699-703 would have
// skipped it) and one whose triangulation failed earlier stays -- each with its status byte (orbm_tri_status) and, for the
// accepted ones, its 3x1 CV_32F position.  Three premises make the snapshot's answer the sequential one:
//   1. mbCheckOrientation == false, as LocalMapping builds its matcher (ORBmatcher matcher(0.6,false), :217): the rotation
//      histogram of src/ORBmatcher.cc:764-810 would cull by which features took part, which the snapshot cannot know;
//   2. vbMatched2 is never set in this reference (:677, :725), so a feature's search depends on no other feature;
//   3. the neighbours are distinct key frames, and none of them is pKF1: the loop writes only to mpCurrentKeyFrame and to the
//      neighbour whose turn it is (:436-451), so before its own turn a neighbour is as the snapshot saw it.  Search() refuses a
//      list that names a key frame twice.
// Between Search() and the last Neighbour() nothing but the loop's own :436-451 may give MapPoints to the key frames involved.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "NewMapPoints.h"

namespace ORB_SLAM2 {
namespace orbm_detail {
// DBoW2::FeatureVector = std::map<NodeId, std::vector<unsigned int>> (ascending ids) appended to a CSR; off continues from its last entry
template <class FV> void AppendFeatureVector(const FV &fv, std::vector<int32_t> &node, std::vector<int32_t> &off, std::vector<int32_t> &idx)
{
    if (off.empty()) off.push_back(0);
    for (typename FV::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        node.push_back((int32_t)it->first);
        for (size_t k = 0; k < it->second.size(); k++) idx.push_back((int32_t)it->second[k]);
        off.push_back((int32_t)idx.size());
    }
}
template <class T> void Append(std::vector<T> &dst, const std::vector<T> &src) { dst.insert(dst.end(), src.begin(), src.end()); }
}  // namespace orbm_detail

template <class KeyFrameT>
class NewMapPointsBatch {
public:
    // The snapshot of pKF1 and of every neighbour, and the one GPU call.  false when the arguments are refused or the call failed
    // (text in *err); Neighbour() returns -1 until a Search() has succeeded.
    bool Search(KeyFrameT *pKF1, const std::vector<KeyFrameT *> &vpKF2, const std::vector<cv::Mat> &vF12, const bool bOnlyStereo,
                std::string *err = nullptr)
    {
        pKF1_ = nullptr; vpKF2_.clear();
        const int nviews = (int)vpKF2.size();
        if (vF12.size() != vpKF2.size()) return fail(err, "one F12 per neighbour: " + std::to_string(vF12.size()) + " for " + std::to_string(nviews));
        for (int i = 0; i < nviews; i++) {
            if (!vpKF2[i] || vpKF2[i] == pKF1) return fail(err, "neighbour " + std::to_string(i) + " is NULL or the current key frame");
            for (int j = 0; j < i; j++)
                if (vpKF2[j] == vpKF2[i]) return fail(err, "neighbours " + std::to_string(j) + " and " + std::to_string(i) + " are the same key frame");
        }
        n1_ = (int)pKF1->mvKeysUn.size();
        matches12_.assign((size_t)nviews * n1_, -1); status_.assign((size_t)nviews * n1_, (unsigned char)ORBM_TRI_NO_MATCH);
        x3d_.assign((size_t)3 * nviews * n1_, 0.f); nmatches_.assign(nviews, 0);
        if (nviews > 0 && n1_ > 0) {
            orbm_detail::Lease lease;
            if (!lease.ready(err)) return false;
            orbm_detail::Scratch &S = *lease.h.s;
            orbm_camera cam1;
            std::vector<orbm_camera> cams2(nviews);
            if (!orbm_detail::FillCamera(pKF1, cam1, err)) return false;
            orbm_detail::FillFeatures(pKF1, S.kp_, S.f0_, S.f1_, S.f2_);
            S.u8_.assign(n1_, 0);
            for (int i = 0; i < n1_; i++) S.u8_[i] = pKF1->GetMapPoint(i) ? 1 : 0;
            S.desc_.resize((size_t)n1_ * 32);
            for (int i = 0; i < n1_; i++) memcpy(&S.desc_[(size_t)i * 32], pKF1->mDescriptors.template ptr<unsigned char>(i), 32);
            S.i0_.clear(); S.i1_.clear(); S.i2_.clear();
            orbm_detail::AppendFeatureVector(pKF1->mFeatVec, S.i0_, S.i1_, S.i2_);
            // the views, concatenated
            std::vector<orbx_keypoint> kp;
            std::vector<float> xy, ur, depth;
            S.kp2_.clear(); S.f3_.clear(); S.f4_.clear(); S.f5_.clear(); S.v8_.clear(); S.desc2_.clear();
            S.j0_.clear(); S.j1_.clear(); S.j2_.clear(); S.g0_.clear();
            std::vector<int32_t> off2(1, 0), fvo(1, 0);
            for (int v = 0; v < nviews; v++) {
                KeyFrameT *pKF2 = vpKF2[v];
                if (!orbm_detail::FillCamera(pKF2, cams2[v], err)) return false;
                orbm_detail::FillFeatures(pKF2, kp, xy, ur, depth);
                const size_t n2 = kp.size();
                orbm_detail::Append(S.kp2_, kp); orbm_detail::Append(S.f3_, xy); orbm_detail::Append(S.f4_, ur); orbm_detail::Append(S.f5_, depth);
                for (size_t i = 0; i < n2; i++) {
                    S.v8_.push_back(pKF2->GetMapPoint(i) ? 1 : 0);
                    const unsigned char *d = pKF2->mDescriptors.template ptr<unsigned char>((int)i);
                    S.desc2_.insert(S.desc2_.end(), d, d + 32);
                }
                orbm_detail::AppendFeatureVector(pKF2->mFeatVec, S.j0_, S.j1_, S.j2_);
                off2.push_back((int32_t)S.kp2_.size()); fvo.push_back((int32_t)S.j0_.size());
                if (vF12[v].rows != 3 || vF12[v].cols != 3) return fail(err, "F12 of neighbour " + std::to_string(v) + " is not 3x3");
                for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) S.g0_.push_back(vF12[v].template at<float>(r, c));
            }
            if (orbm_create_new_map_points(lease.h.m, &cam1, S.kp_.data(), S.f0_.data(), S.f1_.data(), S.f2_.data(), S.desc_.data(), n1_, S.u8_.data(),
                                           S.i0_.data(), S.i1_.data(), S.i2_.data(), (int)S.i0_.size(), cams2.data(), S.g0_.data(), nviews, off2.data(),
                                           S.kp2_.data(), S.f3_.data(), S.f4_.data(), S.f5_.data(), S.desc2_.data(), S.v8_.data(), fvo.data(), S.j0_.data(),
                                           S.j1_.data(), S.j2_.data(), bOnlyStereo ? 1 : 0, matches12_.data(), status_.data(), x3d_.data(),
                                           nmatches_.data()) != ORBX_OK)
                return fail(err, orbm_last_error());
        }
        pKF1_ = pKF1; vpKF2_ = vpKF2;
        return true;
    }

    // Neighbour i's turn (the replay rule above).  Returns the number of accepted pairs among those returned, or -1 without a
    // successful Search() or for an i outside its list; the three vectors are empty then.
    int Neighbour(size_t i, std::vector<std::pair<size_t, size_t> > &vMatchedIndices, std::vector<unsigned char> &status, std::vector<cv::Mat> &x3D)
    {
        vMatchedIndices.clear(); status.clear(); x3D.clear();
        if (!pKF1_ || i >= vpKF2_.size()) return -1;
        int accepted = 0;
        for (int idx1 = 0; idx1 < n1_; idx1++) {
            const size_t slot = i * (size_t)n1_ + idx1;
            if (matches12_[slot] < 0 || pKF1_->GetMapPoint(idx1)) continue;
            vMatchedIndices.push_back(std::make_pair((size_t)idx1, (size_t)matches12_[slot]));
            status.push_back(status_[slot]);
            cv::Mat p;
            if (status_[slot] <= ORBM_TRI_STEREO2) {
                p = cv::Mat(3, 1, CV_32F);
                for (int r = 0; r < 3; r++) p.template at<float>(r) = x3d_[3 * slot + r];
                accepted++;
            }
            x3D.push_back(p);
        }
        return accepted;
    }

    size_t Neighbours() const { return vpKF2_.size(); }
    // what SearchForTriangulation would have returned for neighbour i on the snapshot (before the live filter)
    int SnapshotMatches(size_t i) const { return i < nmatches_.size() ? nmatches_[i] : -1; }

private:
    static bool fail(std::string *err, const std::string &text) { if (err) *err = text; return false; }
    KeyFrameT *pKF1_ = nullptr;
    std::vector<KeyFrameT *> vpKF2_;
    int n1_ = 0;
    std::vector<int32_t> matches12_, nmatches_;
    std::vector<unsigned char> status_;
    std::vector<float> x3d_;
};

}  // namespace ORB_SLAM2
