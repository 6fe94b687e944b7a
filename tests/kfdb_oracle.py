"""Restatement of the reference's src/KeyFrameDatabase.cc (WChen09/My-SLAM) in Python: the test oracle of include/orbk.h.

It keeps the reference's own data structures: an inverted file of per-word lists in push_back order, keyframe objects that
carry the six query fields of KeyFrame (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore;
constructor values from src/KeyFrame.cc:34, the never-initialised scores read as 0.0), and the reference's loops in the
reference's order.  Float steps are np.float32: si, maxCommonWords*0.8f, accScore += and 0.75f*bestAccScore.  The L1
score is DBoW2's (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): double terms summed in ascending common-word order.
"""
import numpy as np

F32 = np.float32


class KF:
    """The query fields of one KeyFrame; it outlives its membership in the database (erase / clear / re-add)."""

    def __init__(self, kf_id):
        self.mnId = kf_id
        self.mnLoopQuery = 0      # src/KeyFrame.cc:34
        self.mnLoopWords = 0
        self.mLoopScore = F32(0.0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0.0)
        self.bow = (np.zeros(0, np.int32), np.zeros(0, np.float64))


def score_l1(bow1, bow2):
    """L1Scoring::score (ScoringObject.cpp:23-68): the terms of the common words, in ascending word order, in double."""
    ids1, v1 = bow1
    ids2, v2 = bow2
    score = 0.0
    i = j = 0
    while i < len(ids1) and j < len(ids2):
        if ids1[i] == ids2[j]:
            vi, wi = float(v1[i]), float(v2[j])
            score += abs(vi - wi) - abs(vi) - abs(wi)        # :40
            i += 1
            j += 1
        elif ids1[i] < ids2[j]:
            i += 1
        else:
            j += 1
    return -score / 2.0                                       # :64


class KeyFrameDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.inv = {}                                         # word -> list of KF (mvInvertedFile, :36)
        self.kfs = {}                                         # id -> KF: the caller's keyframe objects

    def kf(self, kf_id):
        if kf_id not in self.kfs:
            self.kfs[kf_id] = KF(kf_id)
        return self.kfs[kf_id]

    def add(self, kf_id, bow):                               # :40-46
        k = self.kf(kf_id)
        k.bow = (np.asarray(bow[0], np.int32), np.asarray(bow[1], np.float64))
        for w in k.bow[0]:
            self.inv.setdefault(int(w), []).append(k)

    def erase(self, kf_id):                                  # :48-67
        k = self.kfs.get(kf_id)
        if k is None:
            return
        for w in k.bow[0]:
            lst = self.inv.get(int(w), [])
            for i, x in enumerate(lst):
                if x is k:
                    del lst[i]
                    break

    def clear(self):                                         # :69-73
        self.inv = {}

    def _sharing(self, bow, query_id, loop, connected):
        """:83-105 (loop) and :203-222 (relocalisation)."""
        out = []
        for w in bow[0]:
            for k in self.inv.get(int(w), []):
                if loop:
                    if k.mnLoopQuery != query_id:
                        k.mnLoopWords = 0
                        if k.mnId not in connected:
                            k.mnLoopQuery = query_id
                            out.append(k)
                    k.mnLoopWords += 1
                else:
                    if k.mnRelocQuery != query_id:
                        k.mnRelocWords = 0
                        k.mnRelocQuery = query_id
                        out.append(k)
                    k.mnRelocWords += 1
        return out

    def query_begin(self, loop, query_id, bow, connected=(), min_score=0.0):
        """Up to lScoreAndMatch: returns [(si, id)] and the minCommonWords the accumulation uses."""
        bow = (np.asarray(bow[0], np.int32), np.asarray(bow[1], np.float64))
        connected = set(connected)
        sharing = self._sharing(bow, query_id, loop, connected)
        if not sharing:                                       # :107-108 / :224-225
            return [], 0
        words = (lambda k: k.mnLoopWords) if loop else (lambda k: k.mnRelocWords)
        max_common = 0                                        # :112-118 / :229-233
        for k in sharing:
            if words(k) > max_common:
                max_common = words(k)
        min_common = int(F32(max_common) * F32(0.8))          # :120 / :235: int = int * 0.8f
        scored = []
        for k in sharing:                                     # :125-138 / :241-253
            if words(k) > min_common:
                si = F32(score_l1(bow, k.bow))
                if loop:
                    k.mLoopScore = si
                    if si >= F32(min_score):
                        scored.append((si, k.mnId))
                else:
                    k.mRelocScore = si
                    scored.append((si, k.mnId))
        return scored, min_common

    def query_end(self, loop, query_id, scored, min_common, covis, min_score=0.0):
        """:140-196 / :255-308; covis: id -> GetBestCovisibilityKeyFrames(10) ids."""
        if not scored:
            return []
        acc_list = []
        best_acc = F32(min_score) if loop else F32(0.0)
        for si, kid in scored:
            best_score = si
            acc = si
            best = kid
            for nid in covis.get(kid, ()):
                k2 = self.kfs.get(nid) or KF(nid)        # a keyframe never added: constructor state
                if loop:
                    if not (k2.mnLoopQuery == query_id and k2.mnLoopWords > min_common):
                        continue
                    s = k2.mLoopScore
                else:
                    if k2.mnRelocQuery != query_id:
                        continue
                    s = k2.mRelocScore
                acc = F32(acc + s)
                if s > best_score:
                    best = nid
                    best_score = s
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        min_retain = F32(F32(0.75) * best_acc)
        added, out = set(), []
        for acc, kid in acc_list:
            if acc > min_retain and kid not in added:
                out.append(kid)
                added.add(kid)
        return out

    def DetectRelocalizationCandidates(self, query_id, bow, covis):
        scored, mc = self.query_begin(False, query_id, bow)
        return self.query_end(False, query_id, scored, mc, covis)

    def DetectLoopCandidates(self, query_id, bow, connected, min_score, covis):
        scored, mc = self.query_begin(True, query_id, bow, connected, min_score)
        return self.query_end(True, query_id, scored, mc, covis, min_score)
