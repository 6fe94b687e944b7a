/*
 * orbk.h -- C ABI of the keyframe database of liborbx.so: place recognition for relocalisation and loop closing.
 *
 * Reference (WChen09/My-SLAM):
 *   src/KeyFrameDatabase.cc:40-73    add / erase / clear of the inverted file (one list per word, keyframes in add order)
 *   src/KeyFrameDatabase.cc:76-197   DetectLoopCandidates(pKF, minScore)      called at src/LoopClosing.cc:142
 *   src/KeyFrameDatabase.cc:199-309  DetectRelocalizationCandidates(F)        called at src/Tracking.cc:1355
 *   Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68  L1Scoring::score
 *
 * The GPU holds the BowVector of every live keyframe in one arena and scores a query against all of them in one pass
 * (orbk_score).  The host runs the reference's control flow over those records: the encounter order of lKFsSharingWords
 * (the position in the query of the first shared word, then the add order), the word counts, minCommonWords, the float
 * scores and the covisibility accumulation.  The results are the reference's bit for bit, including:
 *   - per-keyframe query state (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore) lives in
 *     the handle, keyed by id, and persists across queries, clear(), erase and re-add; an id the handle has never seen
 *     has the constructor's state (query ids 0, counts 0).  So a relocalisation neighbour whose mnRelocQuery equals the
 *     query id contributes the mRelocScore an earlier query left, a query id of 0 pushes no keyframe that was never
 *     queried, and a repeated query id accumulates counts;
 *   - Deviation: the reference never initialises mLoopScore / mRelocScore (src/KeyFrame.cc:30-42), so reading one that
 *     was never written is undefined there.  Here it reads 0.0f.
 *   - Deviation: a word id outside [0, nwords) indexes past mvInvertedFile in the reference (src/KeyFrameDatabase.cc:45,
 *     :56, :88, :209): undefined there.  Here every entry point that takes a BowVector returns ORBX_E_INVALID for it.
 *   - Deviation: orbk_add of an id that is already in the database returns ORBX_E_INVALID (the reference would list the
 *     keyframe twice in the inverted file; it never does this itself).  orbk_erase of an absent id is a no-op.
 *
 * A query is two calls, because the reference reads GetBestCovisibilityKeyFrames(10) only for the scored keyframes:
 *   orbk_query_begin  voting, scoring and the state update; returns lScoreAndMatch (ids and float si) in encounter order
 *   orbk_query_end    the caller's GetBestCovisibilityKeyFrames(10) of each scored id, in that order; returns the candidates
 * One query of each kind may be pending at a time (a begin replaces a pending query of its kind); every entry point locks
 * the handle, so Tracking, LocalMapping and LoopClosing may share it.
 *
 * Ids are the caller's KeyFrame::mnId / Frame::mnId.  BowVectors are ascending word ids in [0, nwords) with their values.
 * There is no CPU path: orbk_create without a HIP device fails with ORBX_E_HIP.
 */
#ifndef ORBK_H
#define ORBK_H

#include <stdint.h>
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbk_database orbk_database;

enum { ORBK_RELOC = 0, ORBK_LOOP = 1 };

/* one live keyframe sharing at least one word with the query */
typedef struct {
    uint64_t id;        /* keyframe id */
    int32_t words;      /* number of query words it shares */
    int32_t first;      /* position in the query BowVector of the first shared word */
    double score;       /* L1Scoring::score(query, keyframe), DBoW2's summation order */
} orbk_record;

/* scoring must be ORBV_L1_NORM (include/orbv.h); max_keyframes / max_entries only size the arena at first: it grows. */
int orbk_create(orbk_database **out, int device, int nwords, int scoring, int max_keyframes, int max_entries);
void orbk_destroy(orbk_database *db);
int orbk_add(orbk_database *db, uint64_t id, const int32_t *word_ids, const double *values, int n);
int orbk_erase(orbk_database *db, uint64_t id);
int orbk_clear(orbk_database *db);
int orbk_size(const orbk_database *db);           /* live keyframes, or ORBX_E_INVALID for a NULL handle */

/* Stateless: one record per live keyframe sharing a word, in add order.  ORBX_E_CAPACITY (and *nout = the count) if cap
 * is too small. */
int orbk_score(orbk_database *db, const int32_t *ids, const double *vals, int n, orbk_record *out, int cap, int *nout);

/* kind ORBK_RELOC: DetectRelocalizationCandidates(F) with query_id = F->mnId (connected / min_score unused).
 * kind ORBK_LOOP:  DetectLoopCandidates(pKF, minScore) with query_id = pKF->mnId, connected = GetConnectedKeyFrames().
 * Writes the scored list (lScoreAndMatch) to scored / scores.  If cap is too small: ORBX_E_CAPACITY, *nscored = the
 * needed count, and no state is changed (a retry equals a single call with a large enough buffer). */
int orbk_query_begin(orbk_database *db, int kind, uint64_t query_id, const int32_t *ids, const double *vals, int n,
                     const uint64_t *connected, int nconnected, float min_score,
                     uint64_t *scored, float *scores, int cap, int *nscored);
/* nb_off[0..nscored], nb_ids: GetBestCovisibilityKeyFrames(10) of scored[i] is nb_ids[nb_off[i] .. nb_off[i+1]).
 * Writes the candidates in the reference's order.  ORBX_E_CAPACITY (*ncandidates = the count, the query stays pending) if
 * cap is too small; ORBX_E_INVALID without a pending begin of the same kind. */
int orbk_query_end(orbk_database *db, int kind, const int32_t *nb_off, const uint64_t *nb_ids,
                   uint64_t *candidates, int cap, int *ncandidates);

const char *orbk_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
