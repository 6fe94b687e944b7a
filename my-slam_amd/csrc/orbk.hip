// orbk.hip -- keyframe database (src/KeyFrameDatabase.cc of WChen09/My-SLAM): the BowVectors of every live keyframe in one
// device arena, one scoring pass of a query against all of them, and the reference's control flow on the host.
// See include/orbk.h.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "orbk_internal.h"
#include "../../include/orbv.h"

#define K_THREADS 256
#define K_LDS_QUERY 8192          // query word ids staged in LDS up to this length (32 KiB); longer queries search global memory
#define K_MAX_BLOCKS 2048         // the waves of a launch stride over the slots: the query is staged once per block, not per slot

struct KRecDev { int32_t slot, words, first, pad; double score; };

// lower bound of w in the ascending q[0, n); -1 if absent
__device__ __forceinline__ int find_word(const int32_t *q, int n, int32_t w)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < w) lo = mid + 1; else hi = mid;
    }
    return (lo < n && q[lo] == w) ? lo : -1;
}

// One wave per keyframe slot.  Each lane takes one entry of a 64-entry chunk and binary-searches its word in the query; the
// count is the ballot's popcount, the first shared query position is that of the chunk's lowest matching lane in the first
// chunk with a match (both BowVectors ascend), and the L1 terms of the matched lanes are added one at a time in lane order:
// ascending common words, DBoW2's summation order (ScoringObject.cpp:37-42).  The sum is wave-uniform.
template <bool kLds>
__global__ __launch_bounds__(K_THREADS) void k_kfdb_score(const int32_t *__restrict__ kf_ids, const double *__restrict__ kf_vals,
                                                        const KSlotDev *__restrict__ slots, int nslots,
                                                        const int32_t *__restrict__ q_ids, const double *__restrict__ q_vals, int nq,
                                                        int32_t *__restrict__ counter, KRecDev *__restrict__ rec)
{
    extern __shared__ __attribute__((aligned(16))) int32_t s_q[];
    if (kLds) {
        for (int i = threadIdx.x; i < nq; i += K_THREADS) s_q[i] = q_ids[i];
        __syncthreads();
    }
    const int32_t *Q = kLds ? s_q : q_ids;
    const int32_t qmin = q_ids[0], qmax = q_ids[nq - 1];
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * (K_THREADS / 64);
    for (int s = blockIdx.x * (K_THREADS / 64) + (threadIdx.x >> 6); s < nslots; s += nwaves) {
        const KSlotDev sl = slots[s];
        int words = 0, first = -1;
        double score = 0.0;
        for (int base = 0; base < sl.len; base += 64) {
            const int e = base + lane;
            int pos = -1;
            int32_t w = 0;
            if (e < sl.len) {
                w = kf_ids[sl.off + e];
                if (w >= qmin && w <= qmax) pos = find_word(Q, nq, w);
            }
            unsigned long long m = __ballot(pos >= 0);
            if (m == 0) continue;
            words += __popcll(m);
            if (first < 0) first = __shfl(pos, __ffsll((long long)m) - 1);
            double t = 0.0;
            if (pos >= 0) {
                const double vi = q_vals[pos], wi = kf_vals[sl.off + e];
                t = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
            while (m) {
                score += __shfl(t, __ffsll((long long)m) - 1);
                m &= m - 1;
            }
        }
        if (words > 0 && lane == 0) {
            const int o = atomicAdd(counter, 1);
            KRecDev r;
            r.slot = s; r.words = words; r.first = first; r.pad = 0; r.score = -score / 2.0;
            rec[o] = r;
        }
    }
}

// arena compaction: one wave per surviving slot copies its entries to their new offset
__global__ __launch_bounds__(K_THREADS) void k_kfdb_compact(const int32_t *__restrict__ src_ids, const double *__restrict__ src_vals,
                                                          int32_t *__restrict__ dst_ids, double *__restrict__ dst_vals,
                                                          const long long *__restrict__ plan, int nplan)
{
    const int j = blockIdx.x * (K_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= nplan) return;
    const long long src = plan[3 * j], dst = plan[3 * j + 1], len = plan[3 * j + 2];
    for (long long e = threadIdx.x & 63; e < len; e += 64) {
        dst_ids[dst + e] = src_ids[src + e];
        dst_vals[dst + e] = src_vals[src + e];
    }
}

struct KRec { int slot, words, first; double score; };

static size_t query_bytes(int n) { return align16((size_t)n * 4) + align16((size_t)n * 8); }

static int check_bow(const orbk_database *db, const int32_t *ids, const double *vals, int n)
{
    if (n < 0) return kfail(ORBX_E_INVALID, "n = %d", n);
    if (n > 0 && (!ids || !vals)) return kfail(ORBX_E_INVALID, "NULL BowVector");
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= db->nwords) return kfail(ORBX_E_INVALID, "word id %d outside [0, %d)", ids[i], db->nwords);
        if (i > 0 && ids[i] <= ids[i - 1]) return kfail(ORBX_E_INVALID, "word ids not strictly ascending at %d", i);
    }
    return ORBX_OK;
}

hipError_t orbk_launch_compact(const int32_t *src_ids, const double *src_vals, int32_t *dst_ids, double *dst_vals,
                               const long long *d_plan, int nplan, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfdb_compact, dim3((nplan + 3) / 4), dim3(K_THREADS), 0, s, src_ids, src_vals, dst_ids, dst_vals, d_plan, nplan);
    return hipGetLastError();
}

// The scoring pass: one record per live slot sharing a word with the query, in no particular order.
static int run_score(orbk_database *db, const int32_t *ids, const double *vals, int n, std::vector<KRec> &out)
{
    out.clear();
    if (n == 0 || db->nlive == 0) return ORBX_OK;
    const int nslots = (int)db->slots.size();
    const size_t qb = query_bytes(n);
    int rc = orbk_ensure_io(db, qb + 16 + (size_t)nslots * sizeof(KRecDev));
    if (rc != ORBX_OK) return rc;
    std::memcpy(db->h_io, ids, (size_t)n * 4);
    std::memcpy(db->h_io + align16((size_t)n * 4), vals, (size_t)n * 8);
    std::memset(db->h_io + qb, 0, 16);
    KHIP(hipMemcpyAsync(db->d_io, db->h_io, qb + 16, hipMemcpyHostToDevice, db->stream));
    const int32_t *d_q = reinterpret_cast<const int32_t *>(db->d_io.get());
    const double *d_qv = reinterpret_cast<const double *>(db->d_io + align16((size_t)n * 4));
    int32_t *d_cnt = reinterpret_cast<int32_t *>(db->d_io + qb);
    KRecDev *d_rec = reinterpret_cast<KRecDev *>(db->d_io + qb + 16);
    const int blocks = std::min((nslots + 3) / 4, K_MAX_BLOCKS);
    if (n <= K_LDS_QUERY)
        hipLaunchKernelGGL(k_kfdb_score<true>, dim3(blocks), dim3(K_THREADS), (size_t)n * 4, db->stream, db->d_ids, db->d_vals, db->d_slots,
                           nslots, d_q, d_qv, n, d_cnt, d_rec);
    else
        hipLaunchKernelGGL(k_kfdb_score<false>, dim3(blocks), dim3(K_THREADS), 0, db->stream, db->d_ids, db->d_vals, db->d_slots, nslots,
                           d_q, d_qv, n, d_cnt, d_rec);
    KHIP(hipGetLastError());
    // the counter and the first rec_hint records come back in one copy; a second copy only when the count outgrows the hint
    const int guess = std::min(nslots, std::max(db->rec_hint, 256));
    KHIP(hipMemcpyAsync(db->h_io + qb, db->d_io + qb, 16 + (size_t)guess * sizeof(KRecDev), hipMemcpyDeviceToHost, db->stream));
    KHIP(hipStreamSynchronize(db->stream));
    int cnt = 0;
    std::memcpy(&cnt, db->h_io + qb, 4);
    if (cnt < 0 || cnt > nslots) return kfail(ORBX_E_HIP, "scoring kernel returned %d records for %d slots", cnt, nslots);
    if (cnt > guess) {
        KHIP(hipMemcpyAsync(db->h_io + qb + 16 + (size_t)guess * sizeof(KRecDev), db->d_io + qb + 16 + (size_t)guess * sizeof(KRecDev),
                            (size_t)(cnt - guess) * sizeof(KRecDev), hipMemcpyDeviceToHost, db->stream));
        KHIP(hipStreamSynchronize(db->stream));
    }
    db->rec_hint = std::min(nslots, cnt + cnt / 4);
    const KRecDev *r = reinterpret_cast<const KRecDev *>(db->h_io + qb + 16);
    out.resize(cnt);
    for (int i = 0; i < cnt; i++) out[i] = KRec{r[i].slot, r[i].words, r[i].first, r[i].score};
    return ORBX_OK;
}

extern "C" int orbk_add(orbk_database *db, uint64_t id, const int32_t *word_ids, const double *values, int n)
{
    if (!db) return kfail(ORBX_E_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lk(db->mu);
    int rc = check_bow(db, word_ids, values, n);
    if (rc != ORBX_OK) return rc;
    if (db->slot_of.count(id)) return kfail(ORBX_E_INVALID, "keyframe %llu is already in the database", (unsigned long long)id);
    KHIP(hipSetDevice(db->device));
    if ((rc = orbk_make_room(db, n)) != ORBX_OK) return rc;
    if ((rc = orbk_ensure_io(db, align16((size_t)n * 4) + (size_t)n * 8 + sizeof(KSlotDev))) != ORBX_OK) return rc;
    const int s = (int)db->slots.size();
    const long long off = db->tail;
    const KSlotDev sd{off, n, 0};
    const size_t vo = align16((size_t)n * 4), so = vo + (size_t)n * 8;
    if (n > 0) {
        std::memcpy(db->h_io, word_ids, (size_t)n * 4);
        std::memcpy(db->h_io + vo, values, (size_t)n * 8);
    }
    std::memcpy(db->h_io + so, &sd, sizeof(sd));
    if (n > 0) {
        KHIP(hipMemcpyAsync(db->d_ids + off, db->h_io, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
        KHIP(hipMemcpyAsync(db->d_vals + off, db->h_io + vo, (size_t)n * 8, hipMemcpyHostToDevice, db->stream));
    }
    KHIP(hipMemcpyAsync(db->d_slots + s, db->h_io + so, sizeof(sd), hipMemcpyHostToDevice, db->stream));
    KHIP(hipStreamSynchronize(db->stream));       // h_io is reused by the next call
    db->slots.push_back(KSlot{id, off, n, true, &db->state[id]});
    db->slot_of[id] = s;
    db->tail += n; db->live_entries += n; db->nlive++;
    return ORBX_OK;
}

extern "C" int orbk_erase(orbk_database *db, uint64_t id)
{
    if (!db) return kfail(ORBX_E_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lk(db->mu);
    auto it = db->slot_of.find(id);
    if (it == db->slot_of.end()) return ORBX_OK;               // KeyFrameDatabase.cc:48-67 finds nothing to erase
    KSlot &s = db->slots[it->second];
    KHIP(hipSetDevice(db->device));
    if (s.len > 0) KHIP(hipMemsetAsync(&db->d_slots[it->second].len, 0, sizeof(int32_t), db->stream));
    s.live = false;
    db->live_entries -= s.len; db->nlive--;
    db->slot_of.erase(it);
    return ORBX_OK;
}

extern "C" int orbk_clear(orbk_database *db)
{
    if (!db) return kfail(ORBX_E_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lk(db->mu);
    db->slots.clear(); db->slot_of.clear();
    db->tail = 0; db->live_entries = 0; db->nlive = 0;
    return ORBX_OK;
}

extern "C" int orbk_size(const orbk_database *db)
{
    if (!db) return kfail(ORBX_E_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lk(db->mu);
    return db->nlive;
}

extern "C" int orbk_score(orbk_database *db, const int32_t *ids, const double *vals, int n, orbk_record *out, int cap, int *nout)
{
    if (!db || !nout || cap < 0 || (cap > 0 && !out)) return kfail(ORBX_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(db->mu);
    int rc = check_bow(db, ids, vals, n);
    if (rc != ORBX_OK) return rc;
    KHIP(hipSetDevice(db->device));
    std::vector<KRec> rec;
    if ((rc = run_score(db, ids, vals, n, rec)) != ORBX_OK) return rc;
    *nout = (int)rec.size();
    if ((int)rec.size() > cap) return kfail(ORBX_E_CAPACITY, "%zu records, capacity %d", rec.size(), cap);
    std::sort(rec.begin(), rec.end(), [](const KRec &a, const KRec &b) { return a.slot < b.slot; });
    for (size_t i = 0; i < rec.size(); i++)
        out[i] = orbk_record{db->slots[rec[i].slot].id, rec[i].words, rec[i].first, rec[i].score};
    return ORBX_OK;
}

// KeyFrameDatabase.cc:76-138 (loop) and :199-253 (relocalisation) over the records of the scoring pass.
extern "C" int orbk_query_begin(orbk_database *db, int kind, uint64_t query_id, const int32_t *ids, const double *vals, int n,
                                const uint64_t *connected, int nconnected, float min_score,
                                uint64_t *scored, float *scores, int cap, int *nscored)
{
    if (!db) return kfail(ORBX_E_INVALID, "NULL handle");
    if (kind != ORBK_RELOC && kind != ORBK_LOOP) return kfail(ORBX_E_INVALID, "query kind %d", kind);
    if (!nscored || cap < 0 || (cap > 0 && (!scored || !scores))) return kfail(ORBX_E_INVALID, "bad output buffer");
    if (nconnected < 0 || (nconnected > 0 && !connected)) return kfail(ORBX_E_INVALID, "bad connected list");
    std::lock_guard<std::mutex> lk(db->mu);
    int rc = check_bow(db, ids, vals, n);
    if (rc != ORBX_OK) return rc;
    KHIP(hipSetDevice(db->device));
    std::vector<KRec> rec;
    if ((rc = run_score(db, ids, vals, n, rec)) != ORBX_OK) return rc;
    const bool loop = kind == ORBK_LOOP;
    std::unordered_set<uint64_t> conn;
    if (loop) conn.insert(connected, connected + nconnected);
    // Voting (:83-105 / :203-222).  A keyframe's encounters all come in one pass over the query, so its outcome depends
    // only on its state before the query, whether it is connected, and its count.
    std::vector<uint64_t> nq(rec.size());
    std::vector<int> nw(rec.size());
    std::vector<int> pushed;
    int max_common = 0;
    for (size_t i = 0; i < rec.size(); i++) {
        const KSlot &s = db->slots[rec[i].slot];
        const uint64_t q = loop ? s.st->loop_q : s.st->reloc_q;
        const int w = loop ? s.st->loop_w : s.st->reloc_w;
        nq[i] = q;
        if (q == query_id) nw[i] = w + rec[i].words;                     // not reset, not pushed: counts accumulate
        else if (loop && conn.count(s.id)) nw[i] = 1;                  // reset to 0 at every encounter, then ++
        else { nq[i] = query_id; nw[i] = rec[i].words; pushed.push_back((int)i); max_common = std::max(max_common, nw[i]); }
    }
    const int min_common = (int)((float)max_common * 0.8f);            // int minCommonWords = maxCommonWords*0.8f
    // Scoring (:125-138 / :241-253) in encounter order: (position of the first shared query word, add order)
    std::vector<int> sc;
    for (int i : pushed)
        if (nw[i] > min_common) sc.push_back(i);
    std::sort(sc.begin(), sc.end(), [&](int a, int b) {
        return rec[a].first != rec[b].first ? rec[a].first < rec[b].first : rec[a].slot < rec[b].slot;
    });
    int kept = 0;
    for (int i : sc)
        if (!loop || (float)rec[i].score >= min_score) kept++;
    *nscored = kept;
    if (kept > cap) return kfail(ORBX_E_CAPACITY, "%d scored keyframes, capacity %d", kept, cap);
    // commit
    for (size_t i = 0; i < rec.size(); i++) {
        KState *st = db->slots[rec[i].slot].st;
        if (loop) { st->loop_q = nq[i]; st->loop_w = nw[i]; } else { st->reloc_q = nq[i]; st->reloc_w = nw[i]; }
    }
    KPending &p = db->pending[kind];
    p.active = true; p.qid = query_id; p.min_common = min_common; p.min_score = min_score;
    p.ids.clear(); p.si.clear();
    for (int i : sc) {
        const float si = (float)rec[i].score;
        KState *st = db->slots[rec[i].slot].st;
        if (loop) st->loop_s = si; else st->reloc_s = si;
        if (loop && !(si >= min_score)) continue;
        p.ids.push_back(db->slots[rec[i].slot].id);
        p.si.push_back(si);
    }
    for (int i = 0; i < kept; i++) { scored[i] = p.ids[i]; scores[i] = p.si[i]; }
    return ORBX_OK;
}

// KeyFrameDatabase.cc:140-196 (loop) and :255-308 (relocalisation)
extern "C" int orbk_query_end(orbk_database *db, int kind, const int32_t *nb_off, const uint64_t *nb_ids,
                              uint64_t *candidates, int cap, int *ncandidates)
{
    if (!db) return kfail(ORBX_E_INVALID, "NULL handle");
    if (kind != ORBK_RELOC && kind != ORBK_LOOP) return kfail(ORBX_E_INVALID, "query kind %d", kind);
    if (!ncandidates || cap < 0 || (cap > 0 && !candidates)) return kfail(ORBX_E_INVALID, "bad output buffer");
    std::lock_guard<std::mutex> lk(db->mu);
    KPending &p = db->pending[kind];
    if (!p.active) return kfail(ORBX_E_INVALID, "orbk_query_end without a pending orbk_query_begin of kind %d", kind);
    const int ns = (int)p.ids.size();
    if (ns > 0 && !nb_off) return kfail(ORBX_E_INVALID, "NULL neighbour offsets");
    for (int i = 0; i < ns; i++)
        if ((i == 0 && nb_off[0] != 0) || nb_off[i + 1] < nb_off[i]) return kfail(ORBX_E_INVALID, "neighbour offsets not ascending from 0");
    if (ns > 0 && nb_off[ns] > 0 && !nb_ids) return kfail(ORBX_E_INVALID, "NULL neighbour ids");
    const bool loop = kind == ORBK_LOOP;
    const KState fresh;
    std::vector<float> acc(ns);
    std::vector<uint64_t> best(ns);
    float best_acc = loop ? p.min_score : 0.0f;
    for (int i = 0; i < ns; i++) {
        float best_score = p.si[i], a = p.si[i];
        uint64_t b = p.ids[i];
        for (int k = nb_off[i]; k < nb_off[i + 1]; k++) {
            auto it = db->state.find(nb_ids[k]);
            const KState &st = it == db->state.end() ? fresh : it->second;
            float s;
            if (loop) {
                if (!(st.loop_q == p.qid && st.loop_w > p.min_common)) continue;
                s = st.loop_s;
            } else {
                if (st.reloc_q != p.qid) continue;
                s = st.reloc_s;
            }
            a += s;
            if (s > best_score) { b = nb_ids[k]; best_score = s; }
        }
        acc[i] = a; best[i] = b;
        if (a > best_acc) best_acc = a;
    }
    const float min_retain = 0.75f * best_acc;
    std::vector<uint64_t> out;
    std::unordered_set<uint64_t> added;
    for (int i = 0; i < ns; i++)
        if (acc[i] > min_retain && added.insert(best[i]).second) out.push_back(best[i]);
    *ncandidates = (int)out.size();
    if ((int)out.size() > cap) return kfail(ORBX_E_CAPACITY, "%zu candidates, capacity %d", out.size(), cap);
    std::copy(out.begin(), out.end(), candidates);
    p.active = false;
    return ORBX_OK;
}
