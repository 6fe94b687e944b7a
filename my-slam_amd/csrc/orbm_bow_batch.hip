// orbm_bow_batch.hip -- ORBmatcher::SearchByBoW (src/ORBmatcher.cc:159-288 and :522-655 of WChen09/My-SLAM) for ALL candidate key
// frames of a relocalisation (src/Tracking.cc:1377-1398) or of a loop detection (src/LoopClosing.cc:253-281) in one call
// (include/orbm.h):
//   orbm_search_by_bow_batch      nkf key frames against one frame        == orbm_search_by_bow(kfs[c], frame) for every c
//   orbm_search_by_bow_kf_batch   one key frame against nkf key frames    == orbm_search_by_bow_kf(kf1, kfs2[c]) for every c
//
// Why the candidates can share a launch: every call of the loop writes a table of its own and reads only its
// own key frame and the shared side; the skip of :209 acts inside one call and one vocabulary node.  So a work item is a
// (candidate, shared node) pair, one wave runs bow_walk() (orbm_bow_body.h, k_bow_select's body) on it, and the waves do not interact.
//
// One call: one upload (the shared side once, then every candidate's descriptors, `valid` and node lists, all in one block), one
// launch, one download of the tables, one synchronisation.  A work item addresses its two sides by offsets into that block:
//   r = serial list [x, y), lane list [z, w)           feature indices, in ints from the block's start
//   b = x: serial descriptors, y: lane descriptors     in descriptors (32 bytes) from the block's start
//       z: the serial side's `valid`                   in bytes from the block's start, -1 = every feature is valid
//       w: the table row of the candidate              in ints from the table's start
// In the frame variant the shared frame is on the lanes and the candidate is serial; in the key-frame variant the shared key frame 1
// is serial and the candidate is on the lanes.  The indices in a table are local to their candidate.
#include "orbm_internal.h"
#include "orbm_bow_body.h"

struct BowItem { int4 r, b; };

__global__ __launch_bounds__(M_THREADS) void k_bow_select_batch(const uint8_t *__restrict__ blk, const BowItem *__restrict__ items, int nitems,
                                                               float nnratio, int th, int32_t *__restrict__ table)
{
    __shared__ BowStage st;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int w = blockIdx.x * BOW_WAVES + wv;
    if (w >= nitems) return;                 // whole waves leave; nothing below is a block-wide barrier
    // the whole wave serves one item: through readfirstlane its record is scalar loads and the bases stay in scalar registers
    const BowItem *__restrict__ it = items + __builtin_amdgcn_readfirstlane(w);
    const int4 r = it->r, b = it->b;
    const uint4 *D = reinterpret_cast<const uint4 *>(blk);
    const int32_t *I = reinterpret_cast<const int32_t *>(blk);
    bow_walk(st, wv, lane, D + 2 * (long long)b.x, D + 2 * (long long)b.y, I, I, r, b.z >= 0 ? blk + b.z : nullptr, nnratio, th,
             table + b.w);
}

// -------------------------------------------------------------------------------------------------
// host side, shared by the two entry points
// -------------------------------------------------------------------------------------------------
// one side as the entry points receive it: counts, buffers, FeatureVector (offsets monotone from 0, node ids strictly ascending, every
// feature index inside [0, n))
static int bow_check_side(const char *what, int c, const orbm_bow_side *s, bool need_valid)
{
    char name[48];
    if (c >= 0) snprintf(name, sizeof name, "%s %d", what, c);
    else snprintf(name, sizeof name, "%s", what);
    if (s->n < 0 || s->fv_n < 0) return mfail(ORBX_E_INVALID, "%s: negative count (n=%d fv_n=%d)", name, s->n, s->fv_n);
    if (s->n == 0 || s->fv_n == 0) return ORBX_OK;      // nothing of it is read, as in the one-candidate calls: 0 matches
    if (!s->desc || !s->kps || (need_valid && !s->valid)) return mfail(ORBX_E_INVALID, "%s: NULL buffer", name);
    if (!s->fv_node || !s->fv_off) return mfail(ORBX_E_INVALID, "%s: NULL buffer", name);
    if (s->fv_off[0] != 0) return mfail(ORBX_E_INVALID, "%s: fv_off[0] must be 0", name);
    for (int a = 0; a < s->fv_n; a++) {
        if (s->fv_off[a + 1] < s->fv_off[a]) return mfail(ORBX_E_INVALID, "%s: fv_off not monotone at node %d", name, a);
        if (a > 0 && s->fv_node[a] <= s->fv_node[a - 1]) return mfail(ORBX_E_INVALID, "%s: node ids not ascending at node %d", name, a);
    }
    const int ni = s->fv_off[s->fv_n];
    if (ni > 0 && !s->fv_idx) return mfail(ORBX_E_INVALID, "%s: NULL buffer", name);
    for (int k = 0; k < ni; k++)
        if (s->fv_idx[k] < 0 || s->fv_idx[k] >= s->n) return mfail(ORBX_E_INVALID, "%s: feature index %d outside [0,%d)", name, s->fv_idx[k], s->n);
    return ORBX_OK;
}

static bool bow_force_host()
{
    static const bool force_host = [] { const char *e = getenv("ORBM_BOW_HOST_SELECT"); return e && e[0] == '1'; }();
    return force_host;
}

// One candidate of a batch as the launch sees it.  Both FeatureVectors have passed bow_check_side; the lane side's lists may be a
// filtered copy (key-frame variant).
struct BowJob {
    const uint8_t *s_desc, *s_valid; int s_n;                                  // serial side
    const int32_t *s_node, *s_off, *s_idx; int s_fv_n;
    const uint8_t *l_desc; int l_n;                                            // lane side
    const int32_t *l_node, *l_off, *l_idx; int l_fv_n;
    int32_t *out;                                                              // host table of l_n entries, all -1 on entry
    enum { EMPTY, LAUNCH, SINGLE } kind = EMPTY;                               // SINGLE: answered by the one-candidate entry point
    std::vector<int4> pairs;                                                   // the merge-join of :178-262: serial [x, y), lane [z, w)
    int row = 0;                                                               // its row in the device table
};

// the (candidate, shared node) pairs of one job, as search_by_bow_device (orbm.hip) finds them for one call; a pair whose serial
// features are all unusable is left out (its lane-side entries stay -1, as the walk would leave them)
static void bow_job_pairs(BowJob &j)
{
    j.pairs.clear();
    j.kind = BowJob::EMPTY;
    if (j.s_n == 0 || j.l_n == 0) return;
    for (int a = 0, b = 0; a < j.s_fv_n && b < j.l_fv_n;) {
        if (j.s_node[a] == j.l_node[b]) {
            const int ns = j.s_off[a + 1] - j.s_off[a], nl = j.l_off[b + 1] - j.l_off[b];
            if (ns > 0 && nl > 0) {
                if (nl > BOW_MAX_NODE_FEATURES || bow_force_host()) { j.kind = BowJob::SINGLE; j.pairs.clear(); return; }
                bool usable = !j.s_valid;
                for (int c = j.s_off[a]; !usable && c < j.s_off[a + 1]; c++) usable = j.s_valid[j.s_idx[c]] != 0;
                if (usable) j.pairs.push_back(make_int4(j.s_off[a], j.s_off[a + 1], j.l_off[b], j.l_off[b + 1]));
            }
            a++; b++;
        } else if (j.s_node[a] < j.l_node[b]) a++;
        else b++;
    }
    if (!j.pairs.empty()) j.kind = BowJob::LAUNCH;
}

// The LAUNCH jobs of a batch: one upload, one launch, one download, one synchronisation.  shared_on_lanes: every job has the same
// lane side (frame variant); otherwise every job has the same serial side (key-frame variant).
static int bow_batch_launch(orbm_matcher *m, std::vector<BowJob> &jobs, bool shared_on_lanes, float nnratio, int th)
{
    long long table = 0, nitems = 0;
    const BowJob *first = nullptr;
    for (BowJob &j : jobs) {
        if (j.kind != BowJob::LAUNCH) continue;
        if (!first) first = &j;
        j.row = (int)table;
        table += j.l_n; nitems += (long long)j.pairs.size();
        if (table > (1ll << 28) || nitems > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 table entries");
    }
    if (!first) return ORBX_OK;
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, 0, 0, table));                // the tables live in d_out (max_pairs also sizes d_idx, which this call does not use)
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    struct Where { size_t desc, valid, idx; };     // byte offsets of a side's parts in the block
    auto put = [&](const void *src, size_t bytes) { const int k = in.add(src, bytes); return in.parts[k].off; };
    auto add_serial = [&](const BowJob &j) {
        Where w;
        w.desc = put(j.s_desc, (size_t)j.s_n * 32);
        w.valid = j.s_valid ? put(j.s_valid, (size_t)j.s_n) : (size_t)-1;
        w.idx = put(j.s_idx, (size_t)j.s_off[j.s_fv_n] * 4);
        return w;
    };
    auto add_lane = [&](const BowJob &j) {
        Where w;
        w.desc = put(j.l_desc, (size_t)j.l_n * 32);
        w.valid = (size_t)-1;
        w.idx = put(j.l_idx, (size_t)j.l_off[j.l_fv_n] * 4);
        return w;
    };
    const Where shared = shared_on_lanes ? add_lane(*first) : add_serial(*first);
    std::vector<Where> own(jobs.size());
    for (size_t c = 0; c < jobs.size(); c++)
        if (jobs[c].kind == BowJob::LAUNCH) own[c] = shared_on_lanes ? add_serial(jobs[c]) : add_lane(jobs[c]);
    if (in.total + (size_t)nitems * sizeof(BowItem) > ((size_t)1 << 31) - 64) return mfail(ORBX_E_CAPACITY, "request beyond 2^31 bytes of input");
    std::vector<BowItem> items;
    items.reserve((size_t)nitems);
    for (size_t c = 0; c < jobs.size(); c++) {
        const BowJob &j = jobs[c];
        if (j.kind != BowJob::LAUNCH) continue;
        const Where &ws = shared_on_lanes ? own[c] : shared, &wl = shared_on_lanes ? shared : own[c];
        const int si = (int)(ws.idx / 4), li = (int)(wl.idx / 4);
        for (const int4 &p : j.pairs) {
            BowItem it;
            it.r = make_int4(si + p.x, si + p.y, li + p.z, li + p.w);
            it.b = make_int4((int)(ws.desc / 32), (int)(wl.desc / 32), ws.valid == (size_t)-1 ? -1 : (int)ws.valid, j.row);
            items.push_back(it);
        }
    }
    const int pi = in.add(items.data(), items.size() * sizeof(BowItem));
    MTRY(in.upload(s));
    const int ni = (int)items.size();
    hipLaunchKernelGGL(k_bow_select_batch, dim3((ni + BOW_WAVES - 1) / BOW_WAVES), dim3(M_THREADS), 0, s, in.dev, in.at<BowItem>(pi), ni, nnratio, th,
                       m->d_out.get());
    MHIPCHK(hipGetLastError());
    std::vector<int32_t> dl((size_t)table);
    MTRY(orbm_d2h(m, dl.data(), m->d_out, (size_t)table * 4, s));
    MTRY(orbm_sync(m, s));
    for (BowJob &j : jobs) {                        // the kernel wrote the entries of the paired nodes only
        if (j.kind != BowJob::LAUNCH) continue;
        for (const int4 &p : j.pairs)
            for (int c = p.z; c < p.w; c++) j.out[j.l_idx[c]] = dl[(size_t)j.row + j.l_idx[c]];
    }
    return ORBX_OK;
}

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
extern "C" int orbm_search_by_bow_batch(orbm_matcher *m, const orbm_bow_side *kfs, int nkf, const orbm_bow_side *frame, float nnratio,
                                        int check_orientation, int32_t *match_f, int32_t *nmatches)
{
    if (nkf < 0) return mfail(ORBX_E_INVALID, "nkf=%d", nkf);
    if (nkf == 0) return ORBX_OK;
    if (!kfs || !frame || !nmatches) return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(bow_check_side("frame", -1, frame, false));
    for (int c = 0; c < nkf; c++) MTRY(bow_check_side("key frame", c, &kfs[c], false));
    const int nf = frame->n;
    if (nf > 0 && !match_f) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (nkf > (1 << 20) || (long long)nkf * nf > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 (key frame, feature) slots");

    // everything is computed into `table` and committed at the end: a failed call leaves the outputs as they were
    std::vector<int32_t> table((size_t)nkf * nf, -1), counts((size_t)nkf, 0);
    std::vector<BowJob> jobs((size_t)nkf);
    bool device = false;
    if (nf > 0 && frame->fv_n > 0)
        for (int c = 0; c < nkf; c++) {
            const orbm_bow_side &k = kfs[c];
            BowJob &j = jobs[c];
            j.s_desc = k.desc; j.s_valid = k.valid; j.s_n = k.n; j.s_node = k.fv_node; j.s_off = k.fv_off; j.s_idx = k.fv_idx; j.s_fv_n = k.fv_n;
            j.l_desc = frame->desc; j.l_n = nf; j.l_node = frame->fv_node; j.l_off = frame->fv_off; j.l_idx = frame->fv_idx; j.l_fv_n = frame->fv_n;
            j.out = table.data() + (size_t)c * nf;
            bow_job_pairs(j);
            device |= j.kind != BowJob::EMPTY;
        }
    if (device) {
        if (!m) return orbm_no_handle();
        MTRY(bow_batch_launch(m, jobs, true, nnratio, ORBM_TH_LOW));
        for (int c = 0; c < nkf; c++) {
            const orbm_bow_side &k = kfs[c];
            int nm = 0;
            if (jobs[c].kind == BowJob::LAUNCH)
                MTRY(bow_rotation_cull(k.kps, frame->kps, nf, check_orientation, jobs[c].out, &nm));
            else if (jobs[c].kind == BowJob::SINGLE)     // a node beyond the lanes' reach, or host selection forced
                MTRY(orbm_search_by_bow(m, k.desc, k.kps, k.n, k.valid, k.fv_node, k.fv_off, k.fv_idx, k.fv_n, frame->desc, frame->kps, nf,
                                        frame->fv_node, frame->fv_off, frame->fv_idx, frame->fv_n, nnratio, check_orientation, jobs[c].out, &nm));
            counts[c] = nm;
        }
    }
    if (nf > 0) memcpy(match_f, table.data(), table.size() * 4);
    memcpy(nmatches, counts.data(), (size_t)nkf * 4);
    return ORBX_OK;
}

extern "C" int orbm_search_by_bow_kf_batch(orbm_matcher *m, const orbm_bow_side *kf1, const orbm_bow_side *kfs2, int nkf, float nnratio,
                                           int check_orientation, int32_t *matches12, int32_t *nmatches)
{
    if (nkf < 0) return mfail(ORBX_E_INVALID, "nkf=%d", nkf);
    if (nkf == 0) return ORBX_OK;
    if (!kf1 || !kfs2 || !nmatches) return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(bow_check_side("key frame 1", -1, kf1, true));
    for (int c = 0; c < nkf; c++) MTRY(bow_check_side("second key frame", c, &kfs2[c], true));
    const int n1 = kf1->n;
    if (n1 > 0 && !matches12) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (nkf > (1 << 20) || (long long)nkf * n1 > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 (key frame, feature) slots");

    std::vector<int32_t> table((size_t)nkf * n1, -1), counts((size_t)nkf, 0);
    std::vector<BowJob> jobs((size_t)nkf);
    // per candidate: its node lists without the features that can never be taken (:576-580), and its own table (feature of key frame 2
    // -> feature of key frame 1), which is inverted into the row of matches12 at the end
    std::vector<std::vector<int32_t>> off2((size_t)nkf), idx2((size_t)nkf), match2((size_t)nkf);
    bool device = false;
    if (n1 > 0 && kf1->fv_n > 0)
        for (int c = 0; c < nkf; c++) {
            const orbm_bow_side &k = kfs2[c];
            if (k.n == 0 || k.fv_n == 0) continue;
            off2[c].assign((size_t)k.fv_n + 1, 0);
            idx2[c].reserve((size_t)k.fv_off[k.fv_n]);
            for (int b = 0; b < k.fv_n; b++) {
                for (int e = k.fv_off[b]; e < k.fv_off[b + 1]; e++)
                    if (k.valid[k.fv_idx[e]]) idx2[c].push_back(k.fv_idx[e]);
                off2[c][(size_t)b + 1] = (int32_t)idx2[c].size();
            }
            if (idx2[c].empty()) continue;
            match2[c].assign((size_t)k.n, -1);
            BowJob &j = jobs[c];
            j.s_desc = kf1->desc; j.s_valid = kf1->valid; j.s_n = n1; j.s_node = kf1->fv_node; j.s_off = kf1->fv_off; j.s_idx = kf1->fv_idx; j.s_fv_n = kf1->fv_n;
            j.l_desc = k.desc; j.l_n = k.n; j.l_node = k.fv_node; j.l_off = off2[c].data(); j.l_idx = idx2[c].data(); j.l_fv_n = k.fv_n;
            j.out = match2[c].data();
            bow_job_pairs(j);
            device |= j.kind != BowJob::EMPTY;
        }
    if (device) {
        if (!m) return orbm_no_handle();
        MTRY(bow_batch_launch(m, jobs, false, nnratio, ORBM_TH_LOW - 1));
        for (int c = 0; c < nkf; c++) {
            const orbm_bow_side &k = kfs2[c];
            int32_t *row = table.data() + (size_t)c * n1;
            int nm = 0;
            if (jobs[c].kind == BowJob::LAUNCH) {
                MTRY(bow_rotation_cull(kf1->kps, k.kps, k.n, check_orientation, match2[c].data(), &nm));
                for (int i2 = 0; i2 < k.n; i2++)
                    if (match2[c][i2] >= 0) row[match2[c][i2]] = i2;
            } else if (jobs[c].kind == BowJob::SINGLE)
                MTRY(orbm_search_by_bow_kf(m, kf1->desc, kf1->kps, n1, kf1->valid, kf1->fv_node, kf1->fv_off, kf1->fv_idx, kf1->fv_n, k.desc, k.kps, k.n,
                                           k.valid, k.fv_node, k.fv_off, k.fv_idx, k.fv_n, nnratio, check_orientation, row, &nm));
            counts[c] = nm;
        }
    }
    if (n1 > 0) memcpy(matches12, table.data(), table.size() * 4);
    memcpy(nmatches, counts.data(), (size_t)nkf * 4);
    return ORBX_OK;
}
