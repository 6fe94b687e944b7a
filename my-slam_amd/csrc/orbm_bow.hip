// orbm_bow.hip -- ORBmatcher::SearchByBoW (src/ORBmatcher.cc:159-288 and :522-655 of WChen09/My-SLAM): one implementation behind the
// four entry points of include/orbm.h.
//   orbm_search_by_bow            one key frame against a frame                      == the batch call with one candidate
//   orbm_search_by_bow_kf         one key frame against another                      == the batch call with one candidate
//   orbm_search_by_bow_batch      nkf key frames against one frame        (Tracking::Relocalization, src/Tracking.cc:1377-1398)
//   orbm_search_by_bow_kf_batch   one key frame against nkf key frames    (LoopClosing::ComputeSim3, src/LoopClosing.cc:253-281)
//
// Why the candidates can share a launch: every call of the loop writes a table of its own and reads only its
// own key frame and the shared side; the skip of :209 acts inside one call and one vocabulary node.  So a work item is a
// (candidate, shared node) pair, one wave runs bow_walk() (orbm_bow_body.h) on it, and the waves do not interact.
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

// the host-selection fallback's distances: pairs given explicitly as (query << 16 | train), both below 65536, so no per-thread
// binary search over off[] (otherwise: orbm_launch_dist_csr)
__global__ __launch_bounds__(M_THREADS) void k_dist_pairs16(const uint8_t *__restrict__ q, const uint8_t *__restrict__ t,
                                                            const uint32_t *__restrict__ pairs, int total, int32_t *__restrict__ dist)
{
    const int c = blockIdx.x * M_THREADS + threadIdx.x;
    if (c >= total) return;
    const uint32_t p = pairs[c];
    const uint4 *Q = reinterpret_cast<const uint4 *>(q) + 2 * (long long)(p >> 16);
    const uint4 *Tj = reinterpret_cast<const uint4 *>(t) + 2 * (long long)(p & 0xFFFFu);
    dist[c] = hamming256(Q[0], Q[1], Tj[0], Tj[1]);
}

// -------------------------------------------------------------------------------------------------
// host side, shared by the four entry points
// -------------------------------------------------------------------------------------------------
// one side as the entry points receive it: counts, buffers, FeatureVector (offsets monotone from 0, node ids strictly ascending, every
// feature index inside [0, n))
static int bow_check_side(const char *what, int c, const orbm_bow_side *s, bool need_valid)
{
    char buf[48];
    auto name = [&] {                                   // "key frame 3": composed for a refusal only
        if (c >= 0) snprintf(buf, sizeof buf, "%s %d", what, c);
        else snprintf(buf, sizeof buf, "%s", what);
        return buf;
    };
    if (s->n < 0 || s->fv_n < 0) return mfail(ORBX_E_INVALID, "%s: negative count (n=%d fv_n=%d)", name(), s->n, s->fv_n);
    if (s->n == 0 || s->fv_n == 0) return ORBX_OK;      // nothing of it is read: 0 matches
    if (!s->desc || !s->kps || (need_valid && !s->valid)) return mfail(ORBX_E_INVALID, "%s: NULL buffer", name());
    if (!s->fv_node || !s->fv_off) return mfail(ORBX_E_INVALID, "%s: NULL buffer", name());
    if (s->fv_off[0] != 0) return mfail(ORBX_E_INVALID, "%s: fv_off[0] must be 0", name());
    // every call pays for these scans, so the usual answer ("nothing wrong") comes from a branch-free pass; a refusal looks again
    // for its place and text
    bool bad = false;
    for (int a = 0; a < s->fv_n; a++) bad |= s->fv_off[a + 1] < s->fv_off[a];
    for (int a = 1; a < s->fv_n; a++) bad |= s->fv_node[a] <= s->fv_node[a - 1];
    for (int a = 0; bad && a < s->fv_n; a++) {
        if (s->fv_off[a + 1] < s->fv_off[a]) return mfail(ORBX_E_INVALID, "%s: fv_off not monotone at node %d", name(), a);
        if (a > 0 && s->fv_node[a] <= s->fv_node[a - 1]) return mfail(ORBX_E_INVALID, "%s: node ids not ascending at node %d", name(), a);
    }
    const int ni = s->fv_off[s->fv_n];
    if (ni > 0 && !s->fv_idx) return mfail(ORBX_E_INVALID, "%s: NULL buffer", name());
    for (int k = 0; k < ni; k++) bad |= (uint32_t)s->fv_idx[k] >= (uint32_t)s->n;      // negative or beyond n
    for (int k = 0; bad && k < ni; k++)
        if (s->fv_idx[k] < 0 || s->fv_idx[k] >= s->n) return mfail(ORBX_E_INVALID, "%s: feature index %d outside [0,%d)", name(), s->fv_idx[k], s->n);
    return ORBX_OK;
}

static bool bow_force_host()
{
    static const bool force_host = [] { const char *e = getenv("ORBM_BOW_HOST_SELECT"); return e && e[0] == '1'; }();
    return force_host;
}

// rotation histogram + ComputeThreeMaxima cull of SearchByBoW (:236-246, :266-284) on a finished table (out[lane-side feature] =
// serial-side feature or -1); *nmatches = what is left
static int bow_rotation_cull(const orbx_keypoint *kps_s, const orbx_keypoint *kps_l, int n_l, int check_orientation, int32_t *out, int32_t *nmatches)
{
    RotHist rot;
    int nm = 0;
    if (check_orientation) rot.entries.reserve((size_t)n_l);
    for (int i = 0; i < n_l; i++) {
        if (out[i] < 0) continue;
        nm++;
        if (check_orientation) MTRY(rot.add(kps_s[out[i]].angle, kps_l[i].angle, i));
    }
    if (check_orientation) rot.cull([&](int i) { out[i] = -1; nm--; });
    *nmatches = nm;
    return ORBX_OK;
}

// One candidate as the search sees it.  Both sides have passed bow_check_side; the lane side's fv_off / fv_idx may be a filtered
// copy (key-frame variant), kept in `lists`.
struct BowJob {
    orbm_bow_side s, l;                                                        // serial and lane side (of s: valid NULL = all usable)
    int32_t *out = nullptr;                                                    // host table of l.n entries, all -1 before the search
    enum { EMPTY, LAUNCH, HOST } kind = EMPTY;                                 // HOST: bow_host_select (a node beyond the lanes' reach, or forced)
    std::vector<int4> pairs;                                                   // the merge-join of :178-262: serial [x, y), lane [z, w)
    std::vector<int32_t> lists;                                                // key-frame variant: filtered fv_off | fv_idx | table of l.n
    int row = 0;                                                               // its row in the device table
    size_t at_desc = 0, at_valid = 0, at_idx = 0;                              // its own side's parts in the uploaded block, in bytes
};

// the (candidate, shared node) pairs of one job: the merge-join of the two ascending node lists (:178-262).  A pair whose serial
// features are all unusable is left out (its lane-side entries stay -1, as the walk would leave them).  The job is for the launch
// unless the host selection is forced or one of its nodes is beyond the lanes' reach
static void bow_job_pairs(BowJob &j)
{
    const orbm_bow_side &s = j.s, &l = j.l;
    j.kind = BowJob::EMPTY;
    if (s.n == 0 || l.n == 0) return;
    bool host = false;
    const bool force_host = bow_force_host();
    j.pairs.reserve((size_t)std::min(s.fv_n, l.fv_n));
    for (int a = 0, b = 0; a < s.fv_n && b < l.fv_n;) {
        if (s.fv_node[a] == l.fv_node[b]) {
            const int ns = s.fv_off[a + 1] - s.fv_off[a], nl = l.fv_off[b + 1] - l.fv_off[b];
            if (ns > 0 && nl > 0) {
                host |= nl > BOW_MAX_NODE_FEATURES || force_host;
                bool usable = !s.valid;
                for (int c = s.fv_off[a]; !usable && c < s.fv_off[a + 1]; c++) usable = s.valid[s.fv_idx[c]] != 0;
                if (usable) j.pairs.push_back(make_int4(s.fv_off[a], s.fv_off[a + 1], l.fv_off[b], l.fv_off[b + 1]));
            }
            a++; b++;
        } else if (s.fv_node[a] < l.fv_node[b]) a++;   // lower_bound on an ascending list == advance
        else b++;
    }
    if (host) j.kind = BowJob::HOST;
    else if (!j.pairs.empty()) j.kind = BowJob::LAUNCH;
}

// The LAUNCH jobs of a call: one upload, one launch, one download, one synchronisation.  shared_on_lanes: every job has the same
// lane side (frame variant); otherwise every job has the same serial side (key-frame variant).
static int bow_batch_launch(orbm_matcher *m, std::vector<BowJob> &jobs, bool shared_on_lanes, float nnratio, int th)
{
    long long table = 0, nitems = 0;
    const BowJob *first = nullptr;
    for (BowJob &j : jobs) {
        if (j.kind != BowJob::LAUNCH) continue;
        if (!first) first = &j;
        j.row = (int)table;
        table += j.l.n; nitems += (long long)j.pairs.size();
        if (table > (1ll << 28) || nitems > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 table entries");
    }
    if (!first) return ORBX_OK;
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_grow(m, 0, 0, table));                // the tables live in d_out (max_pairs also sizes d_idx, which this call does not use)
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    struct Where { size_t desc, valid, idx; };     // byte offsets of a side's parts in the block
    auto add_side = [&](const orbm_bow_side &d, bool serial) {
        Where w;
        w.desc = in.parts[in.add(d.desc, (size_t)d.n * 32)].off;
        w.valid = serial && d.valid ? in.parts[in.add(d.valid, (size_t)d.n)].off : (size_t)-1;
        w.idx = in.parts[in.add(d.fv_idx, (size_t)d.fv_off[d.fv_n] * 4)].off;
        return w;
    };
    const Where shared = add_side(shared_on_lanes ? first->l : first->s, !shared_on_lanes);
    for (BowJob &j : jobs)
        if (j.kind == BowJob::LAUNCH) {
            const Where w = add_side(shared_on_lanes ? j.s : j.l, shared_on_lanes);
            j.at_desc = w.desc; j.at_valid = w.valid; j.at_idx = w.idx;
        }
    if (in.total + (size_t)nitems * sizeof(BowItem) > ((size_t)1 << 31) - 64) return mfail(ORBX_E_CAPACITY, "request beyond 2^31 bytes of input");
    std::vector<BowItem> items;
    items.reserve((size_t)nitems);
    for (const BowJob &j : jobs) {
        if (j.kind != BowJob::LAUNCH) continue;
        const Where own = {j.at_desc, j.at_valid, j.at_idx};
        const Where &ws = shared_on_lanes ? own : shared, &wl = shared_on_lanes ? shared : own;
        const int si = (int)(ws.idx / 4), li = (int)(wl.idx / 4);
        const int4 b = make_int4((int)(ws.desc / 32), (int)(wl.desc / 32), ws.valid == (size_t)-1 ? -1 : (int)ws.valid, j.row);
        for (const int4 &p : j.pairs) items.push_back({make_int4(si + p.x, si + p.y, li + p.z, li + p.w), b});
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
            for (int c = p.z; c < p.w; c++) j.out[j.l.fv_idx[c]] = dl[(size_t)j.row + j.l.fv_idx[c]];
    }
    return ORBX_OK;
}

// A HOST job: every node-mate distance on the GPU, the order-dependent selection (:199-232) on the host.  For a node of more than
// BOW_MAX_NODE_FEATURES lane-side features, and for every job under ORBM_BOW_HOST_SELECT=1.
static int bow_host_select(orbm_matcher *m, BowJob &j, float nnratio, int th)
{
    const orbm_bow_side &kf = j.s, &f = j.l;
    // queries = usable serial-side features in visiting order, each with its node's lane list [z, w)
    struct Q { int kf, z, w; };
    std::vector<Q> qs;
    std::vector<int32_t> off;
    qs.reserve((size_t)kf.n); off.reserve((size_t)kf.n + 1);
    off.push_back(0);
    long long pairs = 0;
    for (const int4 &p : j.pairs)
        for (int c = p.x; c < p.y; c++) {
            const int ikf = kf.fv_idx[c];
            if (kf.valid && !kf.valid[ikf]) continue;
            qs.push_back({ikf, p.z, p.w});
            pairs += p.w - p.z;
            off.push_back((int32_t)pairs);
        }
    const int nq = (int)qs.size();
    if (nq == 0 || pairs == 0) return ORBX_OK;
    MTRY(orbm_grow(m, 0, 0, pairs));                 // the distances come back through d_out
    // Usual case (both sides below 65536 features): the serial side's descriptor block goes up as it is and every pair is
    // (serial feature << 16 | lane feature).  Otherwise the query descriptors are compacted and the kernel finds a
    // pair's query by binary search over the offsets.
    const bool packed16 = kf.n < 65536 && f.n < 65536;
    std::vector<uint8_t> qd;
    if (!packed16) {
        qd.resize((size_t)nq * 32);
        for (int i = 0; i < nq; i++) memcpy(&qd[(size_t)i * 32], kf.desc + (size_t)qs[i].kf * 32, 32);
    }
    std::vector<int32_t> idx((size_t)pairs), dist((size_t)pairs);
    for (int i = 0; i < nq; i++) {
        const uint32_t hi = packed16 ? (uint32_t)qs[i].kf << 16 : 0u;
        int32_t *dst = idx.data() + off[i];
        for (int c = qs[i].z; c < qs[i].w; c++) *dst++ = (int32_t)(hi | (uint32_t)f.fv_idx[c]);
    }
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    MTRY(orbm_arena_begin(m));
    InBlock in(m);
    const int pq = packed16 ? in.add(kf.desc, (size_t)kf.n * 32) : in.add(qd.data(), qd.size()), pt = in.add(f.desc, (size_t)f.n * 32);
    const int pi = in.add(idx.data(), (size_t)pairs * 4), po = in.add(off.data(), packed16 ? 0 : ((size_t)nq + 1) * 4);
    MTRY(in.upload(s));
    if (packed16)
        hipLaunchKernelGGL(k_dist_pairs16, dim3((unsigned)((pairs + M_THREADS - 1) / M_THREADS)), dim3(M_THREADS), 0, s,
                           in.at<uint8_t>(pq), in.at<uint8_t>(pt), in.at<uint32_t>(pi), (int)pairs, m->d_out);
    else
        orbm_launch_dist_csr(in.at<uint8_t>(pq), nq, in.at<uint8_t>(pt), in.at<int32_t>(po), in.at<int32_t>(pi), (int)pairs, m->d_out, s);
    MHIPCHK(hipGetLastError());
    MTRY(orbm_d2h(m, dist.data(), m->d_out, (size_t)pairs * 4, s));
    MTRY(orbm_sync(m, s));
    for (int i = 0; i < nq; i++) {                   // sequential selection (:199-232)
        int best1 = 256, best2 = 256, bestF = -1;
        for (int c = off[i]; c < off[i + 1]; c++) {
            const int fi = packed16 ? (int)((uint32_t)idx[c] & 0xFFFFu) : idx[c];
            if (j.out[fi] >= 0) continue;                   // :209
            const int d = dist[c];
            if (d < best1) { best2 = best1; best1 = d; bestF = fi; }
            else if (d < best2) best2 = d;
        }
        if (best1 <= th && (float)best1 < nnratio * (float)best2) j.out[bestF] = qs[i].kf;
    }
    return ORBX_OK;
}

// SearchByBoW of nkf candidates against one shared side; table[c * shared->n + i], counts[c].
// kf_variant = false, (KeyFrame*, Frame&) :159-288: the candidates are the key frames (serial), the shared frame is on the lanes, and
// a row is the walk's table (frame feature -> key-frame feature).
// kf_variant = true, (KeyFrame*, KeyFrame*) :522-655, the same node-by-node scan with three differences: features of BOTH key frames
// need a usable MapPoint (:558-562, :576-580), the acceptance is the strict `bestDist1 < TH_LOW` (:598), and the table is indexed by
// the OUTER key frame's features (vpMatches12[idx1]).  The shared key frame 1 is serial; a feature of a candidate that can never be
// taken is dropped from the candidate's node lists before the scan -- skipping it inside the scan is the same thing --, the scan runs
// with th = TH_LOW - 1, and the table it returns (inner feature -> outer feature, one-to-one by vbMatched2) is inverted into the row.
// direct: the rows and counts are computed in place (the one-candidate calls); otherwise in a table of the call's own that is
// committed at the end, so that a failed call leaves the outputs as they were.  Either way nothing is written before the checks
// and the handle test have passed.
static int bow_search(orbm_matcher *m, bool kf_variant, const orbm_bow_side *shared, const orbm_bow_side *cands, int nkf, float nnratio,
                      int check_orientation, int32_t *out_table, int32_t *out_counts, bool direct)
{
    if (!cands || !shared || !out_counts) return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(bow_check_side(kf_variant ? "key frame 1" : "frame", -1, shared, kf_variant));
    for (int c = 0; c < nkf; c++) MTRY(bow_check_side(kf_variant ? "second key frame" : "key frame", c, &cands[c], kf_variant));
    const int ns = shared->n;
    if (ns > 0 && !out_table) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (nkf > (1 << 20) || (long long)nkf * ns > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 (key frame, feature) slots");

    const size_t cells = (size_t)nkf * ns;
    std::vector<int32_t> own(direct ? 0 : cells + nkf);
    int32_t *table = direct ? out_table : own.data(), *counts = direct ? out_counts : own.data() + cells;
    std::vector<BowJob> jobs((size_t)nkf);
    bool device = false;
    if (ns > 0 && shared->fv_n > 0)
        for (int c = 0; c < nkf; c++) {
            const orbm_bow_side &k = cands[c];
            BowJob &j = jobs[c];
            if (!kf_variant) {
                j.s = k; j.l = *shared;
                j.out = table + (size_t)c * ns;
            } else {
                if (k.n == 0 || k.fv_n == 0) continue;
                j.lists.resize((size_t)k.fv_n + 1 + k.fv_off[k.fv_n] + k.n);
                int32_t *off2 = j.lists.data(), *idx2 = off2 + k.fv_n + 1;
                int n2 = 0;
                off2[0] = 0;
                for (int b = 0; b < k.fv_n; b++) {          // :576-580
                    for (int e = k.fv_off[b]; e < k.fv_off[b + 1]; e++)
                        if (k.valid[k.fv_idx[e]]) idx2[n2++] = k.fv_idx[e];
                    off2[b + 1] = n2;
                }
                if (n2 == 0) continue;
                j.s = *shared; j.l = k;
                j.l.fv_off = off2; j.l.fv_idx = idx2;
                j.out = idx2 + k.fv_off[k.fv_n];
                std::fill(j.out, j.out + k.n, -1);
            }
            bow_job_pairs(j);
            device |= j.kind != BowJob::EMPTY;
        }
    if (device && !m) return orbm_no_handle();
    std::fill(table, table + cells, -1);
    std::fill(counts, counts + nkf, 0);
    if (device) {
        const int th = kf_variant ? ORBM_TH_LOW - 1 : ORBM_TH_LOW;
        MTRY(bow_batch_launch(m, jobs, !kf_variant, nnratio, th));
        for (int c = 0; c < nkf; c++) {
            BowJob &j = jobs[c];
            if (j.kind == BowJob::EMPTY) continue;
            if (j.kind == BowJob::HOST) MTRY(bow_host_select(m, j, nnratio, th));
            MTRY(bow_rotation_cull(j.s.kps, j.l.kps, j.l.n, check_orientation, j.out, &counts[c]));
            if (kf_variant) {
                int32_t *row = table + (size_t)c * ns;
                for (int i2 = 0; i2 < j.l.n; i2++)
                    if (j.out[i2] >= 0) row[j.out[i2]] = i2;
            }
        }
    }
    if (!direct) {
        if (cells) memcpy(out_table, table, cells * 4);
        memcpy(out_counts, counts, (size_t)nkf * 4);
    }
    return ORBX_OK;
}

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
extern "C" int orbm_search_by_bow(orbm_matcher *m,
                                  const uint8_t *desc_kf, const orbx_keypoint *kps_kf, int n_kf, const uint8_t *valid_kf,
                                  const int32_t *fv_kf_node, const int32_t *fv_kf_off, const int32_t *fv_kf_idx, int fv_kf_n,
                                  const uint8_t *desc_f, const orbx_keypoint *kps_f, int n_f,
                                  const int32_t *fv_f_node, const int32_t *fv_f_off, const int32_t *fv_f_idx, int fv_f_n,
                                  float nnratio, int check_orientation, int32_t *match_f, int *nmatches)
{
    const orbm_bow_side kf = {desc_kf, kps_kf, n_kf, valid_kf, fv_kf_node, fv_kf_off, fv_kf_idx, fv_kf_n};
    const orbm_bow_side f = {desc_f, kps_f, n_f, nullptr, fv_f_node, fv_f_off, fv_f_idx, fv_f_n};
    return bow_search(m, false, &f, &kf, 1, nnratio, check_orientation, match_f, nmatches, true);
}

extern "C" int orbm_search_by_bow_kf(orbm_matcher *m,
                                     const uint8_t *desc1, const orbx_keypoint *kps1, int n1, const uint8_t *valid1,
                                     const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                                     const uint8_t *desc2, const orbx_keypoint *kps2, int n2, const uint8_t *valid2,
                                     const int32_t *fv2_node, const int32_t *fv2_off, const int32_t *fv2_idx, int fv2_n,
                                     float nnratio, int check_orientation, int32_t *matches12, int *nmatches)
{
    const orbm_bow_side kf1 = {desc1, kps1, n1, valid1, fv1_node, fv1_off, fv1_idx, fv1_n};
    const orbm_bow_side kf2 = {desc2, kps2, n2, valid2, fv2_node, fv2_off, fv2_idx, fv2_n};
    return bow_search(m, true, &kf1, &kf2, 1, nnratio, check_orientation, matches12, nmatches, true);
}

extern "C" int orbm_search_by_bow_batch(orbm_matcher *m, const orbm_bow_side *kfs, int nkf, const orbm_bow_side *frame, float nnratio,
                                        int check_orientation, int32_t *match_f, int32_t *nmatches)
{
    if (nkf < 0) return mfail(ORBX_E_INVALID, "nkf=%d", nkf);
    if (nkf == 0) return ORBX_OK;
    return bow_search(m, false, frame, kfs, nkf, nnratio, check_orientation, match_f, nmatches, false);
}

extern "C" int orbm_search_by_bow_kf_batch(orbm_matcher *m, const orbm_bow_side *kf1, const orbm_bow_side *kfs2, int nkf, float nnratio,
                                           int check_orientation, int32_t *matches12, int32_t *nmatches)
{
    if (nkf < 0) return mfail(ORBX_E_INVALID, "nkf=%d", nkf);
    if (nkf == 0) return ORBX_OK;
    return bow_search(m, true, kf1, kfs2, nkf, nnratio, check_orientation, matches12, nmatches, false);
}
