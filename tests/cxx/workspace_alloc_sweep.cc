// Creation-failure sweep of the handles' device memory, streams and events (my-slam_amd/csrc/dev_buf.h and the *_workspace.cc files),
// on the CPU: this program supplies the HIP calls that code uses, backed by malloc, with counters of what is live and one
// "creation number k fails" switch over device blocks, page-locked blocks, streams and events.  Built with -fsanitize=address,undefined by tests/test_workspace_alloc.py, so a double free
// or a write through a stale pointer is reported by the sanitizer; everything else is checked here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>

#include "orbm_internal.h"
#include "orbv_internal.h"
#include "orbk_internal.h"
#include "orbx_handle.h"

// ---- the HIP calls of the workspace code ----
static int g_allocs = 0, g_fail_at = -1, g_streams = 0, g_events = 0;      // g_allocs counts every creation
static bool g_capturing = false;
static std::set<void *> g_dev, g_pin;
static int live() { return (int)(g_dev.size() + g_pin.size()); }

static hipError_t fake_alloc(std::set<void *> &pool, void **p, size_t bytes)
{
    *p = nullptr;
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    memset(*p, 0xA5, bytes);
    pool.insert(*p);
    return hipSuccess;
}
static hipError_t fake_free(std::set<void *> &pool, void *p, const char *which)
{
    if (!p) return hipSuccess;
    if (!pool.erase(p)) { printf("FAIL: %s of a block this pool does not hold\n", which); exit(1); }
    free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(g_dev, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(g_dev, p, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake_alloc(g_pin, p, bytes); }
hipError_t hipHostFree(void *p) { return fake_free(g_pin, p, "hipHostFree"); }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int)
{
    *s = nullptr;
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    *s = (hipStream_t)malloc(1); g_streams++;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { free(s); g_streams--; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int)
{
    *e = nullptr;
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    *e = (hipEvent_t)malloc(1); g_events++;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); g_events--; return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }       // no graph is captured here
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *st)
{
    *st = g_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(dst, src, bytes); return hipSuccess; }
}
// the one kernel launch of the growth paths (orbk.hip), on the CPU
hipError_t orbk_launch_compact(const int32_t *src_ids, const double *src_vals, int32_t *dst_ids, double *dst_vals,
                               const long long *plan, int nplan, hipStream_t)
{
    for (int j = 0; j < nplan; j++)
        for (long long e = 0; e < plan[3 * j + 2]; e++) {
            dst_ids[plan[3 * j + 1] + e] = src_ids[plan[3 * j] + e];
            dst_vals[plan[3 * j + 1] + e] = src_vals[plan[3 * j] + e];
        }
    return hipSuccess;
}

// the device-side functions orbx_create calls (orbx_octree.hip, orbx_describe.hip, orbx_fast.hip)
int orbx_upload_constants(const int *, const int *) { return 0; }
int orbx_selftest_fp16(void) { return 0; }
size_t orbx_octree_lds_bytes(int, int, int) { return 4096; }

#define REQUIRE(cond, ...)                                                  \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);          \
            printf(__VA_ARGS__);                                            \
            printf("\n");                                                   \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static int test_fail(int code, const char *, ...) { return code; }

// ---- the buffer type alone ----
template <class B> static void buffer_alone(const char *name)
{
    g_allocs = 0; g_fail_at = -1;
    {
        B a;
        REQUIRE(!a && a.bytes() == 0, "%s: a new buffer is empty", name);
        REQUIRE(a.grow(100, test_fail, "a") == ORBX_OK && a && a.bytes() == 100 && live() == 1, "%s: first growth", name);
        void *before = a.get();
        REQUIRE(a.grow(50, test_fail, "a") == ORBX_OK && a.get() == before && g_allocs == 1, "%s: a smaller request allocates nothing", name);
        g_fail_at = g_allocs;
        REQUIRE(a.grow(200, test_fail, "a") == ORBX_E_HIP, "%s: failed growth returns ORBX_E_HIP", name);
        REQUIRE(!a && a.get() == nullptr && a.bytes() == 0 && a.count() == 0 && live() == 0, "%s: failed growth leaves the buffer empty", name);
        g_fail_at = -1;
        REQUIRE(a.grow(200, test_fail, "a") == ORBX_OK && a && a.bytes() == 200 && live() == 1, "%s: the next growth succeeds", name);
        B b(std::move(a));
        REQUIRE(!a && a.bytes() == 0 && b && b.bytes() == 200 && live() == 1, "%s: a moved-from buffer is empty", name);
        B c;
        REQUIRE(c.grow(10, test_fail, "c") == ORBX_OK && live() == 2, "%s: second buffer", name);
        c = std::move(b);
        REQUIRE(!b && b.bytes() == 0 && c.bytes() == 200 && live() == 1, "%s: move assignment frees the target's block", name);
        c.reset(); c.reset();
        REQUIRE(!c && live() == 0, "%s: reset", name);
        REQUIRE(c.grow(30, test_fail, "c") == ORBX_OK && live() == 1, "%s: growth after reset", name);
    }
    REQUIRE(live() == 0, "%s: %d live blocks after the buffers went out of scope", name, live());
}

static bool nothing_live() { return live() == 0 && g_streams == 0 && g_events == 0; }

// ---- the sweep: `call` on a fresh handle without failure (N creations), then with creation k failing for every k < N ----
template <class H>
static void sweep(const char *name, std::function<H *()> make, std::function<int(H *)> call, std::function<void(H *)> coherent,
                  std::function<void(H *)> full, std::function<void(H *)> destroy)
{
    g_fail_at = -1;
    H *h = make();
    g_allocs = 0;
    REQUIRE(call(h) == ORBX_OK, "%s without a failure", name);
    const int N = g_allocs;
    REQUIRE(N > 0, "%s allocates nothing: the case does not reach the growth", name);
    coherent(h); full(h);
    g_allocs = 0;
    REQUIRE(call(h) == ORBX_OK && g_allocs == 0, "%s: the same call again allocates nothing", name);
    destroy(h);
    REQUIRE(nothing_live(), "%s: %d live blocks, %d streams, %d events after destroy", name, live(), g_streams, g_events);
    for (int k = 0; k < N; k++) {
        h = make();
        g_allocs = 0; g_fail_at = k;
        const int rc = call(h);
        g_fail_at = -1;
        REQUIRE(rc == ORBX_E_HIP, "%s with allocation %d of %d failing returned %d", name, k, N, rc);
        coherent(h);
        REQUIRE(call(h) == ORBX_OK, "%s repeated after failure %d of %d", name, k, N);
        coherent(h); full(h);
        g_allocs = 0;
        REQUIRE(call(h) == ORBX_OK && g_allocs == 0, "%s, failure %d: a third call creates nothing", name, k);
        destroy(h);
        REQUIRE(nothing_live(), "%s, failure %d: %d live blocks, %d streams, %d events after destroy", name, k, live(), g_streams, g_events);
    }
    printf("ok %-22s %d creations swept\n", name, N);
}

// ---- matcher ----
static int grid_count(const orbm_matcher *m) { return m->grid_ok ? m->grid.n : -1; }     // orbm_grid_count (orbm_grid.hip)
static void matcher_coherent(orbm_matcher *m)
{
    const size_t q = (size_t)m->max_q(), t = (size_t)m->max_t(), p = (size_t)m->max_pairs();
    REQUIRE(q * 32 <= m->d_q.bytes() && (q == 0 || (q + 1) * 4 <= m->d_off.bytes()), "max_q %zu beyond d_q / d_off", q);
    REQUIRE(t * 32 <= m->d_t.bytes(), "max_t %zu beyond d_t", t);
    REQUIRE(p * 4 <= m->d_idx.bytes(), "max_pairs %zu beyond d_idx", p);
    REQUIRE(std::max(3 * q, p) * 4 <= m->d_out.bytes(), "d_out holds %zu bytes for max_q %zu, max_pairs %zu", m->d_out.bytes(), q, p);
    REQUIRE(m->arena_cap() <= m->arena.bytes() && m->arena_cap() <= m->d_arena.bytes(), "arena capacity beyond its blocks");
    const OrbmGrid *g[2] = {&m->grid, &m->grid2};
    for (int s = 0; s < 2; s++) {
        if (!m->grid_mem[s]) {
            REQUIRE(!g[s]->kx && !g[s]->ky && !g[s]->koct && !g[s]->cell_start && !g[s]->items && !g[s]->cell_of, "grid slot %d: arrays without a block", s);
            REQUIRE(!(s ? m->grid2_ok : m->grid_ok), "grid slot %d is marked as built without its arrays", s);
        } else {
            const uint8_t *lo = m->grid_mem[s].get(), *hi = lo + m->grid_mem[s].bytes();
            const void *arr[5] = {g[s]->kx, g[s]->ky, g[s]->koct, g[s]->items, g[s]->cell_of};
            for (const void *a : arr) REQUIRE((const uint8_t *)a >= lo && (const uint8_t *)a + t * 4 <= hi, "grid slot %d: an array of max_t outside its block", s);
            REQUIRE((const uint8_t *)g[s]->cell_start >= lo && (const uint8_t *)(g[s]->cell_start + ORBM_GRID_CELLS + 1) <= hi, "grid slot %d: cell_start outside its block", s);
        }
    }
}
static orbm_matcher *make_matcher(int q, int t, int p, bool with_grid)
{
    orbm_matcher *m = nullptr;
    REQUIRE(orbm_create(&m, 0, q, t, p) == ORBX_OK && m, "orbm_create: %s", orbm_last_error());
    if (with_grid) {      // a built grid, as orbm_grid_build leaves it
        REQUIRE(orbm_grid_ensure(m, 0) == ORBX_OK && orbm_grid_ensure(m, 1) == ORBX_OK, "grid: %s", orbm_last_error());
        m->grid.n = m->grid2.n = t; m->grid_ok = m->grid2_ok = true;
    }
    return m;
}
static void matcher_cases()
{
    auto destroy = [](orbm_matcher *m) { orbm_destroy(m); };
    sweep<orbm_matcher>("orbm_reserve", [] { return make_matcher(1, 1, 0, true); },
        [](orbm_matcher *m) { return orbm_reserve(m, 100, 200, 5000); }, matcher_coherent,
        [](orbm_matcher *m) {
            REQUIRE(m->max_q() >= 100 && m->max_t() >= 200 && m->max_pairs() >= 5000, "capacities %d %d %d", m->max_q(), m->max_t(), m->max_pairs());
            REQUIRE(grid_count(m) == -1 && !m->grid2_ok, "growing max_train drops both grids");
        }, destroy);
    sweep<orbm_matcher>("orbm_grow", [] { return make_matcher(1, 1, 0, true); },
        [](orbm_matcher *m) { return orbm_grow(m, 40, 48, 120); }, matcher_coherent,
        [](orbm_matcher *m) {
            REQUIRE(m->max_q() >= 40 && m->max_t() >= 48 && m->max_pairs() >= 120, "capacities %d %d %d", m->max_q(), m->max_t(), m->max_pairs());
            REQUIRE(grid_count(m) == -1 && !m->grid2_ok, "growing max_train drops both grids");
        }, destroy);
    sweep<orbm_matcher>("grid ensure", [] { return make_matcher(4, 50, 0, false); },
        [](orbm_matcher *m) { MTRY(orbm_grid_ensure(m, 0)); return orbm_grid_ensure(m, 1); }, matcher_coherent,
        [](orbm_matcher *m) { REQUIRE(m->grid_mem[0] && m->grid_mem[1] && grid_count(m) == -1, "both slots allocated, none built"); }, destroy);
    sweep<orbm_matcher>("ensure_partials", [] { return make_matcher(1, 1, 0, false); },
        [](orbm_matcher *m) { return orbm_ensure_partials(m, 1000, m->stream); }, matcher_coherent,
        [](orbm_matcher *m) { REQUIRE(m->d_part.count() >= 1000, "partials %zu", m->d_part.count()); }, destroy);
    sweep<orbm_matcher>("dd_scratch growth", [] { return make_matcher(1, 1, 0, false); },
        [](orbm_matcher *m) { return orbm_ensure_dd(m, 5000, nullptr); }, matcher_coherent,
        [](orbm_matcher *m) { REQUIRE(m->d_dd.bytes() >= 5000, "scratch %zu", m->d_dd.bytes()); }, destroy);
    sweep<orbm_matcher>("orbm_arena_begin", [] { return make_matcher(1, 1, 0, false); },
        [](orbm_matcher *m) { if (m->arena_cap() < 1000) m->arena_want = 1000; return orbm_arena_begin(m); }, matcher_coherent,
        [](orbm_matcher *m) { REQUIRE(m->arena_cap() >= 1000 && m->arena_used == 0 && m->arena_want == 0, "arena %zu", m->arena_cap()); }, destroy);

    // the capture refusal: one helper, two messages, no allocation and no change
    orbm_matcher *m = make_matcher(1, 1, 0, false);
    g_capturing = true; g_allocs = 0;
    REQUIRE(orbm_ensure_partials(m, 10, m->stream) == ORBX_E_INVALID, "partials grow inside a capture");
    REQUIRE(strstr(orbm_last_error(), "the matcher's partial buffer must grow (0 -> 10 pairs) while the stream is being captured"), "%s", orbm_last_error());
    REQUIRE(orbm_ensure_dd(m, 10, m->stream) == ORBX_E_INVALID, "scratch grows inside a capture");
    REQUIRE(strstr(orbm_last_error(), "the matcher's MapPoint scratch must grow (0 -> 10 bytes) while the stream is being captured"), "%s", orbm_last_error());
    REQUIRE(g_allocs == 0, "a refused growth allocates nothing");
    g_capturing = false;
    orbm_destroy(m);
    REQUIRE(live() == 0 && g_streams == 0, "capture refusal: leak");
}

// ---- vocabulary ----
static void vocabulary_case()
{
    sweep<orbv_vocabulary>("orbv feature buffers",
        [] { orbv_vocabulary *v = new orbv_vocabulary(); REQUIRE(hipStreamCreateWithFlags(&v->stream, 0) == hipSuccess, "stream"); return v; },
        [](orbv_vocabulary *v) { return orbv_ensure_feat(v, 300); },
        [](orbv_vocabulary *v) {
            const size_t c = v->cap_feat();
            REQUIRE(c * 32 <= v->d_feat.bytes() && c * 16 <= v->d_out_i.bytes() && c * 48 <= v->h_pin.bytes(), "cap_feat %zu beyond its buffers", c);
        },
        [](orbv_vocabulary *v) { REQUIRE(v->cap_feat() >= 300, "cap_feat %zu", v->cap_feat()); },
        [](orbv_vocabulary *v) { orbv_destroy(v); });
}

// ---- keyframe database ----
static orbk_database *make_db(bool filled)
{
    orbk_database *db = nullptr;
    REQUIRE(orbk_create(&db, 0, 1000, ORBV_L1_NORM, 0, 0) == ORBX_OK && db, "orbk_create: %s", orbk_last_error());
    if (!filled) return db;
    // four key frames of 60 words each as orbk_add leaves them (minimum capacities: 4 slots, 256 entries), the second erased
    for (int s = 0; s < 4; s++) {
        for (int e = 0; e < 60; e++) { db->d_ids[60 * s + e] = 1000 * s + e; db->d_vals[60 * s + e] = s + e / 64.0; }
        db->d_slots[s] = KSlotDev{60ll * s, 60, 0};
        db->slots.push_back(KSlot{(uint64_t)(10 + s), 60ll * s, 60, true, &db->state[10 + s]});
        db->slot_of[10 + s] = s;
    }
    db->tail = 240; db->live_entries = 240; db->nlive = 4;
    db->slots[1].live = false; db->d_slots[1].len = 0; db->slot_of.erase(11); db->live_entries -= 60; db->nlive--;
    return db;
}
static void db_coherent(orbk_database *db)
{
    REQUIRE((size_t)db->cap_entries() * 4 <= db->d_ids.bytes() && (size_t)db->cap_entries() * 8 <= db->d_vals.bytes(), "cap_entries beyond the arena");
    REQUIRE((size_t)db->cap_slots() * sizeof(KSlotDev) <= db->d_slots.bytes(), "cap_slots beyond the table");
    REQUIRE(db->cap_io() <= db->d_io.bytes() && db->cap_io() <= db->h_io.bytes(), "cap_io beyond its blocks");
    REQUIRE((long long)db->slots.size() <= db->cap_slots() && db->tail <= db->cap_entries(), "slots beyond the capacity");
    // every live key frame's words are where its slot says, whether or not the arena has moved
    for (size_t i = 0; i < db->slots.size(); i++) {
        const KSlot &s = db->slots[i];
        if (!s.live) continue;
        const int orig = (int)s.id - 10;
        REQUIRE(db->slot_of.count(s.id) && db->slot_of[s.id] == (int)i, "slot_of[%d]", (int)s.id);
        REQUIRE(db->d_slots[i].off == s.off && db->d_slots[i].len == s.len, "device slot %zu", i);
        for (int e = 0; e < s.len; e++)
            REQUIRE(db->d_ids[s.off + e] == 1000 * orig + e && db->d_vals[s.off + e] == orig + e / 64.0, "key frame %d entry %d", (int)s.id, e);
    }
}
static void database_cases()
{
    auto destroy = [](orbk_database *db) { orbk_destroy(db); };
    sweep<orbk_database>("orbk ensure_io", [] { return make_db(false); }, [](orbk_database *db) { return orbk_ensure_io(db, 1000); }, db_coherent,
        [](orbk_database *db) { REQUIRE(db->cap_io() >= 1000, "cap_io %zu", db->cap_io()); }, destroy);
    sweep<orbk_database>("orbk make_room", [] { return make_db(true); }, [](orbk_database *db) { return orbk_make_room(db, 30); }, db_coherent,
        [](orbk_database *db) {
            REQUIRE(db->slots.size() == 3 && db->nlive == 3 && db->tail == 180, "compaction keeps the three live key frames: %zu slots, tail %lld", db->slots.size(), db->tail);
            REQUIRE(db->slots[0].id == 10 && db->slots[1].id == 12 && db->slots[2].id == 13, "add order kept");
            REQUIRE((int)db->slots.size() < db->cap_slots() && db->tail + 30 <= db->cap_entries(), "room for one more slot of 30");
        }, destroy);
}

// ---- extractor: 1000 features, 8 levels, at most 2 frames of 322 x 241 ----
static int create_extractor(orbx_extractor **h) { return orbx_create(h, 1000, 1.2f, 8, 20, 7, 0, 322, 241, 2); }
static orbx_extractor *make_extractor()
{
    orbx_extractor *h = nullptr;
    REQUIRE(create_extractor(&h) == ORBX_OK && h, "orbx_create: %s", orbx_last_error());
    return h;
}
template <class T, bool P> static bool inside(const DevBuf<T, P> &b, const void *p, size_t bytes)
{
    const uint8_t *lo = (const uint8_t *)b.get(), *q = (const uint8_t *)p;
    return lo && q >= lo && q + bytes <= lo + b.bytes();
}
static void extractor_coherent(orbx_extractor *h)
{
    const size_t B = (size_t)h->max_batch, LV = B * ORBX_MAX_LEVELS * 4, n = B * h->max_plan.out_cap;
    const OrbxPlan &M = h->max_plan;
    const OrbxWork &w = h->work;
    REQUIRE(inside(h->w_cand, w.cand, B * M.cand_frame * sizeof(OrbxCand)) && inside(h->w_owner, w.owner, B * M.cand_frame * 4), "work.cand / owner outside their blocks");
    REQUIRE(inside(h->w_arena, w.arena, B * M.arena_frame * sizeof(OrbxNode)) && inside(h->w_sel, w.sel, B * M.list_frame * sizeof(OrbxCand)), "work.arena / sel outside their blocks");
    REQUIRE(inside(h->w_cand_count, w.cand_count, LV * ORBX_CNT_STRIDE) && inside(h->w_nk, w.nk, LV) && inside(h->w_ncand, w.ncand, LV) && inside(h->w_errflags, w.errflags, B * 4),
            "work counters outside their blocks");
    REQUIRE(inside(h->d_out, h->d_counts, B * 4) && inside(h->d_out, h->d_status, B * 4) && inside(h->d_out, h->d_kps, n * sizeof(orbx_keypoint)) && inside(h->d_out, h->d_desc, n * 32),
            "device output views outside d_out");
    REQUIRE(inside(h->h_out, h->h_counts, B * 4) && inside(h->h_out, h->h_status, B * 4) && inside(h->h_out, h->h_kps, n * sizeof(orbx_keypoint)) && inside(h->h_out, h->h_desc, n * 32),
            "host output views outside h_out");
    REQUIRE(!h->d_color == !h->h_color && h->d_color.bytes() == h->h_color.bytes(), "colour buffers: both or neither");
    size_t nup = 0, ndone = 0, nring = 0;
    for (const OrbxChunkEvents &p : h->chunk_ev) { nup += p.up.get() != nullptr; ndone += p.done.get() != nullptr; }
    REQUIRE(nup == ndone && nup == h->chunk_ev.size(), "%zu upload events, %zu completion events", nup, ndone);
    for (const OrbxRingSlot &r : h->ring) for (const DevEvent &e : r.e) nring += e.get() != nullptr;
    REQUIRE(nring == 0 || nring == 5 * ORBX_PROF_RING, "%zu of the ring's events exist", nring);
    REQUIRE(h->profiling != 2 || nring == 5 * ORBX_PROF_RING, "ring profiling is on without its events");
}
static void extractor_cases()
{
    // orbx_create: count its creations, then fail each
    g_fail_at = -1; g_allocs = 0;
    orbx_extractor *h = make_extractor();
    const int N = g_allocs, blocks = live(), streams = g_streams, events = g_events;
    extractor_coherent(h);
    orbx_destroy(h);
    REQUIRE(nothing_live(), "orbx_create + orbx_destroy: %d live blocks, %d streams, %d events", live(), g_streams, g_events);
    REQUIRE(N == blocks + streams + events && blocks > 0 && streams > 0 && events > 0, "%d creations: %d blocks, %d streams, %d events", N, blocks, streams, events);
    for (int k = 0; k < N; k++) {
        h = (orbx_extractor *)16;
        g_allocs = 0; g_fail_at = k;
        const int rc = create_extractor(&h);
        g_fail_at = -1;
        REQUIRE(rc == ORBX_E_HIP && h == nullptr, "orbx_create with creation %d of %d failing returned %d, handle %p", k, N, rc, (void *)h);
        REQUIRE(nothing_live(), "orbx_create, failure %d: %d live blocks, %d streams, %d events", k, live(), g_streams, g_events);
    }
    printf("ok %-22s %d creations swept (%d blocks, %d streams, %d events)\n", "orbx_create", N, blocks, streams, events);

    auto destroy = [](orbx_extractor *e) { orbx_destroy(e); };
    sweep<orbx_extractor>("orbx colour buffers", make_extractor, [](orbx_extractor *e) { return orbx_ensure_color(e); }, extractor_coherent,
        [](orbx_extractor *e) { REQUIRE(e->d_color && e->h_color, "colour buffers after a successful call"); }, destroy);
    sweep<orbx_extractor>("orbx pyramid staging", make_extractor, [](orbx_extractor *e) { return orbx_ensure_pyr_staging(e, 100000); }, extractor_coherent,
        [](orbx_extractor *e) { REQUIRE(e->h_pyr.bytes() >= 100000, "staging %zu", e->h_pyr.bytes()); }, destroy);
    sweep<orbx_extractor>("orbx chunk events", make_extractor,
        [](orbx_extractor *e) { XTRY(orbx_ensure_chunk_events(e, 3)); return orbx_ensure_chunk_events(e, 5); }, extractor_coherent,
        [](orbx_extractor *e) { REQUIRE(e->chunk_ev.size() == 5, "%zu chunk event pairs", e->chunk_ev.size()); }, destroy);
    sweep<orbx_extractor>("orbx ring events", make_extractor, [](orbx_extractor *e) { return orbx_set_profiling(e, 2); }, extractor_coherent,
        [](orbx_extractor *e) { REQUIRE(e->profiling == 2 && e->ring.size() == ORBX_PROF_RING, "profiling %d, %zu ring slots", e->profiling, e->ring.size()); }, destroy);
}

int main()
{
    setvbuf(stdout, nullptr, _IONBF, 0);      // a leak report ends the process without flushing
    buffer_alone<DevBuf<int32_t>>("DevBuf");
    buffer_alone<PinBuf<uint8_t>>("PinBuf");
    printf("ok buffer type\n");
    matcher_cases();
    vocabulary_case();
    database_cases();
    extractor_cases();
    REQUIRE(nothing_live(), "%d live blocks, %d streams, %d events at exit", live(), g_streams, g_events);
    printf("sweep ok\n");
    return 0;
}
