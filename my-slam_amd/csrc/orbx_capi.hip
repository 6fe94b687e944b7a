// orbx_capi.hip -- host side of liborbx.so: the per-call path of the extractor and its C ABI.  The handle is declared in orbx_handle.h; its
// life and its lazy resources are in orbx_workspace.cc, shapes are planned in orbx_plan.cc (host arithmetic, no handle) and committed here;
// all pixel work is in the per-stage kernel files (orbx_pyramid/fast/octree/describe.hip).
#include <chrono>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "orbx_handle.h"

// A/B switches of orbx_extract_batch, read once per process
static bool batch_equal_chunks() { static const bool on = getenv("ORBX_BATCH_EQUAL") != nullptr; return on; }   // A/B switch
static int batch_streams() { static const int n = [] { const char *e = getenv("ORBX_BATCH_STREAMS"); const int v = e ? atoi(e) : 3; return v < 1 ? 1 : v > 3 ? 3 : v; }(); return n; }   // compute streams the chunks rotate over
static bool batch_trace() { static const bool on = getenv("ORBX_BATCH_TRACE") != nullptr; return on; }      // host-side time split of a call, to stderr
static bool batch_pinned_ok() { static const bool on = [] { const char *e = getenv("ORBX_BATCH_PINNED"); return !e || atoi(e) != 0; }(); return on; }   // page-locked caller memory is uploaded where it lies (0 keeps the staging copy: A/B switch)

extern "C" const char *orbx_version(void) { return "orbx 0.1 (gfx950)"; }

// Capture what `body` enqueues on s (body returns false if it failed) into an instantiated graph; null if the capture could not begin,
// the body failed or the capture was invalidated.  orbx_capture_mutex() is held for the capture; a capture that began is always ended and its
// hipGraph_t destroyed; a failure leaves no sticky error behind.  Nothing has run then: the caller runs the work plainly.
template <class Body> static DevGraphExec capture_graph(hipStream_t s, Body body)
{
    std::lock_guard<std::recursive_mutex> lk_(orbx_capture_mutex());
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
        const bool ok = body();
        hipGraph_t g = nullptr;
        if (hipStreamEndCapture(s, &g) != hipSuccess || !ok || !g || hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) != hipSuccess) exec = nullptr;
        if (g) (void)hipGraphDestroy(g);
    }
    if (!exec) (void)hipGetLastError();
    return DevGraphExec(exec);
}
// the captured graphs hold the options, the upload and (for colour) the conversion of the format they were captured with
static void drop_graphs(orbx_extractor *h)
{
    h->graph_exec.reset(); h->graph_w = h->graph_h = 0;
    h->bgraph.clear(); h->bg_w = h->bg_h = h->bg_n = 0;
}
extern "C" int orbx_set_option(orbx_extractor *h, int option, int value)
{
    if (!h) return xfail(ORBX_E_INVALID, "NULL handle");
    if (option == ORBX_OPT_BATCH_CHUNK && value >= 0 && value <= 4096) h->batch_chunk = value;
    else if (option == ORBX_OPT_BLUR_ROUNDING && (value == 0 || value == 1)) h->blur_mode = h->plan.blur_mode = value;
    else if (option == ORBX_OPT_SUBBATCHES && value >= 1 && value <= ORBX_MAX_SUB) h->nsub = value;
    else if (option == ORBX_OPT_OVERLAP_PYRAMID && (value == 0 || value == 1)) h->overlap_pyr = value;
    else return xfail(ORBX_E_INVALID, "unknown option %d=%d", option, value);
    drop_graphs(h);
    return ORBX_OK;
}
extern "C" int orbx_set_input_format(orbx_extractor *h, int format)
{
    if (!h) return xfail(ORBX_E_INVALID, "NULL handle");
    if (format < ORBX_FMT_GRAY8 || format > ORBX_FMT_RGBA8) return xfail(ORBX_E_INVALID, "unknown input format %d", format);
    if (h->inflight) return xfail(ORBX_E_INVALID, "an orbx_extract_begin call is in flight on this handle");
    if (format == h->fmt) return ORBX_OK;
    drop_graphs(h);
    h->graph_seen_w = h->graph_seen_h = 0;   // the first call in the new format runs plainly
    h->fmt = format;
    return ORBX_OK;
}
extern "C" int orbx_get_input_format(const orbx_extractor *h) { return h ? h->fmt : xfail(ORBX_E_INVALID, "NULL handle"); }

struct ColorSrc { const uint8_t *base; int stride; long long frame; };
// one colour frame must be below 2 GiB and its row stride below 8 MiB (the conversion kernel's 32-bit offsets inside a frame)
static int check_color_limits(int width, int height, int row_stride)
{
    if (row_stride >= (1 << 23) || (long long)height * row_stride >= (1ll << 31))
        return xfail(ORBX_E_SHAPE, "colour frame %dx%d with row stride %d: one frame must be below 2 GiB, the stride below 8 MiB", width, height, row_stride);
    return ORBX_OK;
}

extern "C" int orbx_get_levels(const orbx_extractor *h) { return h ? h->nlevels : 0; }
extern "C" float orbx_get_scale_factor(const orbx_extractor *h) { return h ? h->scale_factor : 0.f; }
extern "C" int orbx_get_tables(const orbx_extractor *h, float *sf, float *isf, float *s2, float *is2)
{
    if (!h) return xfail(ORBX_E_INVALID, "NULL handle");
    for (int i = 0; i < h->nlevels; i++) {
        if (sf) sf[i] = h->scale[i];
        if (isf) isf[i] = h->inv_scale[i];
        if (s2) s2[i] = h->sigma2[i];
        if (is2) is2[i] = h->inv_sigma2[i];
    }
    return ORBX_OK;
}
extern "C" int orbx_get_features_per_level(const orbx_extractor *h, int *q)
{
    if (!h || !q) return xfail(ORBX_E_INVALID, "NULL argument");
    for (int i = 0; i < h->nlevels; i++) q[i] = h->quota[i];
    return ORBX_OK;
}
extern "C" int orbx_capacity(const orbx_extractor *h) { return h ? h->max_plan.out_cap : 0; }
extern "C" int orbx_stage_ms_ring(orbx_extractor *h, float *ms, int max_calls)
{
    if (!h || !ms || max_calls < 0) return xfail(ORBX_E_INVALID, "bad argument");
    if (h->profiling != 2) return xfail(ORBX_E_INVALID, "ring profiling is off");
    const int n = (int)std::min<long long>(std::min<long long>(h->ring_calls, ORBX_PROF_RING), max_calls);
    for (int i = 0; i < n; i++) {                           // newest first
        const DevEvent *e = h->ring[(h->ring_calls - 1 - i) % ORBX_PROF_RING].e;
        for (int k = 0; k < 4; k++) HIPCHK(hipEventElapsedTime(&ms[4 * i + k], e[k], e[k + 1]));   // fails if the caller has not synchronised
    }
    return n;
}
extern "C" int orbx_last_stage_ms(orbx_extractor *h, float ms[4])
{
    if (!h || !ms) return xfail(ORBX_E_INVALID, "NULL argument");
    memcpy(ms, h->stage_ms, sizeof(float) * 4);
    return ORBX_OK;
}

// (re)plan for a frame shape; buffers stay those sized at create.  Plan, upload, commit: the handle is written only after the last
// step that can fail, so a refused shape leaves it planned for the shape it had.  A copy that fails may have left a device table
// half rewritten, which no plan describes: the one write on that path drops the current shape, so the next call plans and uploads again.
static int ensure_plan(orbx_extractor *h, int W, int H)
{
    if (W == h->cur_w && H == h->cur_h) return ORBX_OK;
    if (W > h->max_w || H > h->max_h) return xfail(ORBX_E_SHAPE, "frame %dx%d exceeds the handle's max %dx%d", W, H, h->max_w, h->max_h);
    ShapePlan S;
    std::string why;
    const int rc = orbx_plan_shape(*h, h->max_plan, W, H, &S, &why);
    if (rc != ORBX_OK) return xfail(rc, "frame %dx%d: %s", W, H, why.c_str());
    {   // a shape change rewrites tables that kernels of an earlier call may still be reading -- on the handle's stream, its aux
        // streams or a caller's stream (orbx_extract_batch_device): wait for the device, not only for h->stream (shape changes are rare)
        std::lock_guard<std::recursive_mutex> lk_(orbx_capture_mutex());
        HIPCHK(hipDeviceSynchronize());
        hipError_t e = hipSuccess;
        auto up = [&e](void *dst, const void *src, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); };
        up(h->d_bands, S.bands.data(), S.bands.size() * sizeof(int4));
        up(h->d_tiles, S.tiles.data(), S.tiles.size() * sizeof(int4));
        up(h->d_cells, S.cells.data(), (size_t)S.plan.ncells * sizeof(uint32_t));
        up(h->d_tab_i, S.tab_i.data(), S.tab_used * sizeof(int));
        up(h->d_tab_s, S.tab_s.data(), S.tab_used * sizeof(short2));
        if (e != hipSuccess) { h->cur_w = h->cur_h = 0; return xfail(ORBX_E_HIP, "table upload for %dx%d: %s", W, H, hipGetErrorString(e)); }
    }
    // commit: the plan with the device addresses filled in
    h->plan = S.plan;
    h->plan.cell_tab = h->d_cells;
    for (int l = 1; l < h->nlevels; l++) {
        h->plan.lv[l].base = h->d_pyr + h->pyr_level_off[l];
        h->tabs[l].xofs = h->d_tab_i + S.xofs_at[l]; h->tabs[l].alpha = h->d_tab_s + S.xofs_at[l];
        h->tabs[l].yofs = h->d_tab_i + S.yofs_at[l]; h->tabs[l].beta = h->d_tab_s + S.yofs_at[l];
        h->resize_mode[l] = S.resize_mode[l];
    }
    h->fuse[0] = S.fuse[0]; h->fuse[1] = S.fuse[1]; h->tile = S.tile;
    h->cur_w = W; h->cur_h = H;
    return ORBX_OK;
}

// what FuseLevel and TileLevel share
template <class U> static void fill_level(U &u, const OrbxLevel &L, const ResizeTab &tab)
{
    u.base = L.base; u.w = L.w; u.h = L.h; u.stride = L.stride; u.frame = L.frame_stride; u.tab = tab;
}
// levels 1 .. last of nf frames, one launch per level
static void launch_levels(const orbx_extractor *h, const OrbxPlan &P, int last, int nf, const uint8_t *src_end, hipStream_t s)
{
    for (int l = 1; l <= last; l++) orbx_launch_resize(P.lv[l - 1], P.lv[l], h->tabs[l], h->resize_mode[l], nf, l == 1 ? src_end : nullptr, s);
}
// build levels 1 .. L-1 of the nf frames of one sub-batch (P: its view of the plan) on stream s
static void enqueue_pyramid(const orbx_extractor *h, const OrbxPlan &P, int nf, const uint8_t *src_end, hipStream_t s)
{
    // The upper levels in one launch -- for a FEW frames only.  The resize arithmetic is ~22 vector instructions per pixel
    // and the per-level kernels of a large batch are bound by that, not by their launches (rocprofv3 + SQ_INSTS_VALU:
    // 47 % VALU-busy over the six upper levels at 64 x 640 x 480); the fused kernel recomputes the band overlaps
    // (+25 % pixels) and measured 70 us against 57 for the chain there.  With one frame the launches dominate and
    // fusing wins (28.6 -> 24.6 us at 640 x 480).  ORBX_PYRAMID_FUSE=2 forces it for A/B measurements.
    const FusePlan *F = nullptr;
    const FusePlan *cand = h->fuse[1].ok ? &h->fuse[1] : (h->fuse[0].ok ? &h->fuse[0] : nullptr);
    if (h->fuse_on == 2 && h->fuse[0].ok && (long long)h->fuse[0].nbands * nf >= 384) cand = &h->fuse[0];
    if (cand && (h->fuse_on == 2 || (long long)nf * P.lv[cand->a + 1].w * P.lv[cand->a + 1].h <= 1200000)) F = cand;
    // many frames: the upper levels as one wave per 2-D tile (k_resize_tiles); it takes precedence over the band kernel
    const bool use_tiles = h->tile.ok && h->fuse_on != 2 && nf >= h->tile_min_frames;
    if (use_tiles) F = nullptr;
    launch_levels(h, P, use_tiles ? h->tile.a : (F ? F->a : h->nlevels - 1), nf, src_end, s);
    if (use_tiles) {
        TileArgs A;
        memset(&A, 0, sizeof(A));
        A.a = h->tile.a; A.b = h->tile.b; A.ntx = h->tile.ntx; A.nty = h->tile.nty;
        for (int l = 0; l < ORBX_FUSE_MAX; l++) { A.lds_off[l] = h->tile.lds_off[l]; A.tab_off[l] = h->tile.tab_off[l]; }
        A.xr = h->d_tiles + h->tile.offx; A.yr = h->d_tiles + h->tile.offy;
        for (int l = A.a; l <= A.b; l++) fill_level(A.lv[l], P.lv[l], h->tabs[l]);
        orbx_launch_resize_tiles(A, nf, (size_t)h->tile.lds, s);
    }
    if (F) {
        FuseArgs A;
        memset(&A, 0, sizeof(A));
        A.a = F->a; A.b = F->b; A.bands = h->d_bands + F->off; A.nbands = F->nbands; A.buf0_bytes = F->buf0;
        for (int l = F->a; l <= F->b; l++) {
            FuseLevel &U = A.lv[l];
            fill_level(U, P.lv[l], h->tabs[l]);
            U.nbx = (U.w + 3) / 4;
            U.rcp_nbx = U.nbx > 1 ? (uint32_t)((1ull << 32) / (unsigned)U.nbx + 1) : 0u;
            U.pitch = (int)align_up((size_t)U.w + 12, 16);
        }
        orbx_launch_resize_fused(A, nf, (size_t)F->lds, s);
    }
}

// Sub-batches on separate streams: the quadtree and the small pyramid levels are latency-bound (few, long workgroups), so one
// half-batch's latency-bound kernels run beside the other half's VALU-bound ones.  Frames are independent, so a sub-batch is
// only a pointer offset: frames [f0, f0 + nf) of the call, its stream, its views of the plan and of the workspace.
struct SubBatch { int f0, nf; hipStream_t s; OrbxPlan plan; OrbxWork work; };
static void make_sub_batches(const orbx_extractor *h, int nframes, int nsub, int work_frame0, hipStream_t s, SubBatch *sb)
{
    const OrbxPlan &P = h->plan;
    for (int i = 0; i < nsub; i++) {
        SubBatch &B = sb[i];
        B.f0 = (int)((long long)nframes * i / nsub); B.nf = (int)((long long)nframes * (i + 1) / nsub) - B.f0;
        B.s = i == 0 ? s : h->aux[i - 1];
        B.plan = P;
        B.work = h->work;
        const long long o = (long long)work_frame0 + B.f0;
        B.plan.lv[0].base = P.lv[0].base + (long long)B.f0 * P.lv[0].frame_stride;      // d_images is this call's first frame already
        for (int l = 1; l < h->nlevels; l++) B.plan.lv[l].base = P.lv[l].base + o * P.lv[l].frame_stride;
        B.work.cand += o * P.cand_frame; B.work.owner += o * P.cand_frame; B.work.arena += o * P.arena_frame;
        B.work.sel += o * P.list_frame; B.work.nk += o * h->nlevels; B.work.ncand += o * h->nlevels; B.work.errflags += o;
        B.work.cand_count += o * h->nlevels * ORBX_CNT_STRIDE;
    }
}

// enqueue the whole pipeline for `nframes` frames already resident in HBM
static int enqueue(orbx_extractor *h, const uint8_t *d_images, int nframes, int W, int H, int row_stride,
                   long long frame_stride, orbx_keypoint *d_kps, uint8_t *d_desc, int32_t *d_counts,
                   int32_t *d_status, hipStream_t s, int work_frame0 = 0,   // work_frame0: first frame slot of the workspace / pyramid
                   const ColorSrc *cs = nullptr)   // colour: d_images is the handle's grey block, filled from *cs ahead of the pyramid
{
    int rc = ensure_plan(h, W, H);
    if (rc != ORBX_OK) return rc;
    OrbxPlan &P = h->plan;
    P.blur_mode = h->blur_mode;
    P.lv[0].base = const_cast<uint8_t *>(d_images); P.lv[0].stride = row_stride; P.lv[0].frame_stride = frame_stride;
    h->last_input = d_images; h->last_in_stride = row_stride; h->last_in_frame = frame_stride; h->last_batch = nframes;

    const bool prof = h->profiling == 1;          // mode 1 times one call in isolation; mode 2 only drops events into the stream
    const DevEvent *pe = h->profiling == 2 ? h->ring[h->ring_calls % ORBX_PROF_RING].e : (prof ? h->ev : nullptr);
    if (h->need_clear) {   // the kernels leave the counters and flags zeroed; only the first call (or one after an error) clears
        HIPCHK(hipMemsetAsync(h->work.cand_count, 0, (size_t)h->max_batch * ORBX_MAX_LEVELS * ORBX_CNT_STRIDE * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(h->work.errflags, 0, (size_t)h->max_batch * sizeof(uint32_t), s));
        h->need_clear = false;
    }
    struct DirtyGuard { orbx_extractor *h; bool ok = false; ~DirtyGuard() { if (!ok) h->need_clear = true; } } guard{h};
    const uint8_t *src_end = nullptr;   // level 0 in caller memory has no slack behind its last byte
    if (d_images < h->d_input || d_images >= h->d_input + (size_t)h->max_batch * h->in_frame)   // the handle's own input block has slack
        src_end = d_images + (long long)(nframes - 1) * frame_stride + (long long)(H - 1) * row_stride + W;

    const int nsub = (h->profiling != 0 || nframes < 16) ? 1 : std::min(h->nsub, ORBX_MAX_SUB);
    SubBatch sb[ORBX_MAX_SUB];
    make_sub_batches(h, nframes, nsub, work_frame0, s, sb);
    if (cs) {   // the conversion is part of stage [0]; it runs on s ahead of the fork, so every sub-batch sees its grey frames
        if (pe) HIPCHK(hipEventRecord(pe[0], s));
        orbx_launch_color(cs->base, cs->stride, cs->frame, const_cast<uint8_t *>(d_images), row_stride, frame_stride, W, H, nframes, h->fmt, s);
    }
    if (nsub > 1) {
        HIPCHK(hipEventRecord(h->ev_fork, s));
        for (int i = 1; i < nsub; i++) HIPCHK(hipStreamWaitEvent(sb[i].s, h->ev_fork, 0));
    }
    if (pe && !cs) HIPCHK(hipEventRecord(pe[0], s));
    // FAST on level 0 needs only the input, so with one sub-batch the resize chain (seven small, latency-bound
    // launches) runs on a side stream underneath it; the remaining levels' cells wait for the chain.
    const bool overlap = h->profiling == 0 && nsub == 1 && h->overlap_pyr && h->nlevels > 1 && P.lv[1].cell_begin > 0;
    if (overlap) {
        hipStream_t sa = h->aux[ORBX_MAX_SUB - 2];
        HIPCHK(hipEventRecord(h->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(sa, h->ev_fork, 0));
        launch_levels(h, sb[0].plan, h->nlevels - 1, nframes, src_end, sa);
        HIPCHK(hipEventRecord(h->ev_join[ORBX_MAX_SUB - 2], sa));
        orbx_launch_fast(sb[0].plan, sb[0].work, nframes, 0, P.lv[1].cell_begin, s);
        HIPCHK(hipStreamWaitEvent(s, h->ev_join[ORBX_MAX_SUB - 2], 0));
        orbx_launch_fast(sb[0].plan, sb[0].work, nframes, P.lv[1].cell_begin, P.ncells, s);
    } else {
        for (int i = 0; i < nsub; i++) enqueue_pyramid(h, sb[i].plan, sb[i].nf, src_end, sb[i].s);
        if (pe) HIPCHK(hipEventRecord(pe[1], s));
        for (int i = 0; i < nsub; i++) orbx_launch_fast(sb[i].plan, sb[i].work, sb[i].nf, 0, P.ncells, sb[i].s);
    }
    if (pe) HIPCHK(hipEventRecord(pe[2], s));
    // dynamic LDS of the quadtree launch: the list arrays for the handle's largest list + this shape's fast-forward tables
    size_t lds = orbx_octree_lds_bytes(h->oct_cap_max, P.oct_ft, P.oct_map);
    const bool plain = lds > 150 * 1024;         // no room for the tables beside very long lists: plain passes
    if (plain) lds = orbx_octree_lds_bytes(h->oct_cap_max, 0, 0);
    for (int i = 0; i < nsub; i++) {
        OrbxPlan &Q = sb[i].plan;
        if (plain) { Q.oct_ft = 0; Q.oct_map = 0; for (int l = 0; l < h->nlevels; l++) Q.lv[l].fastD = 0; }
        Q.oct_cap_max = h->oct_cap_max;
        orbx_launch_octree(Q, sb[i].work, sb[i].nf, lds, sb[i].s);
    }
    if (pe) HIPCHK(hipEventRecord(pe[3], s));
    for (int i = 0; i < nsub; i++)
        orbx_launch_describe(sb[i].plan, sb[i].work, sb[i].nf, d_kps + (long long)sb[i].f0 * P.out_cap,
                             d_desc + (long long)sb[i].f0 * P.out_cap * 32, d_counts + sb[i].f0, d_status + sb[i].f0, sb[i].s);
    if (pe) HIPCHK(hipEventRecord(pe[4], s));
    for (int i = 1; i < nsub; i++) {
        HIPCHK(hipEventRecord(h->ev_join[i - 1], sb[i].s));
        HIPCHK(hipStreamWaitEvent(s, h->ev_join[i - 1], 0));
    }
    HIPCHK(hipGetLastError());
    if (h->profiling == 2) h->ring_calls++;
    guard.ok = true;
    return ORBX_OK;
}

static int finish_profile(orbx_extractor *h)
{
    if (h->profiling != 1) return ORBX_OK;
    HIPCHK(hipEventSynchronize(h->ev[4]));
    for (int i = 0; i < 4; i++) HIPCHK(hipEventElapsedTime(&h->stage_ms[i], h->ev[i], h->ev[i + 1]));
    return ORBX_OK;
}

extern "C" int orbx_extract_batch_device(orbx_extractor *h, const uint8_t *d_images, int nframes, int width,
                                         int height, int row_stride, size_t frame_stride,
                                         orbx_keypoint *d_keypoints, uint8_t *d_descriptors, int cap,
                                         int32_t *d_counts, int32_t *d_status, void *hip_stream)
{
    if (!h) return xfail(ORBX_E_INVALID, "NULL handle");
    if (h->inflight) return xfail(ORBX_E_INVALID, "an orbx_extract_begin call is in flight on this handle (its workspace would be overwritten)");
    if (!d_images || !d_keypoints || !d_descriptors || !d_counts || !d_status) return xfail(ORBX_E_INVALID, "NULL device pointer");
    if (nframes < 1 || nframes > h->max_batch) return xfail(ORBX_E_INVALID, "nframes=%d (max_batch=%d)", nframes, h->max_batch);
    const int cn = orbx_format_channels(h->fmt);
    if (width < 1 || height < 1 || row_stride / cn < width) return xfail(ORBX_E_INVALID, "bad frame geometry %dx%d stride %d (%d channel%s)", width, height, row_stride, cn, cn > 1 ? "s" : "");
    // the kernels index one frame with 31-bit byte offsets and 24-bit row strides
    if (row_stride >= (1 << 23) || (long long)height * row_stride >= (1ll << 31))
        return xfail(ORBX_E_SHAPE, "frame %dx%d with row stride %d: one frame must be below 2 GiB, the stride below 8 MiB", width, height, row_stride);
    if (cap != h->max_plan.out_cap) return xfail(ORBX_E_CAPACITY, "device outputs must be laid out with cap == orbx_capacity() == %d (got %d)", h->max_plan.out_cap, cap);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    int rc;
    if (cn > 1) {   // the caller's buffer is read by the conversion only; level 0 is the handle's grey block
        const ColorSrc cs = {d_images, row_stride, (long long)frame_stride};
        rc = enqueue(h, h->d_input, nframes, width, height, h->in_stride, (long long)h->in_frame, d_keypoints, d_descriptors, d_counts, d_status, s, 0, &cs);
    } else
        rc = enqueue(h, d_images, nframes, width, height, row_stride, (long long)frame_stride, d_keypoints,
                     d_descriptors, d_counts, d_status, s);
    if (rc != ORBX_OK) return rc;
    if (h->profiling == 1) return finish_profile(h);
    return ORBX_OK;
}

// repack frames [k0, k1) into the pinned staging buffer with the aligned pitch (a pitched hipMemcpy2D of a 1241-byte-wide image
// costs ~3 ms; this and ONE contiguous copy cost ~0.1 ms); rows are dealt to the staging threads in blocks
// Is [p, p + bytes) page-locked host memory (hipHostMalloc / hipHostRegister)?  Then the DMA engine can read it where it lies and
// the repack into the handle's pinned staging block -- 0.23 ms of the calling thread for 64 VGA frames -- is skipped.
static bool is_pinned_range(const void *p, size_t bytes)
{
    hipPointerAttribute_t a0, a1;
    if (hipPointerGetAttributes(&a0, p) != hipSuccess || hipPointerGetAttributes(&a1, (const uint8_t *)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary (pageable) pointer is "invalid value" to the runtime: not an error of this call
        return false;
    }
    return a0.type == hipMemoryTypeHost && a1.type == hipMemoryTypeHost;
}
// every frame's first and last byte is checked: frames carved out of several page-locked allocations with pageable gaps between
// them would pass a test of the block's two ends only (the copies are issued per frame or per chunk, never across such a gap
// unless the frames are contiguous -- and contiguous frames inside one registered range are what the per-frame test confirms)
static bool is_pinned_host(const uint8_t *images, int nframes, size_t frame_stride, size_t frame_bytes)
{
    for (int k = 0; k < nframes; k++)
        if (!is_pinned_range(images + (size_t)k * frame_stride, frame_bytes)) return false;
    return true;
}

// upload frames [k0, k1) straight from the caller's page-locked buffer into the handle's input block (rows are re-pitched by the copy)
// (d_dst, dst_stride, dst_frame: that block and its pitches; row_bytes = width * channels)
static int upload_pinned(uint8_t *d_dst, size_t dst_stride, size_t dst_frame, const uint8_t *images, int k0, int k1, size_t row_bytes, int height, int row_stride, size_t frame_stride, hipStream_t s)
{
    const bool tall = frame_stride == (size_t)row_stride * height && dst_frame == dst_stride * height;   // the chunk is one tall image
    if (tall) {
        HIPCHK(hipMemcpy2DAsync(d_dst + (size_t)k0 * dst_frame, dst_stride, images + (size_t)k0 * frame_stride, (size_t)row_stride,
                                row_bytes, (size_t)height * (k1 - k0), hipMemcpyHostToDevice, s));
    } else {
        for (int k = k0; k < k1; k++)
            HIPCHK(hipMemcpy2DAsync(d_dst + (size_t)k * dst_frame, dst_stride, images + (size_t)k * frame_stride, (size_t)row_stride,
                                    row_bytes, (size_t)height, hipMemcpyHostToDevice, s));
    }
    return ORBX_OK;
}
// where the host entry points stage and upload a call's frames: the grey input block, or the colour block with the call's own pitches
struct StageGeom { uint8_t *h_base, *d_base; size_t stride, frame, row_bytes; };
static StageGeom stage_geom(const orbx_extractor *h, int width, int height)
{
    const int cn = orbx_format_channels(h->fmt);
    if (cn == 1) return {h->h_in, h->d_input, (size_t)h->in_stride, h->in_frame, (size_t)width};
    return {h->h_color, h->d_color, (size_t)color_pitch(width, cn), color_frame(width, height, cn), (size_t)width * cn};
}

static void stage_frames(orbx_extractor *h, const StageGeom &G, const uint8_t *images, int k0, int k1, int height, int row_stride, size_t frame_stride)
{
    const int RB = 64, nblk = (height + RB - 1) / RB;
    auto unit = [&](int u) {
        const int k = k0 + u / nblk, y0 = (u % nblk) * RB, y1 = std::min(height, y0 + RB);
        uint8_t *dst = G.h_base + (size_t)k * G.frame;
        const uint8_t *src = images + (size_t)k * frame_stride;
        if ((size_t)row_stride == G.stride) memcpy(dst + (size_t)y0 * row_stride, src + (size_t)y0 * row_stride, (size_t)row_stride * (y1 - y0 - 1) + G.row_bytes);
        else for (int y = y0; y < y1; y++) memcpy(dst + (size_t)y * G.stride, src + (size_t)y * row_stride, G.row_bytes);
    };
    const int n = (k1 - k0) * nblk;
    if (h->pool) h->pool->parallel_for(n, unit);
    else for (int u = 0; u < n; u++) unit(u);
}

static const char *device_status_text(int st)
{
    return st == ORBX_E_CAND_OVERFLOW ? "FAST candidate buffer overflow" : st == ORBX_E_TREE_OVERFLOW ? "quadtree arena overflow" : "capacity";
}
// the staging outputs of the first nframes frames, device to pinned host: the whole block in one copy when it is full
static int download_outputs(orbx_extractor *h, int nframes, hipStream_t s)
{
    if (nframes == h->max_batch) {
        HIPCHK(hipMemcpyAsync(h->h_out, h->d_out, h->d_out.bytes(), hipMemcpyDeviceToHost, s));
    } else {
        const size_t n = (size_t)h->max_plan.out_cap * nframes;
        HIPCHK(hipMemcpyAsync(h->h_out, h->d_out, h->out_hdr, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h->h_kps, h->d_kps, sizeof(orbx_keypoint) * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h->h_desc, h->d_desc, 32 * n, hipMemcpyDeviceToHost, s));
    }
    return ORBX_OK;
}

// hand frames [k0, k1) over to the caller; hc / hs / hk / hd = counts, status, keypoints, descriptors of frame k0 in pinned memory
static int deliver_batch(orbx_extractor *h, int k0, int k1, orbx_keypoint *keypoints, uint8_t *descriptors, int cap, int *counts,
                         const int32_t *hc, const int32_t *hs, const orbx_keypoint *hk, const uint8_t *hd)
{
    const int ocap = h->max_plan.out_cap;
    for (int k = k0; k < k1; k++) {
        const int st = hs[k - k0];
        if (st != ORBX_OK) return xfail(st, "frame %d: device status %d (%s)", k, st, device_status_text(st));
        if (hc[k - k0] > cap) return xfail(ORBX_E_CAPACITY, "frame %d produced %d keypoints, caller capacity %d (use orbx_capacity())", k, hc[k - k0], cap);
    }
    auto unit = [&](int u) {
        const int k = k0 + u, n = hc[u];
        memcpy(keypoints + (size_t)k * cap, hk + (size_t)u * ocap, sizeof(orbx_keypoint) * n);
        memcpy(descriptors + (size_t)k * cap * 32, hd + (size_t)u * ocap * 32, (size_t)32 * n);
        counts[k] = n;
    };
    if (h->pool && k1 - k0 >= 8) h->pool->parallel_for(k1 - k0, unit);
    else for (int u = 0; u < k1 - k0; u++) unit(u);
    return ORBX_OK;
}

// the pipeline for frames [k0, k0 + nf) of the handle's staged-and-uploaded block (grey: the input block itself; colour: converted into it)
static int enqueue_staged(orbx_extractor *h, const StageGeom &G, int k0, int nf, int width, int height, orbx_keypoint *d_kps, uint8_t *d_desc,
                          int32_t *d_counts, int32_t *d_status, hipStream_t s)
{
    const ColorSrc cs = {G.d_base + (size_t)k0 * G.frame, (int)G.stride, (long long)G.frame};
    return enqueue(h, h->d_input + (size_t)k0 * h->in_frame, nf, width, height, h->in_stride, (long long)h->in_frame, d_kps, d_desc, d_counts, d_status, s, k0,
                   h->fmt == ORBX_FMT_GRAY8 ? nullptr : &cs);
}

// The whole batch in one piece: upload, kernels, download, strictly one after the other (first call of a shape, profiling,
// small batches).
static int extract_batch_simple(orbx_extractor *h, const uint8_t *images, int nframes, int width, int height, int row_stride,
                                size_t frame_stride, orbx_keypoint *keypoints, uint8_t *descriptors, int cap, int *counts)
{
    hipStream_t s = h->stream;
    const StageGeom G = stage_geom(h, width, height);
    stage_frames(h, G, images, 0, nframes, height, row_stride, frame_stride);
    HIPCHK(hipMemcpyAsync(G.d_base, G.h_base, (size_t)(nframes - 1) * G.frame + G.stride * height, hipMemcpyHostToDevice, s));
    int rc = enqueue_staged(h, G, 0, nframes, width, height, h->d_kps, h->d_desc, h->d_counts, h->d_status, s);
    if (rc == ORBX_OK) rc = download_outputs(h, nframes, s);
    if (rc != ORBX_OK) return rc;
    HIPCHK(hipStreamSynchronize(s));
    rc = finish_profile(h);
    if (rc != ORBX_OK) return rc;
    return deliver_batch(h, 0, nframes, keypoints, descriptors, cap, counts, h->h_counts, h->h_status, h->h_kps, h->h_desc);
}

// Chunk c's outputs live in a block of their own, [counts nf | status nf | (pad to 256) | keypoints nf x cap | descriptors nf x cap x 32]
// at chunk_off[c] of d_out / h_out, so that they come back with ONE copy (a device-to-host copy on a compute stream is ~8 us of
// stream time whatever its size; a chunk had four).
struct ChunkBlock { int32_t *counts, *status; orbx_keypoint *kps; uint8_t *desc; size_t bytes; };
static ChunkBlock chunk_block(const orbx_extractor *h, uint8_t *base, int c, int nf)
{
    const int ocap = h->max_plan.out_cap;
    uint8_t *b = base + h->chunk_off[c];
    const size_t hdr = align_up((size_t)2 * nf * sizeof(int32_t), 256);
    ChunkBlock B;
    B.counts = reinterpret_cast<int32_t *>(b); B.status = B.counts + nf;
    B.kps = reinterpret_cast<orbx_keypoint *>(b + hdr);
    B.desc = b + hdr + (size_t)nf * ocap * sizeof(orbx_keypoint);
    B.bytes = hdr + (size_t)nf * ocap * (sizeof(orbx_keypoint) + 32);
    return B;
}

// kernels + download of frames [k0, k1) = chunk c of the handle's own input block, on stream s
static int enqueue_chunk(orbx_extractor *h, int c, int k0, int k1, int width, int height, hipStream_t s)
{
    const int nf = k1 - k0;
    const ChunkBlock D = chunk_block(h, h->d_out, c, nf);
    int rc = enqueue_staged(h, stage_geom(h, width, height), k0, nf, width, height, D.kps, D.desc, D.counts, D.status, s);
    if (rc != ORBX_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->h_out + h->chunk_off[c], h->d_out + h->chunk_off[c], D.bytes, hipMemcpyDeviceToHost, s));
    return ORBX_OK;
}

extern "C" int orbx_extract_batch(orbx_extractor *h, const uint8_t *images, int nframes, int width, int height,
                                  int row_stride, size_t frame_stride, orbx_keypoint *keypoints,
                                  uint8_t *descriptors, int cap, int *counts)
{
    if (!h) return xfail(ORBX_E_INVALID, "NULL handle");
    if (!counts) return xfail(ORBX_E_INVALID, "counts is NULL");
    for (int k = 0; k < std::max(nframes, 0); k++) counts[k] = 0;
    if (h->inflight) return xfail(ORBX_E_INVALID, "an orbx_extract_begin call is in flight on this handle");
    if (!images || width <= 0 || height <= 0 || nframes <= 0) return ORBX_OK;   // :1048 empty image: silent return
    if (!keypoints || !descriptors) return xfail(ORBX_E_INVALID, "NULL output buffer");
    if (nframes > h->max_batch) return xfail(ORBX_E_INVALID, "nframes=%d (max_batch=%d)", nframes, h->max_batch);
    const int cn = orbx_format_channels(h->fmt);
    if (row_stride / cn < width) return xfail(ORBX_E_INVALID, "row_stride %d < width %d x %d channel%s", row_stride, width, cn, cn > 1 ? "s" : "");
    if (width > h->max_w || height > h->max_h) return xfail(ORBX_E_SHAPE, "frame %dx%d exceeds the handle's max %dx%d", width, height, h->max_w, h->max_h);
    HIPCHK(hipSetDevice(h->device));
    if (cn > 1) { int rcc = check_color_limits(width, height, color_pitch(width, cn)); if (rcc == ORBX_OK) rcc = orbx_ensure_color(h); if (rcc != ORBX_OK) return rcc; }
    if (!h->pool && nframes >= 8) {                         // staging threads: up to 6, leaving cores to the caller
        const unsigned hc = (unsigned)StagePool::usable_cpus();       // affinity mask and cgroup quota, not the machine's core count
        h->pool.reset(new StagePool((int)std::min<unsigned>(6u, hc > 2 ? hc / 2 - 1 : 0u)));
    }
    // Chunked pipeline ("host-buffer batches"): while chunk c is uploaded and extracted, chunk c + 1 is repacked by the
    // staging threads; chunks alternate between two streams, so the upload of one runs under the kernels of the other, and each
    // chunk's ten kernels + four downloads are ONE graph launch (a launch is ~5 us of host time, a chunk would be ~70).  Every
    // chunk works in its own slice of the workspace.  The first call of a shape, profiling runs and small batches take the
    // plain path.
    const int chunk = h->batch_chunk;
    const bool chunked = chunk > 0 && nframes >= 2 * chunk && h->profiling == 0 && !h->need_clear && width == h->cur_w && height == h->cur_h;
    if (!chunked) return extract_batch_simple(h, images, nframes, width, height, row_stride, frame_stride, keypoints, descriptors, cap, counts);

    // chunk boundaries: a half-size first chunk (the pipeline starts sooner) and a half-size last one (the tail that nothing hides
    // is shorter) around full-size ones
    std::vector<int> cut(1, 0);
    if (nframes >= 3 * chunk && chunk >= 2 && !batch_equal_chunks()) {
        cut.push_back(chunk / 2);
        while (nframes - cut.back() > chunk + chunk / 2) cut.push_back(cut.back() + chunk);
        if (nframes - cut.back() > chunk / 2) cut.push_back(nframes - chunk / 2);
    } else {
        while (nframes - cut.back() > chunk) cut.push_back(cut.back() + chunk);
    }
    cut.push_back(nframes);
    const int nch = (int)cut.size() - 1;
    {   // every chunk's output block (the graphs below are captured with these addresses; they depend on (nframes, chunk) only)
        h->chunk_off.assign(nch, 0);
        size_t off = 0;
        for (int c = 0; c < nch; c++) {
            const int nf = cut[c + 1] - cut[c];
            h->chunk_off[c] = off;
            off += align_up((size_t)2 * nf * sizeof(int32_t), 256) + (size_t)nf * h->max_plan.out_cap * (sizeof(orbx_keypoint) + 32);
        }
        if (off > h->d_out.bytes()) return xfail(ORBX_E_INVALID, "internal: chunk output blocks exceed the staging block");
    }
    hipStream_t st[3] = {h->stream, h->aux[0], h->aux[2]};
    const int nst = batch_streams();
    const bool have_graphs = !h->bg_off && h->bg_w == width && h->bg_h == height && h->bg_n == nframes && h->bg_chunk == chunk && (int)h->bgraph.size() == nch;
    if (!have_graphs && !h->bg_off) {                       // (re)build the per-chunk graphs for this shape
        drop_graphs(h);
        h->bgraph.resize(nch);
        bool ok = true;
        std::lock_guard<std::recursive_mutex> lk_(orbx_capture_mutex());   // once around all chunk captures (capture_graph() takes it again: recursive)
        for (int c = 0; c < nch && ok; c++) {
            hipStream_t s = st[c % nst];
            h->bgraph[c] = capture_graph(s, [&] { return enqueue_chunk(h, c, cut[c], cut[c + 1], width, height, s) == ORBX_OK; });
            ok = h->bgraph[c] != nullptr;
        }
        if (ok) { h->bg_w = width; h->bg_h = height; h->bg_n = nframes; h->bg_chunk = chunk; }
        else { drop_graphs(h); h->bg_off = true; }
    }
    const bool graphs = !h->bg_off && (int)h->bgraph.size() == nch;
    const bool trace = batch_trace();
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    // uploads go back to back on a stream of their own (on a chunk's compute stream the upload of chunk c + 2 would wait for
    // chunk c's kernels and downloads); each chunk's kernels wait for its own upload only
    hipStream_t up = h->aux[1];
    XTRY(orbx_ensure_chunk_events(h, nch));
    const bool pinned_ok = batch_pinned_ok();
    // the answer for one buffer is remembered (a capture pipeline hands over the same page-locked block again and again; should it
    // have been unregistered meanwhile, the copies below are still correct -- the runtime stages them -- only slower)
    const size_t frame_bytes = (size_t)(height - 1) * row_stride + (size_t)width * cn;
    const StageGeom G = stage_geom(h, width, height);
    if (pinned_ok && !(h->pin_ptr == images && h->pin_n == nframes && h->pin_stride == frame_stride && h->pin_bytes == frame_bytes)) {
        h->pin_ptr = images; h->pin_n = nframes; h->pin_stride = frame_stride; h->pin_bytes = frame_bytes;
        h->pin_is = is_pinned_host(images, nframes, frame_stride, frame_bytes);
    }
    const bool pinned_in = pinned_ok && h->pin_is;
    double t_stage = 0, t_launch = 0;
    const double t_begin = trace ? now() : 0;
    for (int c = 0; c < nch; c++) {
        const int k0 = cut[c], k1 = cut[c + 1];
        hipStream_t s = st[c % nst];
        const double ta = trace ? now() : 0;
        if (!pinned_in) stage_frames(h, G, images, k0, k1, height, row_stride, frame_stride);
        const double tb = trace ? now() : 0;
        if (pinned_in) { int rcu = upload_pinned(G.d_base, G.stride, G.frame, images, k0, k1, G.row_bytes, height, row_stride, frame_stride, up); if (rcu != ORBX_OK) return rcu; }
        else
            HIPCHK(hipMemcpyAsync(G.d_base + (size_t)k0 * G.frame, G.h_base + (size_t)k0 * G.frame,
                                  (size_t)(k1 - k0 - 1) * G.frame + G.stride * height, hipMemcpyHostToDevice, up));
        HIPCHK(hipEventRecord(h->chunk_ev[c].up, up));
        HIPCHK(hipStreamWaitEvent(s, h->chunk_ev[c].up, 0));
        if (graphs) HIPCHK(hipGraphLaunch(h->bgraph[c], s));
        else { int rc = enqueue_chunk(h, c, k0, k1, width, height, s); if (rc != ORBX_OK) return rc; }
        HIPCHK(hipEventRecord(h->chunk_ev[c].done, s));
        if (trace) { t_stage += tb - ta; t_launch += now() - tb; }
    }
    const double t_issued = trace ? now() : 0;
    // hand the chunks over as they finish: the copy-out of chunk c runs under the kernels of the chunks behind it
    double t_wait = 0;
    int rcd = ORBX_OK;
    for (int c = 0; c < nch; c++) {
        const int k0 = cut[c], k1 = cut[c + 1];
        const double tw = trace ? now() : 0;
        HIPCHK(hipEventSynchronize(h->chunk_ev[c].done));
        if (trace) t_wait += now() - tw;
        if (rcd == ORBX_OK) {
            const ChunkBlock Hb = chunk_block(h, h->h_out, c, k1 - k0);
            rcd = deliver_batch(h, k0, k1, keypoints, descriptors, cap, counts, Hb.counts, Hb.status, Hb.kps, Hb.desc);
        }
    }
    HIPCHK(hipStreamSynchronize(up));
    h->last_input = h->d_input; h->last_in_stride = h->in_stride; h->last_in_frame = (long long)h->in_frame; h->last_batch = nframes;
    if (trace)
        fprintf(stderr, "orbx_extract_batch %d frames, %d chunks%s%s: stage %.3f ms, launch %.3f, wait %.3f, deliver %.3f, total %.3f\n", nframes, nch,
                graphs ? " (graphs)" : "", pinned_in ? " (page-locked input)" : "", t_stage, t_launch, t_wait, now() - t_issued - t_wait, now() - t_begin);
    return rcd;
}

// one staged frame: upload, then the pipeline
static int upload_and_enqueue_one(orbx_extractor *h, int w, int hgt, hipStream_t s)
{
    const StageGeom G = stage_geom(h, w, hgt);
    HIPCHK(hipMemcpyAsync(G.d_base, G.h_base, G.stride * hgt, hipMemcpyHostToDevice, s));
    return enqueue_staged(h, G, 0, 1, w, hgt, h->d_kps, h->d_desc, h->d_counts, h->d_status, s);
}

extern "C" int orbx_extract_begin(orbx_extractor *h, const uint8_t *image, int width, int height, int stride)
{
    if (!h) return xfail(ORBX_E_INVALID, "NULL handle");
    if (h->inflight) return xfail(ORBX_E_INVALID, "orbx_extract_begin: a call is already in flight on this handle");
    h->inflight_frames = 0;
    if (!image || width <= 0 || height <= 0) { h->inflight = 1; return ORBX_OK; }     // :1048 empty image
    const int cn = orbx_format_channels(h->fmt);
    if (stride / cn < width) return xfail(ORBX_E_INVALID, "row_stride %d < width %d x %d channel%s", stride, width, cn, cn > 1 ? "s" : "");
    if (width > h->max_w || height > h->max_h) return xfail(ORBX_E_SHAPE, "frame %dx%d exceeds the handle's max %dx%d", width, height, h->max_w, h->max_h);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (cn > 1) {
        int rcc = check_color_limits(width, height, color_pitch(width, cn));
        if (rcc == ORBX_OK) rcc = orbx_ensure_color(h);
        if (rcc != ORBX_OK) return rcc;
        const StageGeom G = stage_geom(h, width, height);
        for (int y = 0; y < height; y++) memcpy(G.h_base + (size_t)y * G.stride, image + (size_t)y * stride, G.row_bytes);
    } else if (stride == h->in_stride) memcpy(h->h_in, image, (size_t)stride * height);
    else for (int y = 0; y < height; y++) memcpy(h->h_in + (size_t)y * h->in_stride, image + (size_t)y * stride, (size_t)width);
    // Same shape as the last call, nothing to clear, no profiling: the upload, the kernels and the download are one HIP graph
    // (captured on the second call of a shape, replayed from then on); every pointer in it belongs to the handle.
    const bool graphable = !h->graph_off && h->profiling == 0 && h->max_batch == 1 && !h->need_clear && width == h->cur_w && height == h->cur_h;
    auto have_graph = [&] { return graphable && h->graph_exec && h->graph_w == width && h->graph_h == height && h->graph_fmt == h->fmt; };
    if (!have_graph()) {
        const bool second = graphable && h->graph_seen_w == width && h->graph_seen_h == height;
        h->graph_seen_w = width; h->graph_seen_h = height;
        if (second) {
            h->graph_exec = capture_graph(s, [&] { return upload_and_enqueue_one(h, width, height, s) == ORBX_OK && download_outputs(h, 1, s) == ORBX_OK; });
            // a capture that failed or was invalidated (another thread's synchronous call) is not an error of this call; the capture
            // is tried again on a later call, three times at most
            if (h->graph_exec) { h->graph_w = width; h->graph_h = height; h->graph_fmt = h->fmt; }
            else if (++h->graph_fails >= 3) h->graph_off = true;
            else h->graph_seen_w = h->graph_seen_h = 0;
        }
    }
    // nothing ran during a capture: run this call now, through the graph or (without one) plainly
    if (have_graph()) HIPCHK(hipGraphLaunch(h->graph_exec, s));
    else {
        int rc = upload_and_enqueue_one(h, width, height, s);
        if (rc == ORBX_OK) rc = download_outputs(h, 1, s);
        if (rc != ORBX_OK) return rc;
    }
    h->inflight = 1; h->inflight_frames = 1;
    return ORBX_OK;
}

extern "C" int orbx_extract_end(orbx_extractor *h, orbx_keypoint *keypoints, uint8_t *descriptors, int cap, int *n)
{
    if (!h || !n) return xfail(ORBX_E_INVALID, "NULL argument");
    *n = 0;
    if (!h->inflight) return xfail(ORBX_E_INVALID, "orbx_extract_end without orbx_extract_begin");
    h->inflight = 0;
    if (h->inflight_frames == 0) return ORBX_OK;
    if (!keypoints || !descriptors) return xfail(ORBX_E_INVALID, "NULL output buffer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    int rc = finish_profile(h);
    if (rc != ORBX_OK) return rc;
    if (h->h_status[0] != ORBX_OK) return xfail(h->h_status[0], "device status %d (%s)", h->h_status[0], device_status_text(h->h_status[0]));
    const int cnt = h->h_counts[0];
    if (cnt > cap) return xfail(ORBX_E_CAPACITY, "%d keypoints, caller capacity %d (use orbx_capacity())", cnt, cap);
    memcpy(keypoints, h->h_kps, sizeof(orbx_keypoint) * cnt);
    memcpy(descriptors, h->h_desc, (size_t)32 * cnt);
    *n = cnt;
    return ORBX_OK;
}

extern "C" int orbx_extract(orbx_extractor *h, const uint8_t *image, int width, int height, int stride,
                            orbx_keypoint *keypoints, uint8_t *descriptors, int cap, int *n)
{
    if (!n) return xfail(ORBX_E_INVALID, "n is NULL");
    if (h && h->max_batch == 1 && h->profiling == 0 && !h->inflight) {      // the two halves back to back: one HIP graph per shape
        *n = 0;
        int rc = orbx_extract_begin(h, image, width, height, stride);
        if (rc != ORBX_OK) return rc;
        if (!keypoints || !descriptors) { h->inflight = 0; if (h->inflight_frames) (void)hipStreamSynchronize(h->stream); return xfail(ORBX_E_INVALID, "NULL output buffer"); }
        return orbx_extract_end(h, keypoints, descriptors, cap, n);
    }
    return orbx_extract_batch(h, image, 1, width, height, stride, (size_t)stride * (size_t)std::max(height, 0),
                              keypoints, descriptors, cap, n);
}

extern "C" int orbx_level_size(const orbx_extractor *h, int level, int *width, int *height)
{
    if (!h || level < 0 || level >= h->nlevels || h->cur_w == 0) return xfail(ORBX_E_INVALID, "no plan / bad level");
    if (width) *width = h->plan.lv[level].w;
    if (height) *height = h->plan.lv[level].h;
    return ORBX_OK;
}

// ---- the batched-frames mode sharded over several handles (BASELINE north_star: "a batched-frames mode shards
// independent frames across the GPUs of one node") behind the C ABI: ONE process, one host thread and one set of streams per
// handle.  Handle i (normally one per device; several on one device also work) takes the i-th contiguous block of the batch --
// the split of my-slam_amd/shard.py's shard_range, sizes differ by at most one -- and runs orbx_extract_batch on it; every block's
// outputs land in the caller's flat arrays at its frames' positions, so the result is the one-handle result whatever the split.
// No collective: the frames are independent and the outputs are host arrays.  (RCCL carries only the device-resident gather of
// bench.py's N-rank mode, where results stay in HBM.) ----
extern "C" int orbx_extract_batch_multi(orbx_extractor *const *handles, int nhandles, const uint8_t *images, int nframes, int width,
                                        int height, int row_stride, size_t frame_stride, orbx_keypoint *keypoints,
                                        uint8_t *descriptors, int cap, int *counts)
{
    if (!handles || nhandles < 1) return xfail(ORBX_E_INVALID, "no handles");
    for (int i = 0; i < nhandles; i++) {
        if (!handles[i]) return xfail(ORBX_E_INVALID, "handle %d is NULL", i);
        for (int j = 0; j < i; j++)
            if (handles[j] == handles[i]) return xfail(ORBX_E_INVALID, "handle %d is handle %d again: a handle is not re-entrant", i, j);
    }
    for (int i = 1; i < nhandles; i++)
        if (handles[i]->fmt != handles[0]->fmt) return xfail(ORBX_E_INVALID, "handle %d has input format %d, handle 0 has %d: one batch has one format", i, handles[i]->fmt, handles[0]->fmt);
    if (!counts) return xfail(ORBX_E_INVALID, "counts is NULL");
    for (int k = 0; k < std::max(nframes, 0); k++) counts[k] = 0;
    if (!images || width <= 0 || height <= 0 || nframes <= 0) return ORBX_OK;
    if (!keypoints || !descriptors) return xfail(ORBX_E_INVALID, "NULL output buffer");
    const int nh = std::min(nhandles, nframes);
    std::vector<int> lo(nh + 1);
    for (int i = 0; i <= nh; i++) lo[i] = i * (nframes / nh) + std::min(i, nframes % nh);
    std::vector<int> rc(nh, ORBX_OK);
    std::vector<std::string> msg(nh);
    auto run = [&](int i) {
        const int a = lo[i], n = lo[i + 1] - a;
        rc[i] = orbx_extract_batch(handles[i], images + (size_t)a * frame_stride, n, width, height, row_stride, frame_stride,
                                   keypoints + (size_t)a * cap, descriptors + (size_t)a * cap * 32, cap, counts + a);
        if (rc[i] != ORBX_OK) msg[i] = orbx_last_error();          // the error text is thread-local: carry it over
    };
    std::vector<std::thread> th;
    for (int i = 1; i < nh; i++) th.emplace_back(run, i);
    run(0);
    for (auto &t : th) t.join();
    for (int i = 0; i < nh; i++)
        if (rc[i] != ORBX_OK) return xfail(rc[i], "block %d (frames %d..%d, device %d): %s", i, lo[i], lo[i + 1] - 1, handles[i]->device, msg[i].c_str());
    return ORBX_OK;
}

static inline int reflect101_host(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

// Levels [l0, l1) of frame `frame` of the last call into dst[l - l0]: one asynchronous copy per level into a page-locked staging block,
// ONE synchronisation, then the rows are laid out in the caller's buffers and the reflect-101 border is rebuilt on the host
// (src/ORBextractor.cc:1115-1133).  This is what keeps ORBextractor::mvImagePyramid valid after every operator() in the adapter.
static int download_levels(orbx_extractor *h, int frame, int l0, int l1, uint8_t *const *dst, const int *dst_stride, int border)
{
    if (!dst || !dst_stride || l0 < 0 || l1 > h->nlevels || h->cur_w == 0 || frame < 0 || frame >= h->last_batch || border < 0)
        return xfail(ORBX_E_INVALID, "bad pyramid download argument");
    HIPCHK(hipSetDevice(h->device));
    size_t need = 0, off[ORBX_MAX_LEVELS];
    for (int l = l0; l < l1; l++) {
        const OrbxLevel &L = h->plan.lv[l];
        if (!dst[l - l0] || dst_stride[l - l0] < L.w + 2 * border) return xfail(ORBX_E_INVALID, "level %d: NULL buffer or dst_stride too small", l);
        off[l] = need;
        need += ((size_t)L.w * L.h + 255) & ~(size_t)255;
    }
    XTRY(orbx_ensure_pyr_staging(h, need));
    HIPCHK(hipDeviceSynchronize());   // the last call may have run on a caller stream and the aux streams
    for (int l = l0; l < l1; l++) {
        OrbxLevel L = h->plan.lv[l];
        if (l == 0) { L.base = const_cast<uint8_t *>(h->last_input); L.stride = h->last_in_stride; L.frame_stride = h->last_in_frame; }
        HIPCHK(hipMemcpy2DAsync(h->h_pyr + off[l], (size_t)L.w, L.base + (size_t)frame * L.frame_stride, L.stride, L.w, L.h, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int l = l0; l < l1; l++) {
        const OrbxLevel &L = h->plan.lv[l];
        const int ds = dst_stride[l - l0];
        uint8_t *interior = dst[l - l0] + (size_t)border * ds + border;
        for (int y = 0; y < L.h; y++) memcpy(interior + (size_t)y * ds, h->h_pyr + off[l] + (size_t)y * L.w, (size_t)L.w);
        if (border > 0) {             // copyMakeBorder(..., BORDER_REFLECT_101), :1127-1133
            for (int y = 0; y < L.h; y++) {
                uint8_t *row = interior + (size_t)y * ds;
                for (int x = 1; x <= border; x++) { row[-x] = row[reflect101_host(-x, L.w)]; row[L.w - 1 + x] = row[reflect101_host(L.w - 1 + x, L.w)]; }
            }
            for (int y = 1; y <= border; y++) {
                memcpy(interior - (ptrdiff_t)y * ds - border, interior + (ptrdiff_t)reflect101_host(-y, L.h) * ds - border, (size_t)L.w + 2 * border);
                memcpy(interior + (ptrdiff_t)(L.h - 1 + y) * ds - border, interior + (ptrdiff_t)reflect101_host(L.h - 1 + y, L.h) * ds - border, (size_t)L.w + 2 * border);
            }
        }
    }
    return ORBX_OK;
}
extern "C" int orbx_download_level(orbx_extractor *h, int frame, int level, uint8_t *dst, int dst_stride, int border)
{
    if (!h || level < 0 || level >= h->nlevels) return xfail(ORBX_E_INVALID, "bad download_level argument");
    return download_levels(h, frame, level, level + 1, &dst, &dst_stride, border);
}
extern "C" int orbx_download_pyramid(orbx_extractor *h, int frame, uint8_t *const *dst, const int *dst_stride, int border)
{
    if (!h) return xfail(ORBX_E_INVALID, "bad download_pyramid argument");
    return download_levels(h, frame, 0, h->nlevels, dst, dst_stride, border);
}

extern "C" int orbx_download_candidates(orbx_extractor *h, int frame, int level, int32_t *xyr, int cap)
{
    if (!h || !xyr || level < 0 || level >= h->nlevels || h->cur_w == 0 || frame < 0 || frame >= h->last_batch)
        return xfail(ORBX_E_INVALID, "bad download_candidates argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, h->work.ncand + (size_t)frame * h->nlevels + level, sizeof(n), hipMemcpyDeviceToHost));
    const OrbxLevel &L = h->plan.lv[level];
    n = std::min<uint32_t>(n, (uint32_t)L.cand_cap);
    if ((int)n > cap) return xfail(ORBX_E_CAPACITY, "%u candidates, capacity %d", n, cap);
    std::vector<OrbxCand> tmp(n ? n : 1);
    HIPCHK(hipMemcpy(tmp.data(), h->work.cand + (size_t)frame * h->plan.cand_frame + L.cand_off, sizeof(OrbxCand) * n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        xyr[3 * i] = (int32_t)(tmp[i].xy & 0xFFFFu);
        xyr[3 * i + 1] = (int32_t)(tmp[i].xy >> 16);
        xyr[3 * i + 2] = (int32_t)tmp[i].resp;
    }
    return (int)n;
}

// pyramid description of the last call (frame 0) for the stereo matcher (orbx_stereo.hip)
int orbx_internal_levels(orbx_extractor *h, const uint8_t **base, int *w, int *hh, int *stride, float *scale, float *inv_scale, int *nlevels, int *device)
{
    if (!h || h->cur_w == 0 || h->last_batch < 1) return ORBX_E_INVALID;
    *nlevels = h->nlevels; *device = h->device;
    for (int l = 0; l < h->nlevels; l++) {
        const OrbxLevel &L = h->plan.lv[l];
        base[l] = l == 0 ? h->last_input : L.base;
        stride[l] = l == 0 ? h->last_in_stride : L.stride;
        w[l] = L.w; hh[l] = L.h;
        scale[l] = h->scale[l]; inv_scale[l] = h->inv_scale[l];
    }
    return ORBX_OK;
}
