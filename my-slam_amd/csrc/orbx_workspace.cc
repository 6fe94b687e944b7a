// orbx_workspace.cc -- host-only: the extractor handle's life and its lazy resources (orbx_handle.h, dev_buf.h).  No kernel is
// launched from here, so a host compiler builds this file and a test can run it against its own HIP allocator.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "orbx_handle.h"

static thread_local std::string g_err;
int xfail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
extern "C" const char *orbx_last_error(void) { return g_err.c_str(); }

// Stream captures against the rest of the process.  A capture is begun in RELAXED mode (this library issues nothing unsafe inside one,
// and other threads' calls must not be judged against it), and the phases in which a handle uses synchronous runtime calls -- creation,
// destruction, the table upload of a shape change -- exclude every capture of this library through one process-wide lock: on this runtime
// a synchronous copy in one thread has been seen to fail, and to invalidate the capture of ANOTHER thread's handle, even in thread-local
// mode (tests/test_threads_gpu.py, once in a dozen runs).  A capture that is invalidated all the same is not an error: the call runs
// plainly and the capture is tried again on a later call (three times at most).
std::recursive_mutex &orbx_capture_mutex()
{
    static std::recursive_mutex m;
    return m;
}

// the switches read at every create (tests and A/B runs set them between two handles of one process)
static void read_create_switches(orbx_extractor *h)
{
    if (const char *e = getenv("ORBX_OCT_FAST")) h->oct_fast = atoi(e);
    // ORBX_PYRAMID_TILES = "a[,tile width[,tile height[,min frames]]]": levels a + 1 .. last in one launch (0 = off = default).
    // Bit-exact, and at 64 x 640x480 slower than the per-level launches (levels 3..7: 40 us against 27; without any store 30): the
    // tiles' halos make it compute 1.8x the pixels, two waves per SIMD are all the 1920 tiles give.  Kept as an A/B switch.
    if (const char *e = getenv("ORBX_PYRAMID_TILES")) { int a = 2, tw = 32, th = 32, mf = 8; const int n = sscanf(e, "%d,%d,%d,%d", &a, &tw, &th, &mf); if (n >= 1) h->tile_a = a; if (n >= 2) h->tile_w = tw; if (n >= 3) h->tile_h = th; if (n >= 4) h->tile_min_frames = mf; }
    if (h->tile_w < 8 || h->tile_w > 128 || (h->tile_w & 3) || h->tile_h < 8 || h->tile_h > 128 || (h->tile_h & 3)) h->tile_a = 0;
    if (const char *e = getenv("ORBX_PYRAMID_FUSE")) h->fuse_on = atoi(e);
    if (const char *e = getenv("ORBX_OVERLAP_PYRAMID")) h->overlap_pyr = atoi(e) != 0;   // A/B switch for ORBX_OPT_OVERLAP_PYRAMID
}

// one allocation per block, of 256 bytes at least
template <class B> static int alloc(B &b, size_t bytes, const char *what) { return b.grow(std::max<size_t>(bytes, 256), xfail, what); }

extern "C" int orbx_create(orbx_extractor **out, int nfeatures, float scale_factor, int nlevels,
                           int ini_th, int min_th, int device, int max_width, int max_height, int max_batch)
{
    std::lock_guard<std::recursive_mutex> lk_(orbx_capture_mutex());
    if (!out) return xfail(ORBX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (nfeatures < 0 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scale_factor > 1.0f) ||
        max_width < 1 || max_height < 1 || max_batch < 1)
        return xfail(ORBX_E_INVALID, "bad constructor argument (nfeatures=%d scale=%g nlevels=%d max=%dx%dx%d)",
                     nfeatures, scale_factor, nlevels, max_width, max_height, max_batch);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return xfail(ORBX_E_HIP, "no HIP device: liborbx has no CPU path");
    if (device < 0 || device >= ndev) return xfail(ORBX_E_INVALID, "device %d of %d", device, ndev);
    HIPCHK(hipSetDevice(device));

    std::unique_ptr<orbx_extractor> owner(new orbx_extractor());   // every failure exit below frees what was built so far
    orbx_extractor *h = owner.get();
    h->nfeatures = nfeatures; h->scale_factor = scale_factor; h->nlevels = nlevels;
    h->ini_th = std::min(std::max(ini_th, 0), 255); h->min_th = std::min(std::max(min_th, 0), 255);
    h->device = device; h->max_w = max_width; h->max_h = max_height; h->max_batch = max_batch;
    read_create_switches(h);
    orbx_build_tables(h);

    std::string why;
    int rc = orbx_make_plan(*h, max_width, max_height, &h->max_plan, &why);
    if (rc != ORBX_OK) return xfail(rc, "max shape %dx%d: %s", max_width, max_height, why.c_str());
    int max_list = 0;
    for (int l = 0; l < nlevels; l++) max_list = std::max(max_list, h->max_plan.lv[l].list_cap);
    h->oct_cap_max = std::max(max_list, 8);
    h->oct_lds = orbx_octree_lds_bytes(h->oct_cap_max, 0, 0);
    if (h->oct_lds > 150 * 1024) return xfail(ORBX_E_INVALID, "nfeatures=%d needs %zu B of LDS for the quadtree (max 153600)", nfeatures, h->oct_lds);

    const size_t B = (size_t)max_batch;
    h->in_stride = (int)align_up(max_width, 64);
    h->in_frame = align_up((size_t)h->in_stride * max_height, 256);
    XTRY(alloc(h->d_input, B * h->in_frame + 256, "input block"));
    size_t off = 0, tab_e = 0;
    for (int l = 1; l < nlevels; l++) {
        const OrbxLevel &L = h->max_plan.lv[l];
        h->pyr_level_off[l] = off;
        off += B * align_up(align_up(L.w, 64) * (size_t)L.h, 256);
        tab_e += align_up((size_t)L.w + 4, 4) + align_up((size_t)L.h + 4, 4);
    }
    h->tab_elems = tab_e;
    XTRY(alloc(h->d_pyr, off + 256, "pyramid"));   // slack: the 4x4 resize reads whole dwords around a row segment
    XTRY(alloc(h->d_tab_i, tab_e * sizeof(int), "resize offsets"));
    XTRY(alloc(h->d_tab_s, tab_e * sizeof(short2), "resize weights"));
    h->bands_cap = 2 * ((size_t)max_height / 8 + 4) * ORBX_MAX_LEVELS;
    XTRY(alloc(h->d_bands, h->bands_cap * sizeof(int4), "band table"));
    h->tiles_cap = 8192;
    XTRY(alloc(h->d_tiles, h->tiles_cap * sizeof(int4), "tile table"));
    h->cells_cap = h->max_plan.ncells + 64 * nlevels;   // a smaller frame never has more cells; slack for rounding
    XTRY(alloc(h->d_cells, (size_t)h->cells_cap * sizeof(uint32_t), "cell table"));
    const OrbxPlan &M = h->max_plan;
    XTRY(alloc(h->w_cand, B * M.cand_frame * sizeof(OrbxCand), "FAST candidates"));
    XTRY(alloc(h->w_owner, B * M.cand_frame * sizeof(uint32_t), "quadtree owners"));
    XTRY(alloc(h->w_arena, B * M.arena_frame * sizeof(OrbxNode), "quadtree arena"));
    XTRY(alloc(h->w_sel, B * M.list_frame * sizeof(OrbxCand), "selected keypoints"));
    XTRY(alloc(h->w_cand_count, B * ORBX_MAX_LEVELS * ORBX_CNT_STRIDE * sizeof(uint32_t), "candidate counters"));
    XTRY(alloc(h->w_nk, B * ORBX_MAX_LEVELS * sizeof(uint32_t), "keypoint counts"));
    XTRY(alloc(h->w_ncand, B * ORBX_MAX_LEVELS * sizeof(uint32_t), "candidate counts"));
    XTRY(alloc(h->w_errflags, B * sizeof(uint32_t), "error flags"));
    // the host-buffer entry points' staging outputs live in ONE block, [counts B | status B | keypoints B x cap | descriptors
    // B x cap x 32], mirrored in pinned memory: a full batch (or a max_batch = 1 handle) comes back with a single copy
    h->out_hdr = align_up(2 * B * sizeof(int32_t), 256);
    h->out_kps_bytes = B * M.out_cap * sizeof(orbx_keypoint);
    // + per-chunk blocks of orbx_extract_batch: one aligned header per chunk instead of one per batch
    XTRY(alloc(h->d_out, h->out_hdr + h->out_kps_bytes + B * M.out_cap * 32 + 256 * (B + 2), "output block"));
    XTRY(h->h_in.grow(B * h->in_frame + 256, xfail, "input staging (page-locked)"));
    XTRY(h->h_out.grow(h->d_out.bytes(), xfail, "output staging (page-locked)"));
    // the views: the one place that fills them
    OrbxWork &w = h->work;
    w.cand = h->w_cand; w.cand_count = h->w_cand_count; w.owner = h->w_owner; w.arena = h->w_arena;
    w.sel = h->w_sel; w.ncand = h->w_ncand; w.nk = h->w_nk; w.errflags = h->w_errflags;
    h->d_counts = reinterpret_cast<int32_t *>(h->d_out.get()); h->d_status = h->d_counts + B;
    h->d_kps = reinterpret_cast<orbx_keypoint *>(h->d_out + h->out_hdr); h->d_desc = h->d_out + h->out_hdr + h->out_kps_bytes;
    h->h_counts = reinterpret_cast<int32_t *>(h->h_out.get()); h->h_status = h->h_counts + B;
    h->h_kps = reinterpret_cast<orbx_keypoint *>(h->h_out + h->out_hdr); h->h_desc = h->h_out + h->out_hdr + h->out_kps_bytes;
    XTRY(h->stream.create(xfail, "stream"));
    for (auto &e : h->ev) XTRY(e.create(hipEventDefault, xfail, "stage event"));
    for (auto &a : h->aux) XTRY(a.create(xfail, "side stream"));
    for (auto &e : h->ev_join) XTRY(e.create(hipEventDisableTiming, xfail, "join event"));
    XTRY(h->ev_fork.create(hipEventDisableTiming, xfail, "fork event"));
    if (orbx_upload_constants(h->umax, h->gauss_k) != 0) return xfail(ORBX_E_HIP, "constant upload failed");
    if (orbx_selftest_fp16() != 0) return xfail(ORBX_E_HIP, "fp16 subnormal self-test failed: the FAST score tree needs fp16 subnormals enabled on this device");
    *out = owner.release();
    return ORBX_OK;
}

extern "C" void orbx_destroy(orbx_extractor *h)
{
    std::lock_guard<std::recursive_mutex> lk_(orbx_capture_mutex());
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int orbx_ensure_color(orbx_extractor *h)
{
    if (h->d_color && h->h_color) return ORBX_OK;
    std::lock_guard<std::recursive_mutex> lk_(orbx_capture_mutex());   // allocation is a synchronous runtime call
    const size_t bytes = (size_t)h->max_batch * color_frame(h->max_w, h->max_h, 4) + 256;
    int rc = h->d_color.grow(bytes, xfail, "colour input block");
    if (rc == ORBX_OK) rc = h->h_color.grow(bytes, xfail, "colour input staging (page-locked)");
    if (rc != ORBX_OK) { h->d_color.reset(); h->h_color.reset(); }
    return rc;
}

int orbx_ensure_pyr_staging(orbx_extractor *h, size_t need)
{
    if (need <= h->h_pyr.bytes()) return ORBX_OK;
    return h->h_pyr.grow(need + need / 4, xfail, "pyramid download staging (page-locked)");
}

int orbx_ensure_chunk_events(orbx_extractor *h, int nchunks)
{
    while ((int)h->chunk_ev.size() < nchunks) {      // a pair joins the handle only once both of its events exist
        OrbxChunkEvents p;
        XTRY(p.up.create(hipEventDisableTiming, xfail, "chunk upload event"));
        XTRY(p.done.create(hipEventDisableTiming, xfail, "chunk completion event"));
        h->chunk_ev.push_back(std::move(p));
    }
    return ORBX_OK;
}

extern "C" int orbx_set_profiling(orbx_extractor *h, int mode)
{
    if (!h || mode < 0 || mode > 2) return xfail(ORBX_E_INVALID, "profiling mode %d", mode);
    if (mode == 2 && h->ring.empty()) {              // the ring joins the handle complete, and the mode changes only after it has
        HIPCHK(hipSetDevice(h->device));
        std::vector<OrbxRingSlot> ring(ORBX_PROF_RING);
        for (auto &slot : ring) for (auto &e : slot.e) XTRY(e.create(hipEventDefault, xfail, "profiling ring event"));
        h->ring = std::move(ring);
    }
    h->profiling = mode; h->ring_calls = 0;
    return ORBX_OK;
}
