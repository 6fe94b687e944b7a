// orbm_workspace.cc -- host-only: the matcher handle's life and the growth of its device memory (orbm_internal.h, dev_buf.h).
// No kernel is launched from here, so a host compiler builds this file and a test can run it against its own HIP allocator.
#include <cstdlib>
#include "orbm_internal.h"

static thread_local std::string g_merr;
int mfail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_merr = buf;
    return code;
}
extern "C" const char *orbm_last_error(void) { return g_merr.c_str(); }

extern "C" void orbm_destroy(orbm_matcher *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

extern "C" int orbm_create(orbm_matcher **out, int device, int max_queries, int max_train, int max_pairs)
{
    if (!out) return mfail(ORBX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_queries < 1 || max_train < 1 || max_pairs < 0) return mfail(ORBX_E_INVALID, "bad sizes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return mfail(ORBX_E_HIP, "no HIP device: liborbx has no CPU path");
    if (device < 0 || device >= ndev) return mfail(ORBX_E_INVALID, "device %d of %d", device, ndev);
    MHIPCHK(hipSetDevice(device));
    orbm_matcher *m = new orbm_matcher();
    m->device = device;
    { const char *e = getenv("ORBM_DENSE"); m->dense_popcount = e && !strcmp(e, "popcount"); }
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
        orbm_reserve(m, max_queries, max_train, max_pairs) != ORBX_OK) {
        orbm_destroy(m);
        return mfail(ORBX_E_HIP, "matcher workspace allocation failed");
    }
    *out = m;
    return ORBX_OK;
}

static void grid_drop(orbm_matcher *m)
{
    m->grid_mem[0].reset(); m->grid_mem[1].reset();
    m->grid = {}; m->grid2 = {};
    m->grid_ok = false; m->grid2_ok = false;
}

// Grows the workspace (never shrinks it).  The reference's matcher has no size limit (it works on std::vectors), so every entry
// point that finds its inputs larger than the handle grows the handle instead of refusing; a caller that knows its sizes calls this
// once up front and no call allocates.  Growing max_train drops the Frame grid in the handle (orbm_grid_build again).
extern "C" int orbm_reserve(orbm_matcher *m, int max_queries, int max_train, int max_pairs)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (max_queries <= m->max_q() && max_train <= m->max_t() && max_pairs <= m->max_pairs()) return ORBX_OK;
    const size_t nq = (size_t)std::max(m->max_q(), max_queries), nt = (size_t)std::max(m->max_t(), max_train);
    const size_t np = (size_t)std::max(m->max_pairs(), max_pairs);
    MHIPCHK(hipSetDevice(m->device));
    MHIPCHK(hipStreamSynchronize(m->stream));
    if (nt * 32 > m->d_t.bytes()) grid_drop(m);                     // sized by max_train
    MTRY(m->d_q.grow(nq * 32, mfail, "query descriptors"));
    MTRY(m->d_off.grow((nq + 1) * 4, mfail, "candidate offsets"));
    MTRY(m->d_t.grow(nt * 32, mfail, "train descriptors"));
    MTRY(m->d_idx.grow(std::max<size_t>(np, 1) * 4, mfail, "candidate indices"));
    MTRY(m->d_out.grow(std::max(3 * nq, np) * 4, mfail, "result buffer"));
    return ORBX_OK;
}
int orbm_grow(orbm_matcher *m, long long need_q, long long need_t, long long need_pairs)
{
    if (need_q > (1ll << 28) || need_t > (1ll << 28) || need_pairs > (1ll << 30)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 descriptors / 2^30 pairs");
    auto up = [](long long need, int have) { return need > have ? (int)std::min<long long>(need + need / 2, 1ll << 30) : have; };
    return orbm_reserve(m, up(need_q, m->max_q()), up(need_t, m->max_t()), up(need_pairs, m->max_pairs()));
}

int orbm_grid_ensure(orbm_matcher *m, int slot)
{
    DevBuf<uint8_t> &mem = m->grid_mem[slot];
    if (mem) return ORBX_OK;
    const size_t arr = ((size_t)m->max_t() * 4 + 255) & ~(size_t)255;
    MTRY(mem.grow(5 * arr + (ORBM_GRID_CELLS + 1) * 4, mfail, "frame grid"));
    OrbmGrid &g = slot ? m->grid2 : m->grid;
    uint8_t *p = mem;
    g.kx = (float *)p; g.ky = (float *)(p + arr); g.koct = (int32_t *)(p + 2 * arr);
    g.items = (int32_t *)(p + 3 * arr); g.cell_of = (int32_t *)(p + 4 * arr); g.cell_start = (int32_t *)(p + 5 * arr);
    return ORBX_OK;
}

// ---- pinned staging arena (see orbm_internal.h) ----
int orbm_arena_begin(orbm_matcher *m)
{
    if (m->arena_want > m->arena_cap()) {        // grow between calls only: nothing is in flight here
        MHIPCHK(hipStreamSynchronize(m->stream));
        const size_t cap = m->arena_want + m->arena_want / 2 + (64u << 10);
        MTRY(m->arena.grow(cap, mfail, "pinned staging arena"));
        MTRY(m->d_arena.grow(cap, mfail, "staging arena's device mirror"));
    }
    m->arena_used = 0; m->arena_want = 0; m->npend = 0;
    return ORBX_OK;
}

// Growing means synchronise + free + allocate: not inside a stream capture (warm the handle up with the same arguments first).
static int refuse_growth_in_capture(hipStream_t s, const char *what, size_t have, size_t need, const char *unit)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive)
        return mfail(ORBX_E_INVALID, "the matcher's %s must grow (%zu -> %zu %s) while the stream is being captured: run the call once outside the capture",
                     what, have, need, unit);
    (void)hipGetLastError();
    return ORBX_OK;
}
int orbm_ensure_partials(orbm_matcher *m, size_t need, hipStream_t s)
{
    if (need <= m->d_part.count()) return ORBX_OK;
    MTRY(refuse_growth_in_capture(s, "partial buffer", m->d_part.count(), need, "pairs"));
    MHIPCHK(hipDeviceSynchronize());
    return m->d_part.grow(need * sizeof(uint2), mfail, "partial buffer");
}
int orbm_ensure_dd(orbm_matcher *m, size_t need, hipStream_t s)
{
    if (need <= m->d_dd.bytes()) return ORBX_OK;
    MTRY(refuse_growth_in_capture(s, "MapPoint scratch", m->d_dd.bytes(), need, "bytes"));
    MHIPCHK(hipStreamSynchronize(m->stream));
    if (s && s != m->stream) MHIPCHK(hipStreamSynchronize(s));
    return m->d_dd.grow(need + need / 2, mfail, "MapPoint scratch");
}
int orbm_ensure_fuse(orbm_matcher *m, size_t need)
{
    if (need <= m->d_fuse.bytes()) return ORBX_OK;
    MHIPCHK(hipStreamSynchronize(m->stream));
    return m->d_fuse.grow(need + need / 2, mfail, "Fuse batch workspace");
}
int orbm_ensure_opt(orbm_matcher *m, size_t need)
{
    MTRY(m->opt_pin.grow(64, mfail, "optimizer read-back block"));
    if (need <= m->d_opt.bytes()) return ORBX_OK;
    MHIPCHK(hipStreamSynchronize(m->stream));
    return m->d_opt.grow(need + need / 2, mfail, "optimizer workspace");
}
