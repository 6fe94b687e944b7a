// orbm_internal.h -- shared by orbm.hip, orbm_grid.hip, orbm_kf.hip, orbm_mappoint.hip, orbm_triangulate.hip, orbm_newpoints.hip,
// orbm_frustum.hip, orbm_pose.hip, orbm_bow.hip, orbm_sim3.hip, orbm_pnp.hip and orbm_init.hip.  The window walk of the grid searches (orbm_grid.hip, orbm_kf.hip) is in orbm_window.h,
// the frame of the hypothesis kernels and the argument checks of the batched solver calls in orbm_hyp.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/orbm.h"
#include "dev_buf.h"

#define M_THREADS 256

int mfail(int code, const char *fmt, ...);
#define MHIPCHK(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return mfail(ORBX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define MTRY(expr)                            \
    do {                                      \
        int mtry_ = (expr);                   \
        if (mtry_ != ORBX_OK) return mtry_;   \
    } while (0)

#ifdef __HIPCC__
__device__ __forceinline__ int hamming256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y);
    d += __popc(a0.z ^ b0.z);
    d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x);
    d += __popc(a1.y ^ b1.y);
    d += __popc(a1.z ^ b1.z);
    d += __popc(a1.w ^ b1.w);
    return d;
}
#endif

#define ORBM_GRID_COLS 64   // FRAME_GRID_COLS, include/Frame.h:38
#define ORBM_GRID_ROWS 48   // FRAME_GRID_ROWS, include/Frame.h:37
#define ORBM_GRID_CELLS (ORBM_GRID_COLS * ORBM_GRID_ROWS)

struct OrbmGrid {               // device-resident Frame grid of the train frame
    float min_x, min_y, inv_w, inv_h;   // PosInGrid's origin and cell sizes (Frame::mnMinX / mnMinY, mfGridElementWidthInv / HeightInv)
    float qmin_x, qmin_y;               // GetFeaturesInArea's origin: the same for a Frame; a KeyFrame subtracts its own int mnMinX / mnMinY
    int n;
    float *kx, *ky; int32_t *koct;      // SoA copy of the undistorted keypoints
    int32_t *cell_start;                // [ORBM_GRID_CELLS + 1]
    int32_t *items;                     // [n] keypoint indices, push_back order inside a cell
    int32_t *cell_of;                   // [n] scratch
};

#ifdef __HIPCC__
// wave-wide minimum, every lane gets it: butterfly inside each row of 16 lanes with DPP (quad swaps, half-row and row mirror),
// then the four row results through v_readlane.  ~10 instructions; six ds_bpermute steps are several hundred cycles.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false));     // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false));     // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false));    // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false));    // row_mirror
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(r0, r1), min(r2, r3));
}

// The wave's best key B and second-best S from every lane's own best key and second.  SHIFT = 0: `second` is a key like `best`;
// SHIFT > 0: `second` is a distance and a key is distance << SHIFT | position.  The winning lane offers its second, every other lane
// its best (a lane's second is never below its own best).  Precondition: the keys of the lanes that hold a candidate are unique (the
// positions are), and when no lane holds one, all lanes hold the same sentinel pair, which then comes back as (B, S).
template <int SHIFT>
__device__ __forceinline__ void wave_best2(uint32_t best, uint32_t second, uint32_t &B, uint32_t &S)
{
    B = wave_min_u32(best);
    S = wave_min_u32(best == B ? second : best >> SHIFT);
}

#endif

struct orbm_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> d_q, d_t;
    DevBuf<int32_t> d_off, d_idx, d_out;                             // d_out: max(3*max_q, max_pairs) ints
    DevBuf<uint2> d_part;                                            // train-split partials (lazy)
    int dense_popcount = 0;                                          // ORBM_DENSE=popcount: the VALU kernel instead of the matrix cores (A/B record)
    // N1: Frame grid of the last orbm_grid_build, and a second slot: orbm_search_by_sim3 searches two key frames.  A slot's six
    // arrays are one block of max_t keypoints (grid_mem[slot]): all of them or none.  grid_ok: the slot has been built
    OrbmGrid grid = {};  bool grid_ok = false;
    OrbmGrid grid2 = {}; bool grid2_ok = false;
    DevBuf<uint8_t> grid_mem[2];
    // pinned bump arena for the host-buffer entry points: pageable hipMemcpyAsync is a staged, synchronous copy of tens of
    // microseconds each; through pinned memory the copies of one call queue up behind each other and cost one round trip
    PinBuf<uint8_t> arena; size_t arena_used = 0, arena_want = 0;
    DevBuf<uint8_t> d_arena;        // device mirror of the arena: the inputs of a call (InBlock) go up in ONE copy
    struct Pend { void *dst; const void *src; size_t bytes; };
    Pend pend[8]; int npend = 0;
    DevBuf<uint8_t> d_dd;           // orbm_mappoint.hip: scratch of orbm_distinctive_descriptors (lazy, its own block)
    DevBuf<uint8_t> d_fuse;         // orbm_fuse.hip: the grids of all views and the dense results of orbm_fuse_views (lazy, its own block)
    DevBuf<uint8_t> d_opt;          // the workspace of LBA, BA (orbm_lba.hip), EG (orbm_eg.hip) and both SPD entry points (lazy)
    PinBuf<uint8_t> opt_pin;        // the 64 bytes the three optimizers read back after a trial (OptGpu, orbm_opt.h)
    // the capacities the handle advertises are what its buffers hold
    int max_q() const { return (int)std::min(std::min(d_q.bytes() / 32, (d_off.count() ? d_off.count() - 1 : 0)), d_out.count() / 3); }
    int max_t() const { return (int)(d_t.bytes() / 32); }
    int max_pairs() const { return (int)std::min(d_idx.count(), d_out.count()); }
    size_t arena_cap() const { return std::min(arena.bytes(), d_arena.bytes()); }
};
// orbm_workspace.cc (host-only): workspace growth.  The reference's matcher has no size limit, so entry points grow the handle
// instead of refusing.  A failed growth leaves the buffer empty and the capacity 0: the next call grows again.
int orbm_grow(orbm_matcher *m, long long need_q, long long need_t, long long need_pairs);
int orbm_grid_ensure(orbm_matcher *m, int slot);       // the slot's arrays, sized by max_t (dropped when max_t grows)
int orbm_ensure_partials(orbm_matcher *m, size_t need, hipStream_t s = nullptr);          // d_part of `need` pairs
int orbm_ensure_dd(orbm_matcher *m, size_t need, hipStream_t s);                            // d_dd of `need` bytes
int orbm_ensure_fuse(orbm_matcher *m, size_t need);                                         // d_fuse of `need` bytes
int orbm_ensure_opt(orbm_matcher *m, size_t need);                                          // d_opt of `need` bytes, opt_pin of 64
// orbm_spd.hip: A = L L^T in place in the lower triangle of the row-major n x n A, then L y = b and L^T x = y, all device memory;
// A, b and y are overwritten.  flag: != 0 where a pivot failed (x is then zeros); ok_out (may be NULL): 1.0 / 0.0.  Enqueues only.
int orbm_spd_solve_device(double *A, double *b, double *y, double *x, int *flag, double *ok_out, int n, hipStream_t s);
// orbm_grid.hip: k_grid_build_views, one workgroup per view: view v builds d_grids[v] from the keypoints d_kps + d_off[v]
void orbm_grid_build_views_launch(const OrbmGrid *d_grids, const int32_t *d_off, const orbx_keypoint *d_kps, int nviews, hipStream_t s);
// orbm_grid.hip: builds a grid slot (asynchronous on the handle's stream unless it had to allocate a staging block), and the
// windows + candidate distances pass the host-scanned matchers share (against grid slot g: NULL = m->grid); slot 0 = m->grid, 1 = m->grid2
int orbm_grid_build_into(orbm_matcher *m, int slot, const orbx_keypoint *kps_un, int n, float assign_min_x, float assign_min_y,
                         float inv_w, float inv_h, float query_min_x, float query_min_y);
int orbm_area_pairs(orbm_matcher *m, const float *x, const float *y, const float *r, const int32_t *mn, const int32_t *mx, int nq,
                    const uint8_t *qdesc, const uint8_t *train_desc, int n_train,
                    std::vector<int32_t> &off, std::vector<int32_t> &idx, std::vector<int32_t> &dist);
int orbm_arena_begin(orbm_matcher *m);                                                    // start of a host-API call
int orbm_h2d(orbm_matcher *m, void *dev, const void *host, size_t bytes, hipStream_t s);   // staged host -> device copy
int orbm_d2h(orbm_matcher *m, void *host, const void *dev, size_t bytes, hipStream_t s);   // staged; lands in host at orbm_sync()
// one device block -> several host arrays (the pending list holds eight), one copy (parts[i] bytes each, consecutive in the block)
int orbm_d2h_split(orbm_matcher *m, void *const *host, const size_t *parts, int nparts, const void *dev, hipStream_t s);
int orbm_sync(orbm_matcher *m, hipStream_t s);                                            // synchronise + deliver the D2H copies
// orbm_mappoint.hip: the status of a NULL handle where device work is needed (ORBX_E_HIP without a device, else ORBX_E_INVALID)
int orbm_no_handle();
// orbm_mfma.hip: dense best / second-best partials on the matrix cores (same partial format as k_best2_dense)
int orbm_mfma_splits(int nq_cap, int nt_cap, int nbatch);
int orbm_launch_dense_mfma(orbm_matcher *m, const uint8_t *d_q, const int32_t *d_nq, int nq_fixed, const uint8_t *d_t, const int32_t *d_nt,
                           int nt_fixed, long long qstride, long long tstride, int cap_q, int cap_t, int nbatch, int out_stride, int S,
                           uint2 *part, hipStream_t s);
// orbm_frustum.hip: k_frustum on device pointers.  w != NULL: also each point's SearchByProjection window (radius from the viewing
// cosine, th and the level's scale factor; levels [level-1, level]; r < 0 for a point not in view) for k_area_list
struct FrustumWindows { float th; float *x, *y, *r; int32_t *min_level, *max_level; };
void orbm_frustum_launch(const orbm_frame_view *d_view, int n, const uint8_t *d_skip, const float *d_xw, const float *d_normal,
                         const float *d_mf_max, const float *d_mf_min, float cos_limit, uint8_t *d_status, float *d_proj_x,
                         float *d_proj_y, float *d_proj_xr, int32_t *d_pred_level, float *d_view_cos, const FrustumWindows *w,
                         hipStream_t s);
int orbm_frustum_check(const orbm_frame_view *view, const uint8_t *skip, const float *xw, const float *normal, const float *mf_max,
                       const float *mf_min, const uint8_t *status, const float *proj_x, const float *proj_y, const float *proj_xr,
                       const int32_t *pred_level, const float *view_cos, const int *n_to_match);
// orbm_triangulate.hip: cam1's and every second view's nlevels in range, off2[0] == 0 and monotone (host arrays)
int orbm_tri_check_views(const orbm_camera *cam1, const orbm_camera *cams2, int nviews, const int32_t *off2);
// k_dist_csr (orbm.hip) for callers in other files: dist[c] of every CSR candidate, off has nq + 1 entries
void orbm_launch_dist_csr(const uint8_t *d_q, int nq, const uint8_t *d_t, const int32_t *d_off, const int32_t *d_idx, int total,
                          int32_t *d_dist, hipStream_t s);

// -------------------------------------------------------------------------------------------------
// host-only helpers
// -------------------------------------------------------------------------------------------------
// The host inputs of one call: list the parts, upload() sends them in ONE copy (every hipMemcpyAsync costs ~7 us of host time)
// through the pinned arena to its device mirror.  Before the arena has grown (first call on a handle, or the first call larger
// than any before it) the block lives in memory of its own, which goes with the InBlock.  Declare it before the kernels that
// read it are queued and let it go out of scope after the call's orbm_sync(): the temporary is never freed under a running kernel.
struct InBlock {
    struct Part { const void *src; size_t bytes, off; };
    orbm_matcher *m;
    std::vector<Part> parts;
    size_t total = 0, sent = (size_t)-1;       // sent: the bytes upload() copies (everything unless device_only_from_here())
    uint8_t *host = nullptr, *dev = nullptr;    // the block after upload()
    std::vector<uint8_t> tmp_host;
    void *tmp_dev = nullptr;
    explicit InBlock(orbm_matcher *m_) : m(m_) {}
    InBlock(const InBlock &) = delete;
    InBlock &operator=(const InBlock &) = delete;
    ~InBlock() { if (tmp_dev) (void)hipFree(tmp_dev); }
    int add(const void *src, size_t bytes)
    {
        parts.push_back({src, bytes, total});
        total += (bytes + 63) & ~(size_t)63;
        return (int)parts.size() - 1;
    }
    int reserve(size_t bytes) { return add(nullptr, bytes); }     // a part whose content comes later: fill()
    void device_only_from_here() { if (sent == (size_t)-1) sent = total; }   // the parts reserved after this are written by kernels:
                                                                             // room in the block, not part of the copy
    int upload(hipStream_t s)
    {
        if (total == 0) return ORBX_OK;
        m->arena_want += total;                          // when there is no room now, the next call has it
        if (m->arena_used + total <= m->arena_cap()) {
            host = m->arena + m->arena_used; dev = m->d_arena + m->arena_used;
            m->arena_used += total;
        } else {
            tmp_host.resize(total);
            MHIPCHK(hipMalloc(&tmp_dev, total));
            host = tmp_host.data(); dev = (uint8_t *)tmp_dev;
        }
        for (const Part &p : parts)
            if (p.src && p.bytes) memcpy(host + p.off, p.src, p.bytes);
        if (std::min(sent, total)) MHIPCHK(hipMemcpyAsync(dev, host, std::min(sent, total), hipMemcpyHostToDevice, s));
        if (tmp_dev) MHIPCHK(hipStreamSynchronize(s));   // pageable source
        return ORBX_OK;
    }
    int fill(int part, const void *src, hipStream_t s)   // content of a reserved part, after upload(): one more copy
    {
        const Part &p = parts[part];
        memcpy(host + p.off, src, p.bytes);
        MHIPCHK(hipMemcpyAsync(dev + p.off, host + p.off, p.bytes, hipMemcpyHostToDevice, s));
        return ORBX_OK;
    }
    // a reserved part the caller composes in place after upload(): host_at() is its host side, send() copies its first bytes
    uint8_t *host_at(int part) const { return host + parts[part].off; }
    int send(int part, size_t bytes, hipStream_t s)
    {
        if (bytes) MHIPCHK(hipMemcpyAsync(dev + parts[part].off, host + parts[part].off, bytes, hipMemcpyHostToDevice, s));
        return ORBX_OK;
    }
    template <class T> T *dev_at(int part) const { return reinterpret_cast<T *>(dev + parts[part].off); }
    template <class T> const T *at(int part) const { return parts[part].bytes ? reinterpret_cast<const T *>(dev + parts[part].off) : nullptr; }
};

// The results of one call that the kernel leaves in d_out, back to back: list the parts once (host array, bytes) in the order they
// lie there, an 8-byte type first.  words() is what d_out must hold (orbm_grow), dev_at() a part's device side (after orbm_grow:
// growth moves d_out), download() brings all of them home in one copy and ends the call (orbm_sync).
struct OutBlock {
    struct Part { void *host; size_t bytes; };
    void *host[4];
    size_t bytes[4], off[4], total = 0;
    int n = 0;
    OutBlock(std::initializer_list<Part> parts)
    {
        for (const Part &p : parts) { host[n] = p.host; bytes[n] = p.bytes; off[n++] = total; total += p.bytes; }
    }
    size_t words() const { return (total + 3) / 4; }
    template <class T> T *dev_at(orbm_matcher *m, int part) const { return reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(m->d_out.get()) + off[part]); }
    __attribute__((always_inline)) int download(orbm_matcher *m, hipStream_t s) const      // inlined: the library exports what it did
    {
        MTRY(orbm_d2h_split(m, host, bytes, n, m->d_out, s));
        return orbm_sync(m, s);
    }
};

// Rotation histogram of the matchers' orientation check (src/ORBmatcher.cc:236-246 and siblings) and the ComputeThreeMaxima cull
// (:266-284).  The bin arithmetic is the reference's: float difference, comparison with a double zero, roundf, no contraction.
struct RotHist {
    int32_t hist[ORBM_HISTO_LENGTH] = {0};
    std::vector<std::pair<int, int>> entries;           // rotHist as (bin, tag) in push order
    int add(float angle_a, float angle_b, int tag)
    {
        const float factor = 1.0f / ORBM_HISTO_LENGTH;
        float rot = angle_a - angle_b;
        if (rot < 0.0) rot += 360.0f;
        if (std::isnan(rot)) return mfail(ORBX_E_INVALID, "keypoint angle outside [0, 360)");      // no int holds it
        int bin = (int)roundf(rot * factor);
        if (bin == ORBM_HISTO_LENGTH) bin = 0;
        if (bin < 0 || bin >= ORBM_HISTO_LENGTH) return mfail(ORBX_E_INVALID, "keypoint angle outside [0, 360)");   // the reference asserts
        entries.emplace_back(bin, tag);
        hist[bin]++;
        return ORBX_OK;
    }
    template <class F> void cull(F drop)                // drop(tag) for every entry outside the three maxima, in push order
    {
        int32_t ind[3];
        orbm_three_maxima(hist, ORBM_HISTO_LENGTH, ind);
        for (const auto &e : entries)
            if (e.first != ind[0] && e.first != ind[1] && e.first != ind[2]) drop(e.second);
    }
};

// The window queries of a matcher whose scan is sequential on the host: add() one per usable MapPoint / keypoint, run() gathers
// their descriptors and fetches every window's candidates and distances (orbm_area_pairs): candidates of query k are
// idx / dist[off[k] .. off[k + 1]).
struct AreaQueries {
    std::vector<int> src;                   // index of the query in the caller's arrays
    std::vector<float> x, y, r;
    std::vector<int32_t> mn, mx, off, idx, dist;
    std::vector<uint8_t> desc;
    void add(int src_index, float qx, float qy, float qr, int min_level, int max_level)
    {
        src.push_back(src_index); x.push_back(qx); y.push_back(qy); r.push_back(qr); mn.push_back(min_level); mx.push_back(max_level);
    }
    int size() const { return (int)src.size(); }
    int run(orbm_matcher *m, const uint8_t *src_desc, const uint8_t *train_desc, int n_train)
    {
        const int nq = size();
        MTRY(orbm_grow(m, nq, 0, 0));
        desc.resize((size_t)nq * 32);
        for (int k = 0; k < nq; k++) memcpy(&desc[(size_t)k * 32], src_desc + (size_t)src[k] * 32, 32);
        const int total = orbm_area_pairs(m, x.data(), y.data(), r.data(), mn.data(), mx.data(), nq, desc.data(), train_desc, n_train, off, idx, dist);
        return total < 0 ? total : ORBX_OK;
    }
};

// cv::Mat algebra as OpenCV 3.1.0 evaluates it.  `R*x + t` on a 3x3 and a 3x1 float matrix is one cv::gemm(R, x, 1, t, 1, dst, 0)
// call, whose small-matrix path (modules/core/src/matmul.cpp: flags == 0, 2 <= len <= 4) sums the three float products in float,
// left to right, and finishes with (float)(t0*alpha + c*beta) in double.  `-A.t()*b` materialises the transpose and runs the same
// path with alpha = -1 and no C operand: c = zerof, beta = 0 (a zero sum comes out as +0).
static inline float gemm3(const float *a, int sa, const float *b, double alpha, float c, double beta)
{
    const float t0 = a[0] * b[0] + a[sa] * b[1] + a[2 * sa] * b[2];
    return (float)((double)t0 * alpha + (double)c * beta);
}
static inline float gemm_row(const float *T, int row, const float *x)   // (R x + t)[row] of a row-major [R|t]
{
    return gemm3(T + 4 * row, 1, x, 1.0, T[4 * row + 3], 1.0);
}
static inline void camera_center(const float *T, float Ow[3])           // -Rcw^T tcw
{
    const float t[3] = {T[3], T[7], T[11]};
    for (int k = 0; k < 3; k++) Ow[k] = gemm3(T + k, 4, t, -1.0, 0.f, 0.0);
}
