// orbm_mappoint.hip -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307 of WChen09/My-SLAM) for a whole batch
// of MapPoints in one call: orbm_distinctive_descriptors / orbm_distinctive_descriptors_device (include/orbm.h).
//
// Per point with rows D[0..N-1]: dist[i][j] = Hamming(D[i], D[j]) (:276-285), median[i] = element k = (N-1)/2 of row i sorted
// ascending, own 0 included (:292-294), best = the first i with the smallest median (:296-300).  Integer arithmetic only.
//
// No sort and no N x N matrix: distances lie in 0..256, so element k of a row is the smallest v with
// #{j : dist[i][j] <= v} > k, found by nine bisection steps over v that each recount the row (dd_select).  A thread owns one row
// (its descriptor stays in 8 VGPRs); the rows it is compared with come from LDS as wave-uniform broadcasts, or from global memory
// at a wave-uniform address in the last class.  "First smallest" is a minimum over keys median << s | i.
//
// Size classes by N (the batch is very skewed: mostly 2..15 rows, a tail of hundreds):
//   N <= 2                 no arithmetic: 0, or -1 for an empty run (both medians of N = 2 are the own 0)
//   3..DD_SMALL_MAX (16)   k_dd_small: 16 lanes per point, 4 points per wave; the 16 distances of a row stay in registers, so the
//                          bisection recounts registers.  This kernel visits every point: it answers N <= 2 and sorts the larger
//                          points into one list per class (atomic append; the order in a list does not reach the result)
//   17..DD_WAVE_MAX (64)   k_dd_wave: one wave per point, lane i owns row i, the point's rows in 2 KiB of LDS
//   65..DD_WG_MAX (256)    k_dd_wg: one 256-thread workgroup per point, the point's rows in 8 KiB of LDS
//   beyond                 k_dd_rows: no per-point limit.  Workgroup b owns the 256 consecutive rows 256 b .. 256 b + 255 of the CSR
//                          (they touch at most two points of this class, since each has more than 256 rows), a thread owns one
//                          row and reads its point's rows from global memory; a point's row blocks meet in a 64-bit atomicMin
//                          key, unpacked by k_dd_rows_finish.  A point of N rows is spread over N / 256 workgroups.
// The launches of a class are skipped when max_run says the class is empty; their grids are the worst case that (n_points,
// total_rows) allow, and surplus workgroups leave after reading the class's count.
#include <algorithm>
#include <cstring>

#include "orbm_internal.h"

#define DD_SMALL_MAX 16
#define DD_WAVE_MAX 64
#define DD_WG_MAX 256
#define DD_THREADS 256
#define DD_SMALL_PER_WG (DD_THREADS / DD_SMALL_MAX)
static_assert(DD_WAVE_MAX == 64 && DD_WG_MAX == DD_THREADS, "one lane / one thread per row");

// scratch header: the three list lengths (ints), then the lists; see DdScratch
#define DD_CNT_WAVE 0
#define DD_CNT_WG 1
#define DD_CNT_ROWS 2
#define DD_HEADER_INTS 16

// element k of a row sorted ascending: the smallest v in 0..256 with count_le(v) > k.  count_le(256) = N > k holds at the start
// and stays true of hi; 257 values need nine halvings, and a range that is already one value wide stays as it is.
template <class CountLE> __device__ __forceinline__ int dd_select(int k, CountLE count_le)
{
    int lo = 0, hi = 256;
    for (int step = 0; step < 9; step++) {
        const int mid = (lo + hi) >> 1;
        if (count_le(mid) > k) hi = mid; else lo = mid + 1;
    }
    return hi;
}

__device__ __forceinline__ void dd_store(int32_t *best, int32_t *best_median, int p, int idx, int med)
{
    best[p] = idx;
    if (best_median) best_median[p] = med;
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_small(const int32_t *__restrict__ off, const uint8_t *__restrict__ desc, int n_points,
                                                         int32_t *__restrict__ best, int32_t *__restrict__ best_median,
                                                         int32_t *__restrict__ cnt, int32_t *__restrict__ list_wave,
                                                         int32_t *__restrict__ list_wg, int32_t *__restrict__ list_rows,
                                                         unsigned long long *__restrict__ key)
{
    // one uint4 of padding per group: the four groups of a wave read row j at the same time, 528 B apart = 4 banks, no conflict
    __shared__ uint4 s[DD_SMALL_PER_WG][2 * DD_SMALL_MAX + 1];
    const int g = threadIdx.x / DD_SMALL_MAX, l = threadIdx.x % DD_SMALL_MAX;
    const int p = blockIdx.x * DD_SMALL_PER_WG + g;
    int n = 0, base = 0;
    if (p < n_points) { base = off[p]; n = off[p + 1] - base; }
    const bool mine = n >= 3 && n <= DD_SMALL_MAX;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (mine && l < n) {
        const uint4 *r = reinterpret_cast<const uint4 *>(desc + ((size_t)base + l) * 32);
        a0 = r[0]; a1 = r[1];
        s[g][2 * l] = a0; s[g][2 * l + 1] = a1;
    }
    __syncthreads();
    if (p >= n_points) return;
    if (n > DD_SMALL_MAX) {             // a larger class: append to its list
        if (l == 0) {
            if (n <= DD_WAVE_MAX) list_wave[atomicAdd(&cnt[DD_CNT_WAVE], 1)] = p;
            else if (n <= DD_WG_MAX) list_wg[atomicAdd(&cnt[DD_CNT_WG], 1)] = p;
            else { key[p] = ~0ull; list_rows[atomicAdd(&cnt[DD_CNT_ROWS], 1)] = p; }
        }
        return;
    }
    if (n <= 2) {                       // :256 / :269 (nothing to choose from) and N = 1, 2: every median is the own 0, the first row wins
        if (l == 0) dd_store(best, best_median, p, n > 0 ? 0 : -1, n > 0 ? 0 : -1);
        return;
    }
    int d[DD_SMALL_MAX];
#pragma unroll
    for (int j = 0; j < DD_SMALL_MAX; j++) {
        const uint4 b0 = s[g][2 * j], b1 = s[g][2 * j + 1];          // rows >= n hold stale LDS: read, never counted
        d[j] = j < n ? hamming256(a0, a1, b0, b1) : 512;
    }
    const int med = dd_select((n - 1) >> 1, [&](int v) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < DD_SMALL_MAX; j++) c += d[j] <= v;
        return c;
    });
    uint32_t kmin = l < n ? ((uint32_t)med << 8) | (uint32_t)l : 0xFFFFFFFFu;
#pragma unroll
    for (int m = 1; m < DD_SMALL_MAX; m <<= 1) kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, m, DD_SMALL_MAX));
    if (l == 0) dd_store(best, best_median, p, (int)(kmin & 0xFFu), (int)(kmin >> 8));
}

// count of rows j < n of an LDS-resident point within v of the row (a0, a1); every lane reads the same address
__device__ __forceinline__ int dd_count_lds(const uint4 *s, int n, const uint4 &a0, const uint4 &a1, int v)
{
    int c = 0;
#pragma unroll 4                        // four rows' reads in flight: one wave per SIMD would otherwise wait out every LDS latency
    for (int j = 0; j < n; j++) c += hamming256(a0, a1, s[2 * j], s[2 * j + 1]) <= v;
    return c;
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_wave(const int32_t *__restrict__ off, const uint8_t *__restrict__ desc,
                                                        const int32_t *__restrict__ cnt, const int32_t *__restrict__ list,
                                                        int32_t *__restrict__ best, int32_t *__restrict__ best_median)
{
    __shared__ uint4 s[DD_THREADS / 64][2 * DD_WAVE_MAX];
    const int w = threadIdx.x / 64, l = threadIdx.x % 64;
    const int slot = blockIdx.x * (DD_THREADS / 64) + w;
    const bool have = slot < cnt[DD_CNT_WAVE];
    int p = 0, n = 0, base = 0;
    if (have) { p = list[slot]; base = off[p]; n = off[p + 1] - base; }     // 17..64 by construction of the list
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (l < n) {
        const uint4 *r = reinterpret_cast<const uint4 *>(desc + ((size_t)base + l) * 32);
        a0 = r[0]; a1 = r[1];
        s[w][2 * l] = a0; s[w][2 * l + 1] = a1;
    }
    __syncthreads();
    if (!have) return;
    const int med = dd_select((n - 1) >> 1, [&](int v) { return dd_count_lds(s[w], n, a0, a1, v); });
    const uint32_t kmin = wave_min_u32(l < n ? ((uint32_t)med << 16) | (uint32_t)l : 0xFFFFFFFFu);
    if (l == 0) dd_store(best, best_median, p, (int)(kmin & 0xFFFFu), (int)(kmin >> 16));
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_wg(const int32_t *__restrict__ off, const uint8_t *__restrict__ desc,
                                                      const int32_t *__restrict__ cnt, const int32_t *__restrict__ list,
                                                      int32_t *__restrict__ best, int32_t *__restrict__ best_median)
{
    __shared__ uint4 s[2 * DD_WG_MAX];
    __shared__ uint32_t s_key;
    if ((int)blockIdx.x >= cnt[DD_CNT_WG]) return;         // uniform over the workgroup
    const int t = threadIdx.x;
    const int p = list[blockIdx.x], base = off[p], n = off[p + 1] - base;     // 65..256
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (t < n) {
        const uint4 *r = reinterpret_cast<const uint4 *>(desc + ((size_t)base + t) * 32);
        a0 = r[0]; a1 = r[1];
        s[2 * t] = a0; s[2 * t + 1] = a1;
    }
    if (t == 0) s_key = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t k = 0xFFFFFFFFu;
    if (t < n) k = ((uint32_t)dd_select((n - 1) >> 1, [&](int v) { return dd_count_lds(s, n, a0, a1, v); }) << 16) | (uint32_t)t;
    k = wave_min_u32(k);
    if (t % 64 == 0) atomicMin(&s_key, k);
    __syncthreads();
    if (t == 0) dd_store(best, best_median, p, (int)(s_key & 0xFFFFu), (int)(s_key >> 16));
}

// the point that holds global row r: the last p with off[p] <= r (empty runs share an offset with their successor and lose)
__device__ __forceinline__ int dd_point_of_row(const int32_t *__restrict__ off, int n_points, int r)
{
    int lo = 0, hi = n_points;          // smallest index with off[index] > r; off[n_points] = total_rows > r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] > r) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_rows(const int32_t *__restrict__ off, const uint8_t *__restrict__ desc, int n_points,
                                                        int total_rows, unsigned long long *__restrict__ key)
{
    const int first = blockIdx.x * DD_THREADS, last = min(first + DD_THREADS, total_rows) - 1;
    const int r = first + threadIdx.x;
    const int pa = dd_point_of_row(off, n_points, first), pb = dd_point_of_row(off, n_points, last);
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (r <= last) {
        const uint4 *q = reinterpret_cast<const uint4 *>(desc + (size_t)r * 32);
        a0 = q[0]; a1 = q[1];
    }
    // every point between pa and pb lies inside these 256 rows, so it is not of this class
    for (int side = 0; side < 2; side++) {
        const int p = side == 0 ? pa : pb;
        if (side == 1 && pb == pa) break;
        const int base = off[p], n = off[p + 1] - base;
        if (n <= DD_WG_MAX) continue;
        const bool in = r >= base && r < base + n && r <= last;
        const uint4 *rows = reinterpret_cast<const uint4 *>(desc + (size_t)base * 32);
        int med = 0x7FFF;
        if (in)
            med = dd_select((n - 1) >> 1, [&](int v) {
                int c = 0;
#pragma unroll 4
                for (int j = 0; j < n; j++) c += hamming256(a0, a1, rows[2 * j], rows[2 * j + 1]) <= v;
                return c;
            });
        // first smallest inside the wave, then one atomic per wave: median in the high word, row in the low word
        const uint32_t mmin = wave_min_u32((uint32_t)med);
        const uint32_t imin = wave_min_u32(in && (uint32_t)med == mmin ? (uint32_t)(r - base) : 0xFFFFFFFFu);
        if (threadIdx.x % 64 == 0 && imin != 0xFFFFFFFFu) atomicMin(&key[p], ((unsigned long long)mmin << 32) | imin);
    }
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_rows_finish(const int32_t *__restrict__ cnt, const int32_t *__restrict__ list,
                                                               const unsigned long long *__restrict__ key,
                                                               int32_t *__restrict__ best, int32_t *__restrict__ best_median)
{
    const int slot = blockIdx.x * DD_THREADS + threadIdx.x;
    if (slot >= cnt[DD_CNT_ROWS]) return;
    const int p = list[slot];
    dd_store(best, best_median, p, (int)(key[p] & 0xFFFFFFFFull), (int)(key[p] >> 32));
}

// ---- host side ----
// Scratch of the feature, one device block in the handle (grown, never shrunk; it is this call's own, so no other call's state --
// the grid, the staging buffers -- changes with it):
//   [header: DD_HEADER_INTS ints][key: n_points x 8 B][lists: 3 x n_points ints]  and, for the host-pointer entry point,
//   [out: 2 x n_points ints][off: n_points + 1 ints][desc: total_rows x 32 B]
struct DdScratch {
    int32_t *cnt, *list_wave, *list_wg, *list_rows, *out, *off;
    unsigned long long *key;
    uint8_t *desc;
};
static size_t dd_align(size_t b) { return (b + 255) & ~(size_t)255; }
static int dd_scratch(orbm_matcher *m, int n_points, long long host_rows, hipStream_t s, DdScratch *sc)
{
    const size_t np = (size_t)n_points;
    size_t o_key = dd_align((size_t)DD_HEADER_INTS * 4), o_lists = o_key + dd_align(np * 8), o_out = o_lists + dd_align(3 * np * 4);
    size_t o_off = o_out, o_desc = o_out, need = o_out;
    if (host_rows >= 0) {
        o_off = o_out + dd_align(2 * np * 4); o_desc = o_off + dd_align((np + 1) * 4); need = o_desc + dd_align((size_t)host_rows * 32);
    }
    MTRY(orbm_ensure_dd(m, need, s));
    uint8_t *b = m->d_dd;
    sc->cnt = (int32_t *)b;
    sc->key = (unsigned long long *)(b + o_key);
    sc->list_wave = (int32_t *)(b + o_lists); sc->list_wg = sc->list_wave + np; sc->list_rows = sc->list_wg + np;
    sc->out = (int32_t *)(b + o_out); sc->off = (int32_t *)(b + o_off); sc->desc = b + o_desc;
    return ORBX_OK;
}

static int dd_launch(const DdScratch &sc, int n_points, const int32_t *d_off, const uint8_t *d_desc, int total_rows, int max_run,
                     int32_t *d_best, int32_t *d_best_median, hipStream_t s)
{
    MHIPCHK(hipMemsetAsync(sc.cnt, 0, (size_t)DD_HEADER_INTS * 4, s));
    hipLaunchKernelGGL(k_dd_small, dim3((n_points + DD_SMALL_PER_WG - 1) / DD_SMALL_PER_WG), dim3(DD_THREADS), 0, s,
                       d_off, d_desc, n_points, d_best, d_best_median, sc.cnt, sc.list_wave, sc.list_wg, sc.list_rows, sc.key);
    // a class of runs longer than B has at most total_rows / (B + 1) points
    if (max_run > DD_SMALL_MAX) {
        const int most = std::min(n_points, total_rows / (DD_SMALL_MAX + 1));
        hipLaunchKernelGGL(k_dd_wave, dim3((most + DD_THREADS / 64 - 1) / (DD_THREADS / 64)), dim3(DD_THREADS), 0, s,
                           d_off, d_desc, sc.cnt, sc.list_wave, d_best, d_best_median);
    }
    if (max_run > DD_WAVE_MAX) {
        const int most = std::min(n_points, total_rows / (DD_WAVE_MAX + 1));
        hipLaunchKernelGGL(k_dd_wg, dim3(most), dim3(DD_THREADS), 0, s, d_off, d_desc, sc.cnt, sc.list_wg, d_best, d_best_median);
    }
    if (max_run > DD_WG_MAX) {
        const int most = std::min(n_points, total_rows / (DD_WG_MAX + 1));
        hipLaunchKernelGGL(k_dd_rows, dim3((total_rows + DD_THREADS - 1) / DD_THREADS), dim3(DD_THREADS), 0, s,
                           d_off, d_desc, n_points, total_rows, sc.key);
        hipLaunchKernelGGL(k_dd_rows_finish, dim3((most + DD_THREADS - 1) / DD_THREADS), dim3(DD_THREADS), 0, s,
                           sc.cnt, sc.list_rows, sc.key, d_best, d_best_median);
    }
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

// a NULL handle where device work is needed: without a device that is the library's "no CPU path" failure, with one a bad argument
int orbm_no_handle()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return mfail(ORBX_E_HIP, "no HIP device: liborbx has no CPU path");
    }
    return mfail(ORBX_E_INVALID, "NULL handle");
}

extern "C" int orbm_distinctive_descriptors(orbm_matcher *m, int n_points, const int32_t *off, const uint8_t *desc,
                                            int32_t *best, int32_t *best_median)
{
    if (n_points < 0) return mfail(ORBX_E_INVALID, "n_points=%d", n_points);
    if (n_points == 0) return ORBX_OK;
    if (!off || !best) return mfail(ORBX_E_INVALID, "NULL buffer");
    if (off[0] != 0) return mfail(ORBX_E_INVALID, "off[0] must be 0");
    int max_run = 0;
    for (int p = 0; p < n_points; p++) {
        if (off[p + 1] < off[p]) return mfail(ORBX_E_INVALID, "off not monotone at %d", p);
        max_run = std::max(max_run, off[p + 1] - off[p]);
    }
    const int total_rows = off[n_points];
    if (total_rows > (1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 descriptors");
    if (total_rows > 0 && !desc) return mfail(ORBX_E_INVALID, "desc is NULL");
    if (max_run <= 2) {                 // freshly made points (Tracking.cc, CreateNewMapPoints): nothing to compute, nothing to launch
        for (int p = 0; p < n_points; p++) {
            best[p] = off[p + 1] > off[p] ? 0 : -1;
            if (best_median) best_median[p] = best[p];
        }
        return ORBX_OK;
    }
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    DdScratch sc;
    MTRY(dd_scratch(m, n_points, total_rows, s, &sc));
    MTRY(orbm_arena_begin(m));
    MTRY(orbm_h2d(m, sc.off, off, ((size_t)n_points + 1) * 4, s));
    MTRY(orbm_h2d(m, sc.desc, desc, (size_t)total_rows * 32, s));
    MTRY(dd_launch(sc, n_points, sc.off, sc.desc, total_rows, max_run, sc.out, sc.out + n_points, s));
    void *host[2] = {best, best_median};
    const size_t parts[2] = {(size_t)n_points * 4, (size_t)n_points * 4};
    MTRY(orbm_d2h_split(m, host, parts, best_median ? 2 : 1, sc.out, s));
    return orbm_sync(m, s);
}

extern "C" int orbm_distinctive_descriptors_device(orbm_matcher *m, int n_points, const int32_t *d_off, const uint8_t *d_desc,
                                                   int total_rows, int max_run, int32_t *d_best, int32_t *d_best_median,
                                                   void *hip_stream)
{
    if (n_points < 0 || total_rows < 0 || max_run < 0 || max_run > total_rows)
        return mfail(ORBX_E_INVALID, "n_points=%d total_rows=%d max_run=%d", n_points, total_rows, max_run);
    if (n_points == 0) return ORBX_OK;
    if (total_rows > (1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 descriptors");
    if (!d_off || !d_best || (total_rows > 0 && !d_desc)) return mfail(ORBX_E_INVALID, "NULL buffer");
    if ((uintptr_t)d_desc & 15) return mfail(ORBX_E_INVALID, "d_desc must be 16-byte aligned");
    if (!m) return orbm_no_handle();
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    DdScratch sc;
    MTRY(dd_scratch(m, n_points, -1, s, &sc));
    return dd_launch(sc, n_points, d_off, d_desc, total_rows, max_run, d_best, d_best_median, s);
}
