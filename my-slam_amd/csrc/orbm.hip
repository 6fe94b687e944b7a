// orbm.hip -- gfx950 Hamming matcher primitives + their C ABI (include/orbm.h).
// Reference: src/ORBmatcher.cc of WChen09/My-SLAM (DescriptorDistance :1647-1663, best/second-best
// loops :201-232 and siblings, ComputeThreeMaxima :1601-1642).  Integer/bitwise only: v_xor_b32 +
// v_bcnt_u32_b32 (popcount with accumulate); the train set goes through LDS tiles and is read back as
// wave-uniform broadcasts, so the kernel is VALU-bound, not HBM-bound (16 M pairs
// touch 256 KB).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "orbm_internal.h"
#include "orbm_accept.h"
#include "orbm_bow_body.h"

// ---- pinned staging arena (see orbm_internal.h; orbm_arena_begin is in orbm_workspace.cc) ----
static void *arena_take(orbm_matcher *m, size_t bytes)
{
    const size_t a = (bytes + 63) & ~(size_t)63;
    m->arena_want += a;
    if (m->arena_used + a > m->arena_cap()) return nullptr;     // this call falls back to a pageable copy; the next one has room
    void *p = m->arena + m->arena_used;
    m->arena_used += a;
    return p;
}
int orbm_h2d(orbm_matcher *m, void *dev, const void *host, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return ORBX_OK;
    void *p = arena_take(m, bytes);
    if (p) { memcpy(p, host, bytes); host = p; }
    MHIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
    return ORBX_OK;
}
int orbm_d2h(orbm_matcher *m, void *host, const void *dev, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return ORBX_OK;
    void *p = m->npend < 8 ? arena_take(m, bytes) : nullptr;
    if (p) { m->pend[m->npend++] = {host, p, bytes}; host = p; }
    MHIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    return ORBX_OK;
}
int orbm_d2h_split(orbm_matcher *m, void *const *host, const size_t *parts, int nparts, const void *dev, hipStream_t s)
{
    size_t total = 0;
    for (int i = 0; i < nparts; i++) total += parts[i];
    if (total == 0) return ORBX_OK;
    uint8_t *p = (m->npend + nparts <= 8) ? (uint8_t *)arena_take(m, total) : nullptr;
    if (!p) {     // no room in the arena this call: one copy per part
        size_t o = 0;
        for (int i = 0; i < nparts; i++) {
            MTRY(orbm_d2h(m, host[i], (const uint8_t *)dev + o, parts[i], s));
            o += parts[i];
        }
        return ORBX_OK;
    }
    MHIPCHK(hipMemcpyAsync(p, dev, total, hipMemcpyDeviceToHost, s));
    size_t o = 0;
    for (int i = 0; i < nparts; i++) { m->pend[m->npend++] = {host[i], p + o, parts[i]}; o += parts[i]; }
    return ORBX_OK;
}
int orbm_sync(orbm_matcher *m, hipStream_t s)
{
    MHIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < m->npend; i++) memcpy(m->pend[i].dst, m->pend[i].src, m->pend[i].bytes);
    m->npend = 0;
    return ORBX_OK;
}

// ---- dense best/second-best: one query per thread (8 VGPRs); the train range of a workgroup is
// staged through double-buffered 4 KiB LDS tiles and read back as wave-uniform broadcasts
// (2 x ds_read_b128 per pair against 22 VALU ops).  gridDim.z splits the train range for occupancy; every split writes a partial
// (best key, second key) with key = distance << 22 | train index, so "strictly smaller wins, first
// index wins a tie, a tie with the best becomes the second best" (src/ORBmatcher.cc:214-223) is
// min / median on keys and partials merge exactly (k_merge_best2 / k_accept_rot). ----
#define M_TILE 128   // train descriptors staged per LDS tile (4 KiB)
__global__ __launch_bounds__(M_THREADS) void k_best2_dense(
    const uint8_t *__restrict__ q, const int32_t *__restrict__ nqv, int nq_fixed,
    const uint8_t *__restrict__ t, const int32_t *__restrict__ ntv, int nt_fixed,
    long long qstride, long long tstride, int out_stride, uint2 *__restrict__ part)
{
    __shared__ uint4 tile[2][M_TILE * 2];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nq = nqv ? nqv[b] : nq_fixed;
    const int nt = ntv ? ntv[b] : nt_fixed;
    if ((int)(blockIdx.x * M_THREADS) >= nq) return;
    const int qi = blockIdx.x * M_THREADS + tid;
    const int S = gridDim.z, chunk = (nt + S - 1) / S;
    const int j0 = blockIdx.z * chunk, j1 = min(nt, j0 + chunk);
    const uint4 *Q = reinterpret_cast<const uint4 *>(q + (long long)b * qstride);
    const uint4 *T = reinterpret_cast<const uint4 *>(t + (long long)b * tstride);
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (qi < nq) { q0 = Q[2 * qi]; q1 = Q[2 * qi + 1]; }
    uint32_t bk = M_KEY_NONE, sk = M_KEY_NONE;
    // double-buffered tiles: the loads of tile k+1 are in flight while tile k is scanned
    int cnt = min(M_TILE, j1 - j0);
    if (tid < cnt * 2) tile[0][tid] = T[2 * j0 + tid];
    int buf = 0;
    for (int t0 = j0; t0 < j1; t0 += M_TILE) {
        const int ncnt = min(M_TILE, j1 - (t0 + M_TILE));
        uint4 pre = make_uint4(0, 0, 0, 0);
        if (tid < ncnt * 2) pre = T[2 * (t0 + M_TILE) + tid];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const uint32_t key = ((uint32_t)hamming256(q0, q1, tile[buf][2 * j], tile[buf][2 * j + 1]) << 22) | (uint32_t)(t0 + j);
            sk = med3u(bk, sk, key);                            // second smallest of {bk <= sk, key}
            bk = min(bk, key);
        }
        if (tid < ncnt * 2) tile[buf ^ 1][tid] = pre;
        buf ^= 1;
        cnt = ncnt;
    }
    if (qi < nq) part[((long long)blockIdx.z * gridDim.y + b) * out_stride + qi] = make_uint2(bk, sk);
}

__global__ __launch_bounds__(M_THREADS) void k_merge_best2(const uint2 *__restrict__ part, int S, int nq,
                                                          int32_t *__restrict__ best_idx, int32_t *__restrict__ best_d,
                                                          int32_t *__restrict__ second_d)
{
    const int i = blockIdx.x * M_THREADS + threadIdx.x;
    if (i >= nq) return;
    int bi, bd, sd;
    merge_partials(part, S, nq, i, bi, bd, sd);
    best_idx[i] = bi; best_d[i] = bd; second_d[i] = sd;
}

// ---- CSR best/second-best: one wave per query ----
__global__ __launch_bounds__(M_THREADS) void k_best2_csr(
    const uint8_t *__restrict__ q, int nq, const uint8_t *__restrict__ t,
    const int32_t *__restrict__ off, const int32_t *__restrict__ idx,
    int32_t *__restrict__ best_idx, int32_t *__restrict__ best_d, int32_t *__restrict__ second_d)
{
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (M_THREADS / 64) + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const uint4 *Q = reinterpret_cast<const uint4 *>(q) + 2 * (long long)qi;
    const uint4 q0 = Q[0], q1 = Q[1];
    const int lo = off[qi], hi = off[qi + 1];
    // pack = dist << 22 | position: min() picks the smallest distance, earliest position
    uint32_t bp = (256u << 22) | 0x3FFFFFu, s = 256;
    for (int c = lo + lane; c < hi; c += 64) {
        const uint4 *Tj = reinterpret_cast<const uint4 *>(t) + 2 * (long long)idx[c];
        const uint32_t d = (uint32_t)hamming256(q0, q1, Tj[0], Tj[1]);
        const uint32_t p = (d << 22) | (uint32_t)min(c - lo, 0x3FFFFF);
        if (p < bp) { s = bp >> 22; bp = p; }
        else if (d < s) s = d;
    }
    uint32_t B, S;
    wave_best2<22>(bp, s, B, S);
    if (lane == 0) {
        const int d = (int)(B >> 22);
        best_d[qi] = d;
        second_d[qi] = (int)S;
        best_idx[qi] = d < 256 ? idx[lo + (int)(B & 0x3FFFFFu)] : -1;
    }
}

// ---- per-candidate distances ----
__global__ __launch_bounds__(M_THREADS) void k_dist_csr(
    const uint8_t *__restrict__ q, int nq, const uint8_t *__restrict__ t,
    const int32_t *__restrict__ off, const int32_t *__restrict__ idx, int total, int32_t *__restrict__ dist)
{
    const int c = blockIdx.x * M_THREADS + threadIdx.x;
    if (c >= total) return;
    int lo = 0, hi = nq;   // largest i with off[i] <= c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= c) lo = mid; else hi = mid;
    }
    const uint4 *Q = reinterpret_cast<const uint4 *>(q) + 2 * (long long)lo;
    const uint4 *Tj = reinterpret_cast<const uint4 *>(t) + 2 * (long long)idx[c];
    dist[c] = hamming256(Q[0], Q[1], Tj[0], Tj[1]);
}

void orbm_launch_dist_csr(const uint8_t *d_q, int nq, const uint8_t *d_t, const int32_t *d_off, const int32_t *d_idx, int total,
                          int32_t *d_dist, hipStream_t s)
{
    if (total > 0)
        hipLaunchKernelGGL(k_dist_csr, dim3((unsigned)((total + M_THREADS - 1) / M_THREADS)), dim3(M_THREADS), 0, s, d_q, nq, d_t, d_off, d_idx, total, d_dist);
}

// pairs given explicitly as (query << 16 | train), both below 65536: no per-thread binary search over off[]
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

__global__ __launch_bounds__(M_THREADS) void k_dist_dense(
    const uint8_t *__restrict__ q, int nq, const uint8_t *__restrict__ t, int nt, int32_t *__restrict__ dist)
{
    const long long c = (long long)blockIdx.x * M_THREADS + threadIdx.x;
    if (c >= (long long)nq * nt) return;
    const int i = (int)(c / nt), j = (int)(c - (long long)i * nt);
    const uint4 *Q = reinterpret_cast<const uint4 *>(q) + 2 * (long long)i;
    const uint4 *Tj = reinterpret_cast<const uint4 *>(t) + 2 * (long long)j;
    dist[c] = hamming256(Q[0], Q[1], Tj[0], Tj[1]);
}

// Many splits (few, large frame pairs): k_accept_rot is one workgroup per pair and would pull S partials per query through
// one CU.  This grid-wide pre-merge leaves one (best, second) key pair per query, which merges like a single partial.
__global__ __launch_bounds__(M_THREADS) void k_merge_keys(const uint2 *__restrict__ part, int S, const int32_t *__restrict__ nqv,
                                                         int cap, uint2 *__restrict__ merged)
{
    const int b = blockIdx.y, i = blockIdx.x * M_THREADS + threadIdx.x;
    if (i >= nqv[b] || i >= cap) return;
    const long long o = (long long)b * cap + i;
    uint32_t bk, sk;
    merge_partial_keys(part, S, (long long)gridDim.y * cap, o, bk, sk);
    merged[o] = make_uint2(bk, sk);
}

// ---- acceptance (:228-232) + rotation histogram (:236-246) + ComputeThreeMaxima + cull (:266-284): orbm_accept.h ----
__global__ __launch_bounds__(ACC_THREADS) void k_accept_rot(
    const int32_t *__restrict__ nqv, const orbx_keypoint *__restrict__ kq, const orbx_keypoint *__restrict__ kt,
    int cap, const uint2 *__restrict__ part, int S, int th, float nnratio, int check_ori,
    int32_t *__restrict__ match12, int32_t *__restrict__ nmatches,
    int32_t *__restrict__ best_idx, int32_t *__restrict__ best_d, int32_t *__restrict__ second_d)
{
    __shared__ AcceptShared sh;
    accept_rot_body<ACC_THREADS>(sh, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, nqv, kq, kt, cap, part, S, th, nnratio, check_ori,
                                 match12, nmatches, best_idx, best_d, second_d);
}

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
extern "C" int orbm_distance(const uint8_t a[32], const uint8_t b[32])
{
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t pa, pb;
        memcpy(&pa, a + 4 * i, 4);
        memcpy(&pb, b + 4 * i, 4);
        dist += __builtin_popcount(pa ^ pb);
    }
    return dist;
}

static int check_csr(const int32_t *off, const int32_t *idx, int nq, int nt, int *total)
{
    if (off[0] != 0) return mfail(ORBX_E_INVALID, "cand_off[0] must be 0");
    for (int i = 0; i < nq; i++)
        if (off[i + 1] < off[i]) return mfail(ORBX_E_INVALID, "cand_off not monotone at %d", i);
    *total = off[nq];
    if (*total > 0 && !idx) return mfail(ORBX_E_INVALID, "cand_idx is NULL");
    for (int c = 0; c < *total; c++)
        if (idx[c] < 0 || idx[c] >= nt) return mfail(ORBX_E_INVALID, "cand_idx[%d]=%d outside [0,%d)", c, idx[c], nt);
    return ORBX_OK;
}

// train-range splits so that the launch has >= ~4 waves per SIMD (1024 SIMDs); <= 64
#define ORBM_PREMERGE_SPLITS 16
static int pick_splits(int nq_cap, int nbatch, int nt_hint)
{
    const long long waves = (long long)nbatch * ((nq_cap + M_THREADS - 1) / M_THREADS) * (M_THREADS / 64);
    // ~12 waves per SIMD over the launch (measured on MI355X: 2048..16384 waves -> 76, 69, 64, 62, 57, 58 us for 63 x 1007^2
    // pairs): more, shorter waves hide the LDS broadcast latency and even out the tail
    int S = (int)((12288 + waves - 1) / waves);
    S = std::max(1, std::min(S, 64));
    while (S > 1 && nt_hint / S < 16) S--;       // keep >= 16 train descriptors per split
    return S;
}
extern "C" int orbm_best2(orbm_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                          const int32_t *cand_off, const int32_t *cand_idx,
                          int32_t *best_idx, int32_t *best_d, int32_t *second_d)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (nq < 0 || nt < 0) return mfail(ORBX_E_INVALID, "nq=%d nt=%d", nq, nt);
    MTRY(orbm_grow(m, nq, nt, cand_off && nq > 0 ? cand_off[nq] : 0));
    if (nq == 0) return ORBX_OK;
    if (!q || !best_idx || !best_d || !second_d || (nt > 0 && !t)) return mfail(ORBX_E_INVALID, "NULL buffer");
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    MTRY(orbm_h2d(m, m->d_q, q, (size_t)nq * 32, s));
    if (nt > 0) MTRY(orbm_h2d(m, m->d_t, t, (size_t)nt * 32, s));
    int32_t *o_bi = m->d_out, *o_bd = m->d_out + nq, *o_sd = m->d_out + 2 * (size_t)nq;
    if (cand_off) {
        int total = 0;
        MTRY(check_csr(cand_off, cand_idx, nq, nt, &total));
        MTRY(orbm_h2d(m, m->d_off, cand_off, ((size_t)nq + 1) * 4, s));
        if (total > 0) MTRY(orbm_h2d(m, m->d_idx, cand_idx, (size_t)total * 4, s));
        hipLaunchKernelGGL(k_best2_csr, dim3((nq + 3) / 4), dim3(M_THREADS), 0, s, m->d_q, nq, m->d_t, m->d_off, m->d_idx, o_bi, o_bd, o_sd);
    } else {
        const int S = m->dense_popcount ? pick_splits(nq, 1, nt) : orbm_mfma_splits(nq, nt, 1);
        int rc = orbm_ensure_partials(m, (size_t)S * nq);
        if (rc != ORBX_OK) return rc;
        if (m->dense_popcount)
            hipLaunchKernelGGL(k_best2_dense, dim3((nq + M_THREADS - 1) / M_THREADS, 1, S), dim3(M_THREADS), 0, s,
                               m->d_q, (const int32_t *)nullptr, nq, m->d_t, (const int32_t *)nullptr, nt, 0LL, 0LL, nq, m->d_part);
        else if ((rc = orbm_launch_dense_mfma(m, m->d_q, nullptr, nq, m->d_t, nullptr, nt, 0LL, 0LL, nq, std::max(nt, 1), 1, nq, S, m->d_part, s)) != ORBX_OK)
            return rc;
        hipLaunchKernelGGL(k_merge_best2, dim3((nq + M_THREADS - 1) / M_THREADS), dim3(M_THREADS), 0, s, m->d_part, S, nq, o_bi, o_bd, o_sd);
    }
    MHIPCHK(hipGetLastError());
    MTRY(orbm_d2h(m, best_idx, o_bi, (size_t)nq * 4, s));
    MTRY(orbm_d2h(m, best_d, o_bd, (size_t)nq * 4, s));
    MTRY(orbm_d2h(m, second_d, o_sd, (size_t)nq * 4, s));
    MTRY(orbm_sync(m, s));
    return ORBX_OK;
}

extern "C" int orbm_distances(orbm_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                              const int32_t *cand_off, const int32_t *cand_idx, int32_t *dist)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (nq < 0 || nt < 0) return mfail(ORBX_E_INVALID, "nq=%d nt=%d", nq, nt);
    MTRY(orbm_grow(m, nq, nt, cand_off && nq > 0 ? cand_off[nq] : (long long)nq * nt));
    if (nq == 0 || nt == 0) return ORBX_OK;
    if (!q || !t || !dist) return mfail(ORBX_E_INVALID, "NULL buffer");
    MHIPCHK(hipSetDevice(m->device));
    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    MTRY(orbm_h2d(m, m->d_q, q, (size_t)nq * 32, s));
    MTRY(orbm_h2d(m, m->d_t, t, (size_t)nt * 32, s));
    long long total;
    if (cand_off) {
        int tot = 0;
        MTRY(check_csr(cand_off, cand_idx, nq, nt, &tot));
        total = tot;
        if (total == 0) return ORBX_OK;
        MTRY(orbm_h2d(m, m->d_off, cand_off, ((size_t)nq + 1) * 4, s));
        MTRY(orbm_h2d(m, m->d_idx, cand_idx, (size_t)total * 4, s));
        hipLaunchKernelGGL(k_dist_csr, dim3((unsigned)((total + M_THREADS - 1) / M_THREADS)), dim3(M_THREADS), 0, s,
                           m->d_q, nq, m->d_t, m->d_off, m->d_idx, (int)total, m->d_out);
    } else {
        total = (long long)nq * nt;
        if (total > (long long)m->d_out.count())
            return mfail(ORBX_E_CAPACITY, "dense distances need %lld ints, matcher sized for %d pairs", total, m->max_pairs());
        hipLaunchKernelGGL(k_dist_dense, dim3((unsigned)((total + M_THREADS - 1) / M_THREADS)), dim3(M_THREADS), 0, s,
                           m->d_q, nq, m->d_t, nt, m->d_out);
    }
    MHIPCHK(hipGetLastError());
    MTRY(orbm_d2h(m, dist, m->d_out, (size_t)total * 4, s));
    MTRY(orbm_sync(m, s));
    return ORBX_OK;
}

static int launch_dense_batch(orbm_matcher *m, const uint8_t *d_q, const int32_t *d_nq, const uint8_t *d_t,
                              const int32_t *d_nt, int cap, int nbatch, hipStream_t s, int *S_out)
{
    const int S = m->dense_popcount ? pick_splits(cap, nbatch, cap) : orbm_mfma_splits(cap, cap, nbatch);
    int rc = orbm_ensure_partials(m, (size_t)(S + 1) * nbatch * cap, s);     // + one slot per query for k_merge_keys
    if (rc != ORBX_OK) return rc;
    if (m->dense_popcount)
        hipLaunchKernelGGL(k_best2_dense, dim3((cap + M_THREADS - 1) / M_THREADS, nbatch, S), dim3(M_THREADS), 0, s,
                           d_q, d_nq, 0, d_t, d_nt, 0, (long long)cap * 32, (long long)cap * 32, cap, m->d_part);
    else if ((rc = orbm_launch_dense_mfma(m, d_q, d_nq, 0, d_t, d_nt, 0, (long long)cap * 32, (long long)cap * 32, cap, cap, nbatch, cap, S, m->d_part, s)) != ORBX_OK)
        return rc;
    MHIPCHK(hipGetLastError());
    *S_out = S;
    return ORBX_OK;
}

// all-ones acceptance (th = 256 never rejects a found match; nnratio huge) is not what best2 wants:
// k_accept_rot also exports the merged (best_idx, best_d, second_d) when given the arrays.
extern "C" int orbm_match_batch_device(orbm_matcher *m, const uint8_t *d_q, const orbx_keypoint *d_kq,
                                       const int32_t *d_nq, const uint8_t *d_t, const orbx_keypoint *d_kt,
                                       const int32_t *d_nt, int cap, int nbatch, int th, float nnratio,
                                       int check_orientation, int32_t *d_match12, int32_t *d_nmatches, void *hip_stream)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (!d_q || !d_nq || !d_t || !d_nt || !d_kq || !d_kt || !d_match12 || !d_nmatches) return mfail(ORBX_E_INVALID, "NULL device pointer");
    if (cap < 1 || nbatch < 1 || cap > 0x3FFFFF) return mfail(ORBX_E_INVALID, "cap=%d nbatch=%d", cap, nbatch);
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    int S = 1;
    // (The acceptance as the tail of the LAST workgroup of a pair inside the match launch -- arrival counter, agent-scope release /
    // acquire -- was built and measured in round 3: identical tables, 76.7 us against 22.9 + 6.6: every workgroup's release is an L2
    // write-back on this multi-XCD part.  It stays a launch of its own.)
    MTRY(launch_dense_batch(m, d_q, d_nq, d_t, d_nt, cap, nbatch, s, &S));
    const uint2 *part = m->d_part;
    if (S > ORBM_PREMERGE_SPLITS) {
        uint2 *merged = m->d_part + (size_t)S * nbatch * cap;
        hipLaunchKernelGGL(k_merge_keys, dim3((cap + M_THREADS - 1) / M_THREADS, nbatch), dim3(M_THREADS), 0, s, m->d_part, S, d_nq, cap, merged);
        part = merged; S = 1;
    }
    hipLaunchKernelGGL(k_accept_rot, dim3(nbatch), dim3(ACC_THREADS), 0, s, d_nq, d_kq, d_kt, cap, part, S,
                       th, nnratio, check_orientation, d_match12, d_nmatches,
                       (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

__global__ __launch_bounds__(M_THREADS) void k_merge_batch(const uint2 *__restrict__ part, int S, const int32_t *__restrict__ nqv,
                                                          int cap, int32_t *__restrict__ best_idx,
                                                          int32_t *__restrict__ best_d, int32_t *__restrict__ second_d)
{
    const int b = blockIdx.y, i = blockIdx.x * M_THREADS + threadIdx.x;
    if (i >= cap) return;
    const long long o = (long long)b * cap + i;
    int bi = -1, bd = 256, sd = 256;
    if (i < nqv[b]) merge_partials(part, S, (long long)gridDim.y * cap, o, bi, bd, sd);
    best_idx[o] = bi; best_d[o] = bd; second_d[o] = sd;
}

extern "C" int orbm_best2_batch_device(orbm_matcher *m, const uint8_t *d_q, const int32_t *d_nq,
                                       const uint8_t *d_t, const int32_t *d_nt, int cap, int nbatch,
                                       int32_t *d_best_idx, int32_t *d_best_d, int32_t *d_second_d, void *hip_stream)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (!d_q || !d_nq || !d_t || !d_nt || !d_best_idx || !d_best_d || !d_second_d) return mfail(ORBX_E_INVALID, "NULL device pointer");
    if (cap < 1 || nbatch < 1 || cap > 0x3FFFFF) return mfail(ORBX_E_INVALID, "cap=%d nbatch=%d", cap, nbatch);
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : m->stream;
    int S = 1;
    MTRY(launch_dense_batch(m, d_q, d_nq, d_t, d_nt, cap, nbatch, s, &S));
    hipLaunchKernelGGL(k_merge_batch, dim3((cap + M_THREADS - 1) / M_THREADS, nbatch), dim3(M_THREADS), 0, s,
                       m->d_part, S, d_nq, cap, d_best_idx, d_best_d, d_second_d);
    MHIPCHK(hipGetLastError());
    return ORBX_OK;
}

// ---- N2: SearchByBoW's selection on the GPU (src/ORBmatcher.cc:199-232).  One wave per pair of equal vocabulary nodes: the
// node's key-frame features are visited in order (the loop is sequential in the reference because a frame feature taken by an
// earlier key-frame feature is skipped, :209), the lanes hold the node's frame features (position = chunk * 64 + lane, a
// "taken" bit per chunk in a register), key = distance << 16 | position so that min() is "smallest distance, first in list".
// A frame feature lives in exactly one node, so nodes do not interact. ----
__global__ __launch_bounds__(M_THREADS) void k_bow_select(
    const uint8_t *__restrict__ q, const uint8_t *__restrict__ t, const int32_t *__restrict__ kf_idx,
    const int32_t *__restrict__ f_idx, const int4 *__restrict__ pairs, int npairs, const uint8_t *__restrict__ valid,
    float nnratio, int th, int32_t *__restrict__ match_f)
{
    // the walk is bow_walk() (orbm_bow_body.h): key-frame features serial, frame features on the lanes
    __shared__ BowStage st;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int w = blockIdx.x * BOW_WAVES + wv;
    if (w >= npairs) return;                 // whole waves leave; nothing below is a block-wide barrier
    const int4 p = pairs[w];                 // key-frame range [x, y) of kf_idx, frame range [z, w) of f_idx
    bow_walk(st, wv, lane, reinterpret_cast<const uint4 *>(q), reinterpret_cast<const uint4 *>(t), kf_idx, f_idx, p, valid, nnratio, th, match_f);
}

// ---- host helpers ----
// rotation histogram + ComputeThreeMaxima cull of SearchByBoW (:236-246, :266-284) on a finished match table
int bow_rotation_cull(const orbx_keypoint *kps_kf, const orbx_keypoint *kps_f, int n_f, int check_orientation,
                      int32_t *match_f, int *nmatches)
{
    RotHist rot;
    int nm = 0;
    for (int i = 0; i < n_f; i++) {
        if (match_f[i] < 0) continue;
        nm++;
        if (check_orientation) MTRY(rot.add(kps_kf[match_f[i]].angle, kps_f[i].angle, i));
    }
    if (check_orientation) rot.cull([&](int i) { match_f[i] = -1; nm--; });
    *nmatches = nm;
    return ORBX_OK;
}

// Returns 1 when the GPU selection does not apply (a node with more than BOW_MAX_NODE_FEATURES frame features, a match table larger
// than the handle's result buffer, ORBM_BOW_HOST_SELECT=1 in the environment): the caller then takes the host-selection path.
static int search_by_bow_device(orbm_matcher *m,
                                const uint8_t *desc_kf, const orbx_keypoint *kps_kf, int n_kf, const uint8_t *valid_kf,
                                const int32_t *fv_kf_node, const int32_t *fv_kf_off, const int32_t *fv_kf_idx, int fv_kf_n,
                                const uint8_t *desc_f, const orbx_keypoint *kps_f, int n_f,
                                const int32_t *fv_f_node, const int32_t *fv_f_off, const int32_t *fv_f_idx, int fv_f_n,
                                float nnratio, int th, int check_orientation, int32_t *match_f, int *nmatches)
{
    static const bool force_host = [] { const char *e = getenv("ORBM_BOW_HOST_SELECT"); return e && e[0] == '1'; }();
    if (force_host) return 1;
    const int nki = fv_kf_off[fv_kf_n], nfi = fv_f_off[fv_f_n];
    if (nki < 0 || nfi < 0) return 1;
    std::vector<int4> pairs;
    for (int a = 0, b = 0; a < fv_kf_n && b < fv_f_n;) {       // merge-join of the ascending node lists (:178-262)
        if (fv_kf_node[a] == fv_f_node[b]) {
            if (fv_f_off[b + 1] - fv_f_off[b] > BOW_MAX_NODE_FEATURES) return 1;
            if (fv_kf_off[a + 1] > fv_kf_off[a] && fv_f_off[b + 1] > fv_f_off[b])
                pairs.push_back(make_int4(fv_kf_off[a], fv_kf_off[a + 1], fv_f_off[b], fv_f_off[b + 1]));
            a++; b++;
        } else if (fv_kf_node[a] < fv_f_node[b]) a++;
        else b++;
    }
    const int np = (int)pairs.size();
    if (np == 0) return ORBX_OK;
    for (int c = 0; c < nki; c++)
        if (fv_kf_idx[c] < 0 || fv_kf_idx[c] >= n_kf) return mfail(ORBX_E_INVALID, "key-frame feature index %d outside [0,%d)", fv_kf_idx[c], n_kf);
    for (int c = 0; c < nfi; c++)
        if (fv_f_idx[c] < 0 || fv_f_idx[c] >= n_f) return mfail(ORBX_E_INVALID, "frame feature index %d outside [0,%d)", fv_f_idx[c], n_f);
    if ((size_t)n_f > m->d_out.count()) return 1;     // the match table lives in d_out
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    MTRY(orbm_arena_begin(m));
    InBlock in(m);                                  // one copy up, one kernel, one copy back
    const int pq = in.add(desc_kf, (size_t)n_kf * 32), pt = in.add(desc_f, (size_t)n_f * 32);
    const int pki = in.add(fv_kf_idx, (size_t)nki * 4), pfi = in.add(fv_f_idx, (size_t)nfi * 4);
    const int pp = in.add(pairs.data(), (size_t)np * 16), pv = in.add(valid_kf, valid_kf ? (size_t)n_kf : 0);
    MTRY(in.upload(s));
    hipLaunchKernelGGL(k_bow_select, dim3((np + M_THREADS / 64 - 1) / (M_THREADS / 64)), dim3(M_THREADS), 0, s,
                       in.at<uint8_t>(pq), in.at<uint8_t>(pt), in.at<int32_t>(pki), in.at<int32_t>(pfi), in.at<int4>(pp), np,
                       in.at<uint8_t>(pv), nnratio, th, m->d_out);
    MHIPCHK(hipGetLastError());
    std::vector<int32_t> out((size_t)n_f);
    MTRY(orbm_d2h(m, out.data(), m->d_out, (size_t)n_f * 4, s));
    MTRY(orbm_sync(m, s));
    for (int k = 0; k < np; k++)         // the kernel wrote the entries of the paired nodes only
        for (int c = pairs[k].z; c < pairs[k].w; c++) match_f[fv_f_idx[c]] = out[fv_f_idx[c]];
    return bow_rotation_cull(kps_kf, kps_f, n_f, check_orientation, match_f, nmatches);
}

// ---- N2: SearchByBoW (src/ORBmatcher.cc:159-288).  Usual path: search_by_bow_device above (selection on the GPU).  The rest
// of this function is the general fallback: every node-mate distance on the GPU, the order-dependent selection on the host ----
static int search_by_bow_impl(orbm_matcher *m,
                              const uint8_t *desc_kf, const orbx_keypoint *kps_kf, int n_kf, const uint8_t *valid_kf,
                              const int32_t *fv_kf_node, const int32_t *fv_kf_off, const int32_t *fv_kf_idx, int fv_kf_n,
                              const uint8_t *desc_f, const orbx_keypoint *kps_f, int n_f,
                              const int32_t *fv_f_node, const int32_t *fv_f_off, const int32_t *fv_f_idx, int fv_f_n,
                              float nnratio, int th, int check_orientation, int32_t *match_f, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n_kf < 0 || n_f < 0 || fv_kf_n < 0 || fv_f_n < 0 || !match_f || !nmatches) return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n_f; i++) match_f[i] = -1;
    if (n_kf == 0 || n_f == 0 || fv_kf_n == 0 || fv_f_n == 0) return ORBX_OK;
    if (!desc_kf || !kps_kf || !desc_f || !kps_f || !fv_kf_node || !fv_kf_off || !fv_kf_idx || !fv_f_node || !fv_f_off || !fv_f_idx)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    MTRY(orbm_grow(m, n_kf, n_f, 0));
    {   // selection on the GPU when every matched node fits a wave's registers
        int rc = search_by_bow_device(m, desc_kf, kps_kf, n_kf, valid_kf, fv_kf_node, fv_kf_off, fv_kf_idx, fv_kf_n, desc_f, kps_f, n_f,
                                      fv_f_node, fv_f_off, fv_f_idx, fv_f_n, nnratio, th, check_orientation, match_f, nmatches);
        if (rc != 1) return rc;    // 1 = not applicable: distances on the GPU, selection on the host (below)
    }
    // merge-join of the two ascending node lists (:178-262); queries = usable key-frame features in visiting order
    struct Q { int kf, f_node; };
    std::vector<Q> qs;
    std::vector<int32_t> off;
    qs.reserve((size_t)n_kf); off.reserve((size_t)n_kf + 1);
    off.push_back(0);
    long long pairs = 0;
    for (int a = 0, b = 0; a < fv_kf_n && b < fv_f_n;) {
        if (fv_kf_node[a] == fv_f_node[b]) {
            const int nb = fv_f_off[b + 1] - fv_f_off[b];
            for (int c = fv_kf_off[a]; c < fv_kf_off[a + 1]; c++) {
                const int ikf = fv_kf_idx[c];
                if (ikf < 0 || ikf >= n_kf) return mfail(ORBX_E_INVALID, "key-frame feature index %d outside [0,%d)", ikf, n_kf);
                if (valid_kf && !valid_kf[ikf]) continue;
                qs.push_back({ikf, b});
                pairs += nb;
                off.push_back((int32_t)pairs);
            }
            a++; b++;
        } else if (fv_kf_node[a] < fv_f_node[b]) a++;   // lower_bound on an ascending list == advance
        else b++;
    }
    const int nq = (int)qs.size();
    if (nq == 0 || pairs == 0) return ORBX_OK;
    MTRY(orbm_grow(m, 0, 0, pairs));                 // the distances come back through d_out
    // Usual case (both frames below 65536 features): the key frame's descriptor block goes up as it is and every pair is
    // (key-frame feature << 16 | frame feature).  Otherwise the query descriptors are compacted and the kernel finds a
    // pair's query by binary search over the offsets.
    const bool packed16 = n_kf < 65536 && n_f < 65536;
    std::vector<uint8_t> qd;
    if (!packed16) {
        qd.resize((size_t)nq * 32);
        for (int i = 0; i < nq; i++) memcpy(&qd[(size_t)i * 32], desc_kf + (size_t)qs[i].kf * 32, 32);
    }
    std::vector<int32_t> idx((size_t)pairs), dist((size_t)pairs);
    for (int i = 0; i < nq; i++) {
        const int b = qs[i].f_node;
        const uint32_t hi = packed16 ? (uint32_t)qs[i].kf << 16 : 0u;
        int32_t *dst = idx.data() + off[i];
        for (int c = fv_f_off[b]; c < fv_f_off[b + 1]; c++) {
            const int fi = fv_f_idx[c];
            if (fi < 0 || fi >= n_f) return mfail(ORBX_E_INVALID, "frame feature index %d outside [0,%d)", fi, n_f);
            *dst++ = (int32_t)(hi | (uint32_t)fi);
        }
    }
    MHIPCHK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    MTRY(orbm_arena_begin(m));
    InBlock in(m);
    const int pq = packed16 ? in.add(desc_kf, (size_t)n_kf * 32) : in.add(qd.data(), qd.size()), pt = in.add(desc_f, (size_t)n_f * 32);
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
            if (match_f[fi] >= 0) continue;                 // :209
            const int d = dist[c];
            if (d < best1) { best2 = best1; best1 = d; bestF = fi; }
            else if (d < best2) best2 = d;
        }
        if (best1 <= th && (float)best1 < nnratio * (float)best2) match_f[bestF] = qs[i].kf;
    }
    return bow_rotation_cull(kps_kf, kps_f, n_f, check_orientation, match_f, nmatches);
}

extern "C" int orbm_search_by_bow(orbm_matcher *m,
                                  const uint8_t *desc_kf, const orbx_keypoint *kps_kf, int n_kf, const uint8_t *valid_kf,
                                  const int32_t *fv_kf_node, const int32_t *fv_kf_off, const int32_t *fv_kf_idx, int fv_kf_n,
                                  const uint8_t *desc_f, const orbx_keypoint *kps_f, int n_f,
                                  const int32_t *fv_f_node, const int32_t *fv_f_off, const int32_t *fv_f_idx, int fv_f_n,
                                  float nnratio, int check_orientation, int32_t *match_f, int *nmatches)
{
    return search_by_bow_impl(m, desc_kf, kps_kf, n_kf, valid_kf, fv_kf_node, fv_kf_off, fv_kf_idx, fv_kf_n, desc_f, kps_f, n_f,
                              fv_f_node, fv_f_off, fv_f_idx, fv_f_n, nnratio, ORBM_TH_LOW, check_orientation, match_f, nmatches);
}

// ---- ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (src/ORBmatcher.cc:522-655) ----
// The same node-by-node scan as the key-frame / frame variant above with three differences: features of BOTH key frames need a
// usable MapPoint (:558-562, :576-580), the acceptance is the strict `bestDist1 < TH_LOW` (:598), and the table is indexed by the
// OUTER key frame's features (vpMatches12[idx1]).  A feature of KF2 that can never be taken (no MapPoint, bad MapPoint) is dropped
// from KF2's node lists before the scan -- skipping it inside the scan is the same thing --, the scan runs with th = TH_LOW - 1,
// and the table it returns (inner feature -> outer feature, one-to-one by vbMatched2) is inverted.
extern "C" int orbm_search_by_bow_kf(orbm_matcher *m,
                                     const uint8_t *desc1, const orbx_keypoint *kps1, int n1, const uint8_t *valid1,
                                     const int32_t *fv1_node, const int32_t *fv1_off, const int32_t *fv1_idx, int fv1_n,
                                     const uint8_t *desc2, const orbx_keypoint *kps2, int n2, const uint8_t *valid2,
                                     const int32_t *fv2_node, const int32_t *fv2_off, const int32_t *fv2_idx, int fv2_n,
                                     float nnratio, int check_orientation, int32_t *matches12, int *nmatches)
{
    if (!m) return mfail(ORBX_E_INVALID, "NULL handle");
    if (n1 < 0 || n2 < 0 || fv1_n < 0 || fv2_n < 0 || !matches12 || !nmatches) return mfail(ORBX_E_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;                             // :534
    if (n1 == 0 || n2 == 0 || fv1_n == 0 || fv2_n == 0) return ORBX_OK;
    if (!fv2_node || !fv2_off || !fv2_idx || !valid1 || !valid2) return mfail(ORBX_E_INVALID, "NULL buffer");
    std::vector<int32_t> off2((size_t)fv2_n + 1, 0), idx2;
    idx2.reserve((size_t)std::max(fv2_off[fv2_n], 0));
    for (int b = 0; b < fv2_n; b++) {
        for (int c = fv2_off[b]; c < fv2_off[b + 1]; c++) {
            const int i2 = fv2_idx[c];
            if (i2 < 0 || i2 >= n2) return mfail(ORBX_E_INVALID, "feature index %d outside [0,%d)", i2, n2);
            if (valid2[i2]) idx2.push_back(i2);
        }
        off2[(size_t)b + 1] = (int32_t)idx2.size();
    }
    if (idx2.empty()) return ORBX_OK;
    std::vector<int32_t> match2((size_t)n2, -1);
    int rc = search_by_bow_impl(m, desc1, kps1, n1, valid1, fv1_node, fv1_off, fv1_idx, fv1_n, desc2, kps2, n2,
                                fv2_node, off2.data(), idx2.data(), fv2_n, nnratio, ORBM_TH_LOW - 1, check_orientation, match2.data(), nmatches);
    if (rc != ORBX_OK) return rc;
    for (int i2 = 0; i2 < n2; i2++)
        if (match2[i2] >= 0) matches12[match2[i2]] = i2;
    return ORBX_OK;
}

extern "C" int orbm_three_maxima(const int32_t *histo, int L, int32_t ind[3])
{
    if (!histo || !ind || L < 0) return mfail(ORBX_E_INVALID, "bad argument");
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = histo[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    ind[0] = ind1; ind[1] = ind2; ind[2] = ind3;
    return ORBX_OK;
}

extern "C" int orbm_rot_filter(const float *angle_q, const float *angle_t, int32_t *match12, int nq)
{
    if (nq < 0 || (nq > 0 && (!angle_q || !angle_t || !match12))) return mfail(ORBX_E_INVALID, "bad argument");
    RotHist rot;
    int nmatches = 0;
    for (int i = 0; i < nq; i++) {
        if (match12[i] < 0) continue;
        MTRY(rot.add(angle_q[i], angle_t[match12[i]], i));
        nmatches++;
    }
    rot.cull([&](int i) { match12[i] = -1; nmatches--; });
    return nmatches;
}
