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
