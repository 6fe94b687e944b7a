// orbm_fuse.hip -- ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:825-975 of
// WChen09/My-SLAM) for ALL target key frames of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:456-536) in one call:
// orbm_fuse_views (include/orbm.h).  Projection -> gates -> window -> selection for every (key frame, MapPoint) slot without
// coming back to the host; what happens to a fused point (:954-970) is object-graph work and is replayed by the caller in the
// reference's order (host/ORBmatcher.h, DESIGN.md section 17: what can and cannot change between two key frames of the loop).
//
// One upload, two launches, one download, one synchronisation:
//   k_grid_build_views   (orbm_grid.hip) one workgroup per view builds the view's grid in the call's own storage (d_fuse); the
//                        two grid slots of the handle are not touched
//   k_fuse_views         launch grid (ceil(n_mp / 64), nviews): the 64 slots of a wave belong to one view, whose block and grid are
//                        read at wave-uniform addresses (scalar loads).
//                        Phase 1, one lane per slot: :852-890 (fuse_project below, on orbm_project.h).
//                        Phase 2, the wave together: for every lane that reached :892 in turn, its u, v, ur, radius, level and
//                        descriptor are broadcast (v_readlane) and the wave walks the window with kf_window_search (orbm_window.h,
//                        k_search_kf's body: octave window, chi-square gate, Hamming distance, packed minimum).
//                        No LDS, no scratch, no atomics.
#include "orbm_window.h"
#include "orbm_project.h"

#define FUSE_THREADS 64

struct FuseViewDev {
    orbm_fuse_view v;           // inv_level_sigma2 past nlevels zeroed, as orbm_fuse's launch does
    OrbmGrid g;                 // the view's slices of d_fuse
    int32_t base;               // the view's first feature in the concatenated arrays
};
struct FuseProj { float u, v, ur; int level; };

// :852-887 for one MapPoint.  ORBM_FUSE_NO_MATCH = the point reached :887 and o is valid; the search decides between that and
// ORBM_FUSE_MATCH.  Operation by operation: invz = 1/z a float division, x = Pc0*invz, u = fx*x+cx (:859-864, not isInFrustum's
// order), KeyFrame::IsInImage as [min, max) (a NaN u or v fails it), the getters' 1.2f / 0.8f, cv::norm and Mat::dot in double,
// 0.5*dist3D a double product.
__host__ __device__ __forceinline__ int fuse_project(const orbm_fuse_view *__restrict__ V, float Px, float Py, float Pz, float Nx, float Ny,
                                                     float Nz, float mf_max, float mf_min, FuseProj &o)
{
    const float PcX = fru_gemm_row(V->Rcw, V->tcw[0], Px, Py, Pz);                      // :853
    const float PcY = fru_gemm_row(V->Rcw + 3, V->tcw[1], Px, Py, Pz);
    const float PcZ = fru_gemm_row(V->Rcw + 6, V->tcw[2], Px, Py, Pz);
    if (PcZ < 0.0f) return ORBM_FUSE_BEHIND;                                            // :856 (+-0 and NaN pass)
    const float invz = PJ_DIV(1.0f, PcZ);                                               // :859
    const float x = PJ_MUL(PcX, invz), y = PJ_MUL(PcY, invz);                           // :860-861
    const float u = PJ_ADD(PJ_MUL(V->fx, x), V->cx);                                    // :863
    const float v = PJ_ADD(PJ_MUL(V->fy, y), V->cy);                                    // :864
    if (!(u >= V->bounds[0] && u < V->bounds[1] && v >= V->bounds[2] && v < V->bounds[3])) return ORBM_FUSE_OUT_IMAGE;   // :867
    const float ur = PJ_SUB(u, PJ_MUL(V->mbf, invz));                                   // :870
    const float max_distance = PJ_MUL(1.2f, mf_max);                                    // src/MapPoint.cc:382
    const float min_distance = PJ_MUL(0.8f, mf_min);                                    // src/MapPoint.cc:376
    const float POx = PJ_SUB(Px, V->Ow[0]), POy = PJ_SUB(Py, V->Ow[1]), POz = PJ_SUB(Pz, V->Ow[2]);   // :874
    const float dist = (float)sqrt(fru_dot3(POx, POy, POz, POx, POy, POz));             // :875
    if (dist < min_distance || dist > max_distance) return ORBM_FUSE_DISTANCE;          // :878
    if (fru_dot3(POx, POy, POz, Nx, Ny, Nz) < 0.5 * (double)dist) return ORBM_FUSE_VIEW_ANGLE;   // :884 (NaN passes)
    int level;
    if (!fru_predict_scale(mf_max, dist, V->log_scale_factor, V->nlevels, level)) return ORBM_FUSE_UNDEFINED;   // :887
    o.u = u; o.v = v; o.ur = ur; o.level = level;
    return ORBM_FUSE_NO_MATCH;
}

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ uint32_t lane_u(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_views(
    const FuseViewDev *__restrict__ views, int n_mp, const uint8_t *__restrict__ skip, const float *__restrict__ xw,
    const float *__restrict__ normal, const float *__restrict__ mf_max, const float *__restrict__ mf_min,
    const uint8_t *__restrict__ mp_desc, const float *__restrict__ u_right, const uint8_t *__restrict__ desc_kf, float th,
    uint8_t *__restrict__ status, int32_t *__restrict__ best_idx, int32_t *__restrict__ best_dist, float *__restrict__ proj_u,
    float *__restrict__ proj_v, float *__restrict__ proj_ur, int32_t *__restrict__ pred_level)
{
    const int lane = threadIdx.x;
    const FuseViewDev *__restrict__ V = views + blockIdx.y;                 // wave-uniform: scalar loads
    const int i = blockIdx.x * FUSE_THREADS + lane;
    const bool live = i < n_mp;                                             // a lane past the end stays: the walk needs the whole wave
    const long long slot = (long long)blockIdx.y * n_mp + i;

    // phase 1: one lane per slot
    int st = ORBM_FUSE_SKIPPED;
    FuseProj o = {0.f, 0.f, 0.f, 0};
    if (live && !skip[slot]) {
        const long long b = 3 * (long long)i;
        st = fuse_project(&V->v, xw[b], xw[b + 1], xw[b + 2], normal[b], normal[b + 1], normal[b + 2], mf_max[i], mf_min[i], o);
    }
    const bool searched = st == ORBM_FUSE_NO_MATCH;
    float r = 0.f;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (searched) {
        r = __fmul_rn(th, V->v.scale_factors[o.level]);                     // :890
        const uint4 *D = reinterpret_cast<const uint4 *>(mp_desc) + 2 * (long long)i;
        d0 = D[0]; d1 = D[1];
    }

    // phase 2: the lanes that reached :892, one after the other, each searched by the whole wave
    const OrbmGrid g = V->g;
    const float *__restrict__ ur_kf = u_right + V->base;
    const uint8_t *__restrict__ dk = desc_kf + 32 * (long long)V->base;
    int my_idx = -1, my_dist = 256;
    unsigned long long todo = __builtin_amdgcn_ballot_w64(searched);
    while (todo) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        const float x = lane_f(o.u, src), y = lane_f(o.v, src), ur = lane_f(o.ur, src), rr = lane_f(r, src);
        const int lv = __builtin_amdgcn_readlane(o.level, src);
        const uint4 q0 = make_uint4(lane_u(d0.x, src), lane_u(d0.y, src), lane_u(d0.z, src), lane_u(d0.w, src));
        const uint4 q1 = make_uint4(lane_u(d1.x, src), lane_u(d1.y, src), lane_u(d1.z, src), lane_u(d1.w, src));
        int bidx;
        const uint32_t bp = kf_window_search(g, x, y, rr, lv, true, ur, ur_kf, [&](int l) { return V->v.inv_level_sigma2[l]; }, q0, q1, dk,
                                             lane, bidx);
        const uint32_t B = wave_min_u32(bp);
        if (B != KF_KEY_NONE) {                                             // positions are unique: one lane holds the winner
            const unsigned long long w = __builtin_amdgcn_ballot_w64(bp == B);
            const int widx = __builtin_amdgcn_readlane(bidx, __builtin_amdgcn_readfirstlane(__ffsll((long long)w) - 1));
            if (lane == src) { my_idx = widx; my_dist = (int)(B >> 22); }
        }
    }
    if (!live) return;
    if (searched && my_dist <= ORBM_TH_LOW) st = ORBM_FUSE_MATCH;           // :952
    status[slot] = (uint8_t)st;
    best_idx[slot] = st == ORBM_FUSE_MATCH ? my_idx : -1;
    best_dist[slot] = my_dist;
    proj_u[slot] = o.u; proj_v[slot] = o.v; proj_ur[slot] = o.ur; pred_level[slot] = o.level;   // zeros unless the slot reached :887
}

extern "C" int orbm_fuse_views(orbm_matcher *m, const orbm_fuse_view *views, int nviews, const int32_t *off, const orbx_keypoint *kps_un,
                               const float *u_right, const uint8_t *desc_kf, int n_mp, const uint8_t *skip, const float *xw,
                               const float *normal, const float *mf_max, const float *mf_min, const uint8_t *mp_desc, float th,
                               uint8_t *status, int32_t *best_idx, int32_t *best_dist, float *proj_u, float *proj_v, float *proj_ur,
                               int32_t *pred_level, int32_t *nfused)
{
    if (nviews < 0 || n_mp < 0) return mfail(ORBX_E_INVALID, "nviews=%d n_mp=%d", nviews, n_mp);
    if (nviews == 0 || n_mp == 0) return ORBX_OK;
    if (nviews > 65535 || (long long)nviews * n_mp > (1ll << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 65535 views / 2^28 (view, MapPoint) slots");
    if (!views || !off || !skip || !xw || !normal || !mf_max || !mf_min || !mp_desc || !status || !best_idx || !best_dist || !proj_u ||
        !proj_v || !proj_ur || !pred_level || !nfused)
        return mfail(ORBX_E_INVALID, "NULL buffer");
    if (off[0] != 0) return mfail(ORBX_E_INVALID, "off[0] must be 0");
    for (int v = 0; v < nviews; v++)
        if (off[v + 1] < off[v]) return mfail(ORBX_E_INVALID, "off not monotone at %d", v);
    const int n_kf = off[nviews];
    if (n_kf > (1 << 28)) return mfail(ORBX_E_CAPACITY, "request beyond 2^28 key-frame features");
    if (n_kf > 0 && (!kps_un || !u_right || !desc_kf)) return mfail(ORBX_E_INVALID, "NULL buffer");
    for (int v = 0; v < nviews; v++) {
        if (views[v].nlevels < 1 || views[v].nlevels > ORBX_MAX_LEVELS) return mfail(ORBX_E_INVALID, "view %d has nlevels=%d", v, views[v].nlevels);
        if (!(views[v].grid.inv_w > 0.f) || !(views[v].grid.inv_h > 0.f)) return mfail(ORBX_E_INVALID, "view %d: grid cell sizes must be positive", v);
    }
    const size_t slots = (size_t)nviews * n_mp;
    bool any = false;
    for (size_t k = 0; k < slots && !any; k++) any = !skip[k];

    // nothing to search: every slot skipped, or not one key-frame feature (every window is empty).  Phase 1 on the host.
    if (!any || n_kf == 0) {
        for (int v = 0; v < nviews; v++) {
            for (int i = 0; i < n_mp; i++) {
                const size_t k = (size_t)v * n_mp + i;
                FuseProj o = {0.f, 0.f, 0.f, 0};
                const float *X = xw + 3 * (size_t)i, *N = normal + 3 * (size_t)i;
                status[k] = (uint8_t)(skip[k] ? ORBM_FUSE_SKIPPED : fuse_project(&views[v], X[0], X[1], X[2], N[0], N[1], N[2], mf_max[i], mf_min[i], o));
                best_idx[k] = -1; best_dist[k] = 256;
                proj_u[k] = o.u; proj_v[k] = o.v; proj_ur[k] = o.ur; pred_level[k] = o.level;
            }
            nfused[v] = 0;
        }
        return ORBX_OK;
    }
    if (!m) return orbm_no_handle();

    MHIPCHK(hipSetDevice(m->device));
    // d_fuse: cell_start of every view, the five feature arrays of the grids, then the dense results (six words and a byte per slot)
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t cells = up((size_t)nviews * (ORBM_GRID_CELLS + 1) * 4), arr = up((size_t)n_kf * 4), word = slots * 4;
    MTRY(orbm_ensure_fuse(m, cells + 5 * arr + 6 * word + slots));
    uint8_t *base = m->d_fuse;
    int32_t *d_cells = (int32_t *)base;
    float *d_kx = (float *)(base + cells), *d_ky = (float *)(base + cells + arr);
    int32_t *d_koct = (int32_t *)(base + cells + 2 * arr), *d_items = (int32_t *)(base + cells + 3 * arr), *d_cell_of = (int32_t *)(base + cells + 4 * arr);
    uint8_t *d_res = base + cells + 5 * arr;

    std::vector<FuseViewDev> dv((size_t)nviews);
    for (int v = 0; v < nviews; v++) {
        FuseViewDev &D = dv[v];
        D.v = views[v];
        for (int l = D.v.nlevels; l < ORBX_MAX_LEVELS; l++) D.v.inv_level_sigma2[l] = 0.f;
        const orbm_kf_grid &kg = views[v].grid;
        const int o = off[v];
        D.g.min_x = kg.assign_min_x; D.g.min_y = kg.assign_min_y; D.g.inv_w = kg.inv_w; D.g.inv_h = kg.inv_h;
        D.g.qmin_x = kg.query_min_x; D.g.qmin_y = kg.query_min_y;
        D.g.n = off[v + 1] - o;
        D.g.kx = d_kx + o; D.g.ky = d_ky + o; D.g.koct = d_koct + o; D.g.items = d_items + o; D.g.cell_of = d_cell_of + o;
        D.g.cell_start = d_cells + (size_t)v * (ORBM_GRID_CELLS + 1);
        D.base = o;
    }
    // the grid builder reads an OrbmGrid per view: the records' grids, packed
    std::vector<OrbmGrid> dg((size_t)nviews);
    for (int v = 0; v < nviews; v++) dg[v] = dv[v].g;

    MTRY(orbm_arena_begin(m));
    hipStream_t s = m->stream;
    InBlock in(m);
    const size_t N = (size_t)n_mp;
    const int pv = in.add(dv.data(), dv.size() * sizeof(FuseViewDev)), pg = in.add(dg.data(), dg.size() * sizeof(OrbmGrid));
    const int po = in.add(off, ((size_t)nviews + 1) * 4), pk = in.add(kps_un, (size_t)n_kf * sizeof(orbx_keypoint));
    const int pu = in.add(u_right, (size_t)n_kf * 4), pd = in.add(desc_kf, (size_t)n_kf * 32), ps = in.add(skip, slots);
    const int px = in.add(xw, N * 12), pn = in.add(normal, N * 12), pa = in.add(mf_max, N * 4), pi = in.add(mf_min, N * 4);
    const int pm = in.add(mp_desc, N * 32);
    MTRY(in.upload(s));
    orbm_grid_build_views_launch(in.at<OrbmGrid>(pg), in.at<int32_t>(po), in.at<orbx_keypoint>(pk), nviews, s);
    MHIPCHK(hipGetLastError());
    int32_t *o_idx = (int32_t *)d_res, *o_dist = (int32_t *)(d_res + word), *o_lvl = (int32_t *)(d_res + 5 * word);
    float *o_u = (float *)(d_res + 2 * word), *o_v = (float *)(d_res + 3 * word), *o_ur = (float *)(d_res + 4 * word);
    uint8_t *o_st = d_res + 6 * word;
    hipLaunchKernelGGL(k_fuse_views, dim3((n_mp + FUSE_THREADS - 1) / FUSE_THREADS, nviews), dim3(FUSE_THREADS), 0, s, in.at<FuseViewDev>(pv), n_mp,
                       in.at<uint8_t>(ps), in.at<float>(px), in.at<float>(pn), in.at<float>(pa), in.at<float>(pi), in.at<uint8_t>(pm),
                       in.at<float>(pu), in.at<uint8_t>(pd), th, o_st, o_idx, o_dist, o_u, o_v, o_ur, o_lvl);
    MHIPCHK(hipGetLastError());
    void *host[7] = {best_idx, best_dist, proj_u, proj_v, proj_ur, pred_level, status};
    const size_t parts[7] = {word, word, word, word, word, word, slots};
    MTRY(orbm_d2h_split(m, host, parts, 7, d_res, s));
    MTRY(orbm_sync(m, s));
    for (int v = 0; v < nviews; v++) {
        int cnt = 0;
        for (int i = 0; i < n_mp; i++) cnt += status[(size_t)v * n_mp + i] == ORBM_FUSE_MATCH;
        nfused[v] = cnt;
    }
    return ORBX_OK;
}
