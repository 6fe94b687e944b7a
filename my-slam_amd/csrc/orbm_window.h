// orbm_window.h -- Frame / KeyFrame::GetFeaturesInArea for one wave (src/Frame.cc:327-380, src/KeyFrame.cc:569-606 of WChen09/My-SLAM):
// the cell range of a window, the membership test and the walk over the members in the reference's candidate order.  Used by
// k_area_list and k_search_area (orbm_grid.hip) and k_search_kf (orbm_kf.hip); "first candidate wins a tie" rests on this order, so
// it exists once.  The window maths is fp32 exactly as written in the reference (no contraction: __f*_rn).
#pragma once
#include "orbm_internal.h"
#include "orbx_internal.h"

// cell range of a window, src/Frame.cc:332-346.  Returns false when the window misses the grid.
__device__ __forceinline__ bool window_cells(const OrbmGrid &g, float x, float y, float r,
                                             int &cx0, int &cx1, int &cy0, int &cy1)
{
    cx0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, g.qmin_x), r), g.inv_w)));
    if (cx0 >= ORBM_GRID_COLS) return false;
    cx1 = min(ORBM_GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, g.qmin_x), r), g.inv_w)));
    if (cx1 < 0) return false;
    cy0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, g.qmin_y), r), g.inv_h)));
    if (cy0 >= ORBM_GRID_ROWS) return false;
    cy1 = min(ORBM_GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, g.qmin_y), r), g.inv_h)));
    if (cy1 < 0) return false;
    return true;
}

__device__ __forceinline__ bool in_window(const OrbmGrid &g, int i, float x, float y, float r, int minl, int maxl)
{
    if ((minl > 0) || (maxl >= 0)) {                       // bCheckLevels :348
        const int oct = g.koct[i];
        if (oct < minl) return false;
        if (maxl >= 0 && oct > maxl) return false;
    }
    return fabsf(__fsub_rn(g.kx[i], x)) < r && fabsf(__fsub_rn(g.ky[i], y)) < r;   // :368-372
}

// One wave walks the window (x, y, r) of grid g in the reference's order: cell column by cell column (a column's cells cy0 .. cy1 are
// one contiguous item range), 64 items per round.  member(i) decides whether keypoint i is a candidate of this search; members are
// what the ballot and the running position count.  visit(i, position) runs in the lane that holds member i; position is its index
// in the candidate list the reference would build (vIndices).  Returns the number of members; every lane of the wave must call it.
template <class Member, class Visit>
__device__ __forceinline__ int window_walk(const OrbmGrid &g, float x, float y, float r, int lane, Member member, Visit visit)
{
    int n = 0, cx0, cx1, cy0, cy1;
    if (!window_cells(g, x, y, r, cx0, cx1, cy0, cy1)) return 0;
    for (int ix = cx0; ix <= cx1; ix++) {
        const int s = g.cell_start[ix * ORBM_GRID_ROWS + cy0], e = g.cell_start[ix * ORBM_GRID_ROWS + cy1 + 1];
        for (int j0 = s; j0 < e; j0 += 64) {
            const int j = j0 + lane;
            int i = -1;
            bool ok = false;
            if (j < e) { i = g.items[j]; ok = member(i); }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
            if (ok) visit(i, orbx_prefix_cnt(m, n));
            n += __popcll(m);
        }
    }
    return n;
}

#define KF_KEY_NONE 0xFFFFFFFFu
// The stateless key-frame search of one window by one wave (k_search_kf in orbm_kf.hip, k_fuse_views in orbm_fuse.hip): KeyFrame::
// GetFeaturesInArea(x, y, r) in the reference's order, the octave window [lv - 1, lv] (src/ORBmatcher.cc:380, :911, :1067, :1207),
// with `gated` Fuse's chi-square gate (:914-938; ur = the query's u - bf*invz, t_uright = mvuRight, inv_sigma2(octave) =
// mvInvLevelSigma2 with the octave clamped into [0, ORBX_MAX_LEVELS)), then the Hamming distance.  The window itself has no level test
// (src/KeyFrame.cc:569-606): positions count every window member, as vIndices does, and the octave window and the gate drop candidates
// afterwards.  Returns this lane's smallest key = distance << 22 | position (KF_KEY_NONE: none) and its feature in bidx; the wave's
// minimum over the keys is the reference's strict '<' scan: the first candidate wins a tie.  Every lane of the wave must call it.
template <class InvSigma2>
__device__ __forceinline__ uint32_t kf_window_search(const OrbmGrid &g, float x, float y, float r, int lv, bool gated, float ur,
                                                     const float *__restrict__ t_uright, InvSigma2 inv_sigma2, const uint4 &q0,
                                                     const uint4 &q1, const uint8_t *__restrict__ tdesc, int lane, int &bidx)
{
    uint32_t bp = KF_KEY_NONE;
    bidx = -1;
    window_walk(g, x, y, r, lane, [&](int i) { return in_window(g, i, x, y, r, -1, -1); },
                [&](int i, int pos) {
                    const int oct = g.koct[i];
                    bool use = !(oct < lv - 1 || oct > lv);
                    if (use && gated) {
                        const float ex = __fsub_rn(x, g.kx[i]), ey = __fsub_rn(y, g.ky[i]);
                        const float kr = t_uright[i];
                        const float inv = inv_sigma2(min(max(oct, 0), ORBX_MAX_LEVELS - 1));
                        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                        if (kr >= 0) {
                            const float er = __fsub_rn(ur, kr);
                            e2 = __fadd_rn(e2, __fmul_rn(er, er));
                            use = !((double)__fmul_rn(e2, inv) > 7.8);          // :925
                        } else {
                            use = !((double)__fmul_rn(e2, inv) > 5.99);         // :936
                        }
                    }
                    if (use) {
                        const uint4 *Tj = reinterpret_cast<const uint4 *>(tdesc) + 2 * (long long)i;
                        const int d = hamming256(q0, q1, Tj[0], Tj[1]);
                        const uint32_t p = ((uint32_t)d << 22) | (uint32_t)min(pos, 0x3FFFFF);
                        if (p < bp) { bp = p; bidx = i; }
                    }
                });
    return bp;
}
