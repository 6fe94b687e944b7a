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
