// orbx_plan.h -- the extractor's shape planner (orbx_plan.cc): host arithmetic only.  It makes no HIP call and never sees a handle;
// orbx_capi.hip plans a shape into a ShapePlan, uploads its tables and only then commits it to the handle.
#pragma once
#include <string>
#include <vector>

#include "orbx_internal.h"

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// several pyramid levels per launch (k_resize_fused): one plan per band height (16 rows for batches, 8 for a few frames)
struct FusePlan { bool ok = false; int a = 0, b = 0, nbands = 0, buf0 = 0, lds = 0, bh = 0; size_t off = 0; };
// upper pyramid levels in one launch, one wave per 2-D tile (k_resize_tiles): levels a + 1 .. nlevels - 1
struct TilePlan { bool ok = false; int a = 0, b = 0, ntx = 0, nty = 0, lds = 0; int lds_off[ORBX_FUSE_MAX] = {}, tab_off[ORBX_FUSE_MAX] = {}; size_t offx = 0, offy = 0; };

// what planning depends on: the constructor's arguments and tables, the A/B switches, the capacities of the handle's table buffers
struct PlanParams {
    int nfeatures = 0; float scale_factor = 0; int nlevels = 0, ini_th = 0, min_th = 0;
    int blur_mode = 0;
    int oct_fast = 1, fuse_on = 1;
    int tile_a = 0, tile_w = 32, tile_h = 32, tile_min_frames = 8;   // off by default: measured slower than the launches it replaces
    size_t bands_cap = 0, tiles_cap = 0, tab_elems = 0; int cells_cap = 0;
    float scale[ORBX_MAX_LEVELS], inv_scale[ORBX_MAX_LEVELS], sigma2[ORBX_MAX_LEVELS], inv_sigma2[ORBX_MAX_LEVELS];
    int quota[ORBX_MAX_LEVELS];
    int umax[16]; int gauss_k[7];
};

// everything one frame shape needs.  Device addresses (lv[l].base of levels >= 1, cell_tab, the ResizeTab pointers) are not the
// planner's to know: the handle fills them in when it commits the plan.
struct ShapePlan {
    OrbxPlan plan;                                          // offsets and capacities are those of the handle's maximum plan
    int resize_mode[ORBX_MAX_LEVELS] = {};                  // RESIZE_* of the step into level l
    std::vector<int> tab_i; std::vector<short2> tab_s;      // xofs | yofs and alpha | beta of levels 1 .. L-1, back to back
    size_t xofs_at[ORBX_MAX_LEVELS] = {}, yofs_at[ORBX_MAX_LEVELS] = {}, tab_used = 0;
    std::vector<uint32_t> cells;                            // [plan.ncells] level | cell row << 4 | cell column << 16
    FusePlan fuse[2]; std::vector<int4> bands;
    TilePlan tile; std::vector<int4> tiles;
};

void orbx_build_tables(PlanParams *pp);                                                    // A1, once per handle
int orbx_make_plan(const PlanParams &pp, int W, int H, OrbxPlan *P, std::string *why);    // the handle's maximum plan
// plan a W x H frame against the maximum plan M; ORBX_OK, or a status and *why (nothing of *S is to be used then)
int orbx_plan_shape(const PlanParams &pp, const OrbxPlan &M, int W, int H, ShapePlan *S, std::string *why);
