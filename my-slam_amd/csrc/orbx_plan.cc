// orbx_plan.cc -- shape planning of the extractor: constructor tables, level sizes, cv::resize tables, the FAST cell table, the band and
// tile plans of the fused pyramid kernels.  Host arithmetic that restates the reference constructor and OpenCV's resize planning
// (citations: src/ORBextractor.cc of WChen09/My-SLAM); no kernel, no HIP call, no handle (orbx_plan.h).
#include <cfloat>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "orbx_plan.h"

static inline int cv_round(double v) { return (int)lrint(v); }   // cvRound: half to even
static inline int cv_floor(double v) { int i = (int)v; return i - (v < i); }
static inline int cv_ceil(double v) { int i = (int)v; return i + (v > i); }
// read once per process
static bool resize6_on() { static const bool on = [] { const char *e = getenv("ORBX_RESIZE6"); return !e || atoi(e) != 0; }(); return on; }   // A/B switch

// ---- A1: ORBextractor::ORBextractor tables (:412-472) ----
void orbx_build_tables(PlanParams *pp)
{
    const int L = pp->nlevels;
    pp->scale[0] = 1.0f; pp->sigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) {
        pp->scale[i] = pp->scale[i - 1] * pp->scale_factor;
        pp->sigma2[i] = pp->scale[i] * pp->scale[i];
    }
    for (int i = 0; i < L; i++) {
        pp->inv_scale[i] = 1.0f / pp->scale[i];
        pp->inv_sigma2[i] = 1.0f / pp->sigma2[i];
    }
    float factor = 1.0f / pp->scale_factor;
    float nDesired = pp->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int level = 0; level < L - 1; level++) {
        pp->quota[level] = cv_round(nDesired);
        sum += pp->quota[level];
        nDesired *= factor;
    }
    pp->quota[L - 1] = std::max(pp->nfeatures - sum, 0);

    int v, v0, vmax = cv_floor(ORBX_HALF_PATCH * sqrtf(2.f) / 2 + 1);
    int vmin = cv_ceil(ORBX_HALF_PATCH * sqrtf(2.f) / 2);
    const double hp2 = ORBX_HALF_PATCH * ORBX_HALF_PATCH;
    for (v = 0; v <= vmax; ++v) pp->umax[v] = cv_round(sqrt(hp2 - v * v));
    for (v = ORBX_HALF_PATCH, v0 = 0; v >= vmin; --v) {
        while (pp->umax[v0] == pp->umax[v0 + 1]) ++v0;
        pp->umax[v] = v0;
        ++v0;
    }
    // OpenCV getGaussianKernel(7, 2, CV_32F) -> x256 fixed point (cv::GaussianBlur u8 path)
    float cf[7]; double s = 0;
    for (int i = 0; i < 7; i++) { double x = i - 3.0; cf[i] = (float)exp(-0.5 / 4.0 * x * x); s += cf[i]; }
    s = 1. / s;
    for (int i = 0; i < 7; i++) { cf[i] = (float)(cf[i] * s); pp->gauss_k[i] = cv_round((double)cf[i] * 256.0); }
}

// ---- shape planning: level sizes (:1113-1114), cell grid (:775-789), quadtree roots (:545-547) ----
int orbx_make_plan(const PlanParams &pp, int W, int H, OrbxPlan *P, std::string *why)
{
    memset(P, 0, sizeof(*P));
    P->nlevels = pp.nlevels; P->ini_th = pp.ini_th; P->min_th = pp.min_th; P->blur_mode = pp.blur_mode;
    long long cand_off = 0, list_off = 0, arena_off = 0;
    int cells = 0;
    for (int l = 0; l < pp.nlevels; l++) {
        OrbxLevel &L = P->lv[l];
        L.w = cv_round((float)W * pp.inv_scale[l]);
        L.h = cv_round((float)H * pp.inv_scale[l]);
        if (L.w < 1 || L.h < 1 || L.w > 65535 || L.h > 65535) { *why = "level size out of range"; return ORBX_E_SHAPE; }
        L.maxBX = L.w - ORBX_MINB; L.maxBY = L.h - ORBX_MINB;
        const float width = (float)(L.maxBX - ORBX_MINB), height = (float)(L.maxBY - ORBX_MINB);
        L.nCols = width > 0 ? (int)(width / 30.f) : 0;
        L.nRows = height > 0 ? (int)(height / 30.f) : 0;
        if (L.nCols <= 0 || L.nRows <= 0) { L.nCols = L.nRows = 0; L.wCell = L.hCell = 1; }   // no cell => no keypoint
        else { L.wCell = (int)ceilf(width / L.nCols); L.hCell = (int)ceilf(height / L.nRows); }
        L.rcpW = L.wCell > 1 ? (uint32_t)((1ull << 32) / (unsigned)L.wCell + 1) : 0u;
        L.rcpH = L.hCell > 1 ? (uint32_t)((1ull << 32) / (unsigned)L.hCell + 1) : 0u;
        L.cell_begin = cells;
        cells += L.nCols * L.nRows;
        L.quota = pp.quota[l];
        L.nIni = 0; L.hX = 1.f;
        if (L.nCols > 0) {
            L.nIni = (int)roundf(width / (float)(L.maxBY - ORBX_MINB));
            if (L.nIni <= 0) { *why = "portrait level (quadtree root count 0): undefined in the reference"; return ORBX_E_SHAPE; }
            L.hX = width / L.nIni;
        }
        // Candidate capacity = the most NMS survivors a level can have, so that no image overflows it (the reference has no
        // such limit): survivors are strict 8-neighbour maxima inside a cell's zone (cv::FAST nonmax, per cell :811-817), no
        // two of them are adjacent, so a zw x zh zone holds at most ceil(zw/2) * ceil(zh/2); the zones of a level's cells tile
        // [19, w-19) x [19, h-19), hence sum <= ceil((w-38+nCols)/2) * ceil((h-38+nRows)/2) (monotone in w and h, so a
        // smaller frame always fits the workspace planned for the handle's maximum).  The quadtree packs a candidate index
        // into 20 bits: only a level beyond ~4.1 M pixels can still report ORBX_E_CAND_OVERFLOW.
        const long long zw_all = std::max(L.w - 2 * ORBX_EDGE, 0), zh_all = std::max(L.h - 2 * ORBX_EDGE, 0);
        const long long zone = zw_all * zh_all;
        const long long nmax = ((zw_all + L.nCols + 1) / 2) * ((zh_all + L.nRows + 1) / 2);
        L.cand_cap = L.nCols > 0 ? (int)std::min<long long>(nmax + 64, (1 << 20) - 1) : 0;
        if (L.nCols > 0 && zone / 8 + 256 >= 100000) P->oct_big = 1;   // 1080p-class level: the quadtree runs 1024-thread workgroups
        // quadtree fast-forward depth (k_octree): 4 levels of the tree from one key histogram, 5 for 1080p-class levels; fewer when
        // many roots (a wide level) would make the tables large.  ORBX_OCT_FAST=0 turns it off (A/B measurements).
        L.fastD = 0;
        if (L.nCols > 0 && pp.oct_fast) {
            int d = (zone / 8 + 256 >= 100000) ? 5 : 4;
            while (d > 0 && (long long)L.nIni * (((1ll << (2 * (d + 1))) - 1) / 3) > 2800) d--;
            L.fastD = d;
            P->oct_ft = std::max(P->oct_ft, (int)(L.nIni * (((1ll << (2 * (d + 1))) - 1) / 3)));
            // per-coordinate path tables of the fast-forward (k_octree): one u16 per column and per row of the level's box
            if (d > 0) P->oct_map = std::max(P->oct_map, (int)align_up((size_t)std::max(L.maxBX - ORBX_MINB, 1), 8) + (int)align_up((size_t)std::max(L.maxBY - ORBX_MINB, 1), 8));
        }
        L.cand_off = cand_off; cand_off += (L.cand_cap + 15) / 16 * 16;
        L.list_cap = L.nCols > 0 ? (std::max(L.quota + 3, 4 * L.nIni) + 1 + 3) / 4 * 4 : 0;
        L.list_off = list_off; list_off += L.list_cap;
        L.arena_cap = L.nCols > 0 ? 24 * L.list_cap + 256 : 0;
        L.arena_off = arena_off; arena_off += L.arena_cap;
        L.scale = pp.scale[l];
        L.kp_size = (float)(int)(31 * pp.scale[l]);   // :839,:848
    }
    P->ncells = cells;
    P->cand_frame = cand_off; P->list_frame = list_off; P->arena_frame = arena_off;
    P->out_cap = (int)list_off;
    return ORBX_OK;
}

// cv::resize INTER_LINEAR planning for one level pair (OpenCV 3.1.0 imgwarp.cpp)
static void plan_resize(int sw, int sh, int dw, int dh, int *xofs, short2 *alpha, int *yofs, short2 *beta, int *mode)
{
    const double inv_x = (double)dw / sw, inv_y = (double)dh / sh;
    const double scale_x = 1. / inv_x, scale_y = 1. / inv_y;
    const int isx = cv_round(scale_x), isy = cv_round(scale_y);
    const bool area2 = fabs(scale_x - isx) < DBL_EPSILON && fabs(scale_y - isy) < DBL_EPSILON && isx == 2 && isy == 2;
    auto sat = [](float v) { int i = cv_round(v); return (short)(i < -32768 ? -32768 : i > 32767 ? 32767 : i); };
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        xofs[dx] = sx;
        alpha[dx] = make_short2(sat((1.f - fx) * 2048), sat(fx * 2048));
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        yofs[dy] = sy;
        beta[dy] = make_short2(sat((1.f - fy) * 2048), sat(fy * 2048));
    }
    // the 4x4 kernel moves 8 source bytes per 4 destination columns: needs xofs[x+3]+1 - xofs[x] <= 7
    int span = 0;
    for (int dx = 0; dx + 3 < dw; dx += 4) span = std::max(span, xofs[dx + 3] + 1 - xofs[dx]);
    *mode = area2 ? RESIZE_AREA2 : (span <= 7 && sw >= 12 ? RESIZE_FAST : RESIZE_GENERIC);
    // the shared-row kernel (k_resize_linear_4x4s / k_resize_tiles): rows y4 .. y4+3 of every block of four destination rows
    // start r or r + 1 source rows below the block's first one (true for scale factors up to 4/3) and nothing reflects at the top
    if (*mode == RESIZE_FAST) {
        bool six = resize6_on() && sh >= 2;
        for (int y4 = 0; y4 < dh && six; y4++) {                 // any first row: k_resize_tiles starts its blocks where a tile's region starts
            six = yofs[y4] >= 0;
            for (int r = 1; r < 4 && y4 + r < dh; r++) { const int o = yofs[y4 + r] - yofs[y4]; six = six && (o == r || o == r + 1); }
        }
        for (int dx = 0; dx + 3 < dw && six; dx++) six = xofs[dx + 3] + 1 - xofs[dx] <= 7;     // and any first column (the 8-byte window)
        if (six) *mode = RESIZE_FAST6;
    }
}

// One axis of the tile plan of k_resize_tiles.  n[l] = extent of level l, ofs[l] = level l's source-offset table (level-l coordinate ->
// level l-1 coordinate, monotone), T = tile extent at level b.  out[i * (b - a + 1) + (l - a)] = (own0, own1, comp0, comp1) of tile i at
// level l: the owned ranges of a level are cut at the images of the level-b tile boundaries , so they partition the level; the computed range is the hull of the owned range
// and the bilinear footprint of what the tile computes one level down, lengthened to a multiple of 4 (the kernel works in 4x4 blocks
// counted from the range's first pixel).  align_own (the x axis): the computed range starts a multiple of 4 before the owned one, so
// that a block is owned from its first column on or not at all (the range may then start at -1 .. -3: the kernel's table slices repeat column 0).
static int plan_tile_axis(int a, int b, int T, const int *n, const int *const *ofs, bool align_own, std::vector<int4> &out, int *max_comp)
{
    const int nt = (n[b] + T - 1) / T, nl = b - a + 1;
    T = std::min(T, (((n[b] + nt - 1) / nt) + 3) & ~3);       // equal tiles: the kernel ends with its largest tile, and a sliver of a tile carries a full halo
    out.assign((size_t)nt * nl, make_int4(0, 0, 0, 0));
    std::vector<std::vector<int>> B((size_t)nl, std::vector<int>((size_t)nt + 1, 0));
    for (int i = 0; i <= nt; i++) B[(size_t)(b - a)][(size_t)i] = std::min(i * T, n[b]);
    for (int l = b - 1; l >= a; l--)
        for (int i = 0; i <= nt; i++) {
            int v = 0;
            if (i == nt) v = n[l];
            else if (i > 0) {
                const int d = B[(size_t)(l + 1 - a)][(size_t)i];
                if (d >= n[l + 1]) v = n[l];
                else v = std::min(std::max(ofs[l + 1][d], 0), n[l] - 1);
                v = std::max(v, B[(size_t)(l - a)][(size_t)i - 1]);
            }
            B[(size_t)(l - a)][(size_t)i] = v;
        }
    for (int l = a; l <= b; l++) max_comp[l] = 0;
    for (int i = 0; i < nt; i++) {
        int c0 = B[(size_t)(b - a)][(size_t)i], c1 = c0 + ((B[(size_t)(b - a)][(size_t)i + 1] - c0 + 3) & ~3);
        out[(size_t)i * nl + (size_t)(b - a)] = make_int4(B[(size_t)(b - a)][(size_t)i], B[(size_t)(b - a)][(size_t)i + 1], c0, c1);
        max_comp[b] = std::max(max_comp[b], c1 - c0);
        for (int l = b - 1; l >= a; l--) {
            const int v1 = std::min(c1, n[l + 1]);                     // valid coordinates of the computed range one level down
            if (v1 <= c0) return -1;
            const int need0 = std::min(std::max(ofs[l + 1][std::max(c0, 0)], 0), n[l] - 1);
            const int need1 = std::min(std::max(ofs[l + 1][v1 - 1], 0) + 1, n[l] - 1) + 1;
            const int o0 = B[(size_t)(l - a)][(size_t)i], o1 = B[(size_t)(l - a)][(size_t)i + 1];
            c0 = o0 < o1 ? std::min(o0, need0) : need0;
            if (align_own && o0 < o1) c0 = o0 - ((o0 - c0 + 3) & ~3);                // the owned part starts on a block boundary (c0 may be -1 .. -3)
            c1 = c0 + (((o0 < o1 ? std::max(o1, need1) : need1) - c0 + 3) & ~3);     // whole 4x4 blocks from the range's first pixel on
            out[(size_t)i * nl + (size_t)(l - a)] = make_int4(o0, o1, c0, c1);
            max_comp[l] = std::max(max_comp[l], c1 - c0);
        }
    }
    return nt;
}

// ---- fused upper levels: row-band ownership / footprint tables (k_resize_fused) ----
static void plan_bands(const PlanParams &pp, ShapePlan *S)
{
    const OrbxPlan &P = S->plan;
    const std::vector<int> &ti = S->tab_i;
    std::vector<int4> &bands = S->bands;
    for (int v = 0; v < 2; v++) {
        FusePlan &F = S->fuse[v];
        F.bh = v == 0 ? 16 : 8;
        const int b = pp.nlevels - 1;
        for (int a = 1; pp.fuse_on && b - a >= 2 && b < ORBX_FUSE_MAX; a++) {
            bool fast = true;
            for (int l = a + 1; l <= b; l++) fast = fast && resize_is_fast(S->resize_mode[l]) && (P.lv[l].w + 3) / 4 <= 512;
            if (!fast) continue;
            const int nl = b - a + 1, nb = (P.lv[b].h + F.bh - 1) / F.bh;
            std::vector<int4> t((size_t)nb * nl);
            int need_rows[ORBX_MAX_LEVELS] = {};
            for (int j = 0; j < nb; j++) {
                int o0 = j * F.bh, o1 = std::min((j + 1) * F.bh, P.lv[b].h), n0 = o0, n1 = o1;
                t[(size_t)j * nl + (b - a)] = make_int4(o0, o1, n0, n1);
                need_rows[b] = std::max(need_rows[b], n1 - n0);
                for (int l = b - 1; l >= a; l--) {
                    const int *yo = &ti[S->yofs_at[l + 1]];
                    const int hl = P.lv[l].h, hu = P.lv[l + 1].h;
                    auto cl = [&](int v2) { return std::min(std::max(v2, 0), hl - 1); };
                    const int p0 = o0 == 0 ? 0 : cl(yo[o0]), p1 = o1 == hu ? hl : cl(yo[o1]);
                    const int q0 = std::min(cl(yo[n0]), p0), q1 = std::max(cl(yo[n1 - 1] + 1) + 1, p1);
                    o0 = p0; o1 = p1; n0 = q0; n1 = q1;
                    t[(size_t)j * nl + (l - a)] = make_int4(o0, o1, n0, n1);
                    need_rows[l] = std::max(need_rows[l], n1 - n0);
                }
            }
            int buf[2] = {0, 0};
            for (int l = a + 1; l < b; l++) {
                const int pitch = (int)align_up((size_t)P.lv[l].w + 12, 16);
                buf[(l - a) & 1] = std::max(buf[(l - a) & 1], need_rows[l] * pitch);
            }
            int ysum = 0;
            for (int l = a + 1; l <= b; l++) ysum += need_rows[l];
            if (buf[0] + buf[1] > 64 * 1024 || ysum > ORBX_FUSE_YTAB) continue;      // too much for LDS from this level on: start the fusion one level up
            if (bands.size() + t.size() > pp.bands_cap) break;
            F.ok = true; F.a = a; F.b = b; F.nbands = nb; F.buf0 = (int)align_up((size_t)buf[0], 16); F.lds = F.buf0 + (int)align_up((size_t)buf[1], 16) + 16;
            F.off = bands.size();
            bands.insert(bands.end(), t.begin(), t.end());
            break;
        }
    }
}

// ---- fused upper levels, one wave per 2-D tile (k_resize_tiles) ----
static void plan_tiles(const PlanParams &pp, ShapePlan *S)
{
    const OrbxPlan &P = S->plan;
    const std::vector<int> &ti = S->tab_i;
    std::vector<int4> &tiles = S->tiles;
    TilePlan &T = S->tile;
    const int b = pp.nlevels - 1, a = pp.tile_a;
    bool ok = a >= 1 && b - a >= 2 && b < ORBX_FUSE_MAX;
    for (int l = a + 1; l <= b && ok; l++) ok = S->resize_mode[l] == RESIZE_FAST6;
    if (!ok) return;
    int nw[ORBX_MAX_LEVELS], nh[ORBX_MAX_LEVELS], mcx[ORBX_MAX_LEVELS], mcy[ORBX_MAX_LEVELS];
    const int *ox[ORBX_MAX_LEVELS] = {}, *oy[ORBX_MAX_LEVELS] = {};
    for (int l = a; l <= b; l++) { nw[l] = P.lv[l].w; nh[l] = P.lv[l].h; if (l > a) { ox[l] = &ti[S->xofs_at[l]]; oy[l] = &ti[S->yofs_at[l]]; } }
    std::vector<int4> tx, ty;
    const int ntx = plan_tile_axis(a, b, pp.tile_w, nw, ox, true, tx, mcx), nty = plan_tile_axis(a, b, pp.tile_h, nh, oy, false, ty, mcy);
    ok = ntx >= 1 && nty >= 1 && ntx <= 64 && ntx * nty < 4096 && tx.size() + ty.size() <= pp.tiles_cap;
    int off = 0;
    for (int l = a + 1; l <= b && ok; l++) {                             // every fused level has its own region in the wave's LDS
        ok = mcx[l] / 4 <= 64 && (mcx[l] / 4) * mcy[l] < 4096;           // the lane -> block / lane -> dword division table of the kernel
        T.lds_off[l] = off;
        off += (int)align_up((size_t)mcy[l] * mcx[l] + ORBX_TILE_SLACK, 16);
    }
    for (int l = a + 1; l <= b && ok; l++) { T.tab_off[l] = off; off += 8 * (mcx[l] + mcy[l]); }    // the tile's table slices (mcx, mcy: multiples of 4)
    if (ok && off <= 60 * 1024) {
        T.ok = true; T.a = a; T.b = b; T.ntx = ntx; T.nty = nty; T.lds = off;
        T.offx = 0; T.offy = tx.size();
        tiles = tx; tiles.insert(tiles.end(), ty.begin(), ty.end());
    }
}

// Plan a W x H frame against the handle's maximum plan M; the handle's buffers stay those sized at create, so every check that a
// shape fits them is made here, before anything is uploaded.
int orbx_plan_shape(const PlanParams &pp, const OrbxPlan &M, int W, int H, ShapePlan *S, std::string *why)
{
    *S = ShapePlan();
    OrbxPlan &P = S->plan;
    const int rc = orbx_make_plan(pp, W, H, &P, why);
    if (rc != ORBX_OK) return rc;
    // keep the allocation layout of the max plan (offsets/capacities) so every shape fits
    for (int l = 0; l < pp.nlevels; l++) {
        OrbxLevel &L = P.lv[l];
        const OrbxLevel &X = M.lv[l];
        if (L.cand_cap > X.cand_cap || L.list_cap > X.list_cap || L.arena_cap > X.arena_cap || L.w > X.w || L.h > X.h)
            { *why = "level " + std::to_string(l) + " does not fit the workspace planned for the handle's maximum shape"; return ORBX_E_SHAPE; }
        L.cand_off = X.cand_off; L.list_off = X.list_off; L.arena_off = X.arena_off;
        if (L.nCols > 0) { L.cand_cap = X.cand_cap; L.arena_cap = X.arena_cap; }
    }
    P.cand_frame = M.cand_frame; P.list_frame = M.list_frame; P.arena_frame = M.arena_frame; P.out_cap = M.out_cap;

    std::vector<int> &ti = S->tab_i;
    std::vector<short2> &ts = S->tab_s;
    ti.assign(pp.tab_elems ? pp.tab_elems : 1, 0);
    ts.assign(ti.size(), make_short2(0, 0));
    size_t e = 0;
    for (int l = 1; l < pp.nlevels; l++) {
        OrbxLevel &L = P.lv[l];
        L.stride = (int)align_up(L.w, 64);
        L.frame_stride = (long long)align_up((size_t)L.stride * L.h, 256);
        const OrbxLevel &Src = P.lv[l - 1];
        const size_t ex = align_up((size_t)L.w + 4, 4), ey = align_up((size_t)L.h + 4, 4);
        if (e + ex + ey > ti.size()) { *why = "resize tables larger than those planned for the handle's maximum shape"; return ORBX_E_SHAPE; }
        plan_resize(Src.w, Src.h, L.w, L.h, &ti[e], &ts[e], &ti[e + ex], &ts[e + ex], &S->resize_mode[l]);
        for (size_t dy = (size_t)L.h; dy < ey; dy++) { ti[e + ex + dy] = ti[e + ex + L.h - 1]; ts[e + ex + dy] = ts[e + ex + L.h - 1]; }   // k_resize_linear_4x4 reads rows in fours
        S->xofs_at[l] = e; S->yofs_at[l] = e + ex;
        e += ex + ey;
    }
    S->tab_used = e;
    if (P.ncells > pp.cells_cap) { *why = "more FAST cells than the workspace planned for the handle's maximum shape"; return ORBX_E_SHAPE; }
    std::vector<uint32_t> &cells = S->cells;
    cells.assign((size_t)std::max(P.ncells, 1), 0u);
    for (int l = 0; l < pp.nlevels; l++) {
        const OrbxLevel &L = P.lv[l];
        if (L.nRows >= 4096 || L.nCols >= 4096) { *why = "level " + std::to_string(l) + " has too many FAST cells"; return ORBX_E_SHAPE; }
        for (int i = 0; i < L.nRows; i++)
            for (int j = 0; j < L.nCols; j++) cells[(size_t)L.cell_begin + (size_t)i * L.nCols + j] = (uint32_t)l | ((uint32_t)i << 4) | ((uint32_t)j << 16);
    }
    plan_bands(pp, S);
    plan_tiles(pp, S);
    return ORBX_OK;
}
