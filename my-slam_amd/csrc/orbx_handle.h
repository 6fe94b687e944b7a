// orbx_handle.h -- host-only: the extractor handle, shared by its life and lazy resources (orbx_workspace.cc, host compiler) and the
// per-call path and C ABI (orbx_capi.hip).  Every block, stream, event and graph has an owning member (dev_buf.h); what kernels take
// (OrbxWork, the plan's addresses, the output pointers) are views into those, filled in one place each.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

#include "dev_buf.h"
#include "orbx_plan.h"
#include "stage_pool.h"

int xfail(int code, const char *fmt, ...);          // sets orbx_last_error()'s text (thread-local) and returns code
#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return xfail(ORBX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define XTRY(expr)                            \
    do {                                      \
        int xtry_ = (expr);                   \
        if (xtry_ != ORBX_OK) return xtry_;   \
    } while (0)

#define ORBX_MAX_SUB 4
struct OrbxRingSlot { DevEvent e[5]; };             // the stage events of one call under profiling mode 2
struct OrbxChunkEvents { DevEvent up, done; };      // orbx_extract_batch: a chunk's upload has landed / its download has

struct orbx_extractor : PlanParams {   // the constructor's arguments and tables, the A/B switches and the table capacities are what the planner reads
    int device = 0, max_w = 0, max_h = 0, max_batch = 0;
    bool need_clear = true;
    int nsub = 1; int overlap_pyr = 0;
    // current plan
    int cur_w = 0, cur_h = 0; int last_batch = 0;
    const uint8_t *last_input = nullptr; int last_in_stride = 0; long long last_in_frame = 0;
    const uint8_t *pin_ptr = nullptr; int pin_n = 0; size_t pin_stride = 0, pin_bytes = 0; bool pin_is = false;   // last is_pinned_host() answer
    // the plan of cur_w x cur_h, committed by ensure_plan(): all of it or none (level 0's source and blur_mode follow the call)
    OrbxPlan plan; ResizeTab tabs[ORBX_MAX_LEVELS]; int resize_mode[ORBX_MAX_LEVELS]; FusePlan fuse[2]; TilePlan tile;
    int oct_cap_max = 0; size_t oct_lds = 0;
    // the layout of the blocks below (sized for the max shape)
    OrbxPlan max_plan; size_t pyr_level_off[ORBX_MAX_LEVELS];
    int in_stride = 0; size_t in_frame = 0;
    size_t out_hdr = 0, out_kps_bytes = 0;
    std::vector<size_t> chunk_off;   // orbx_extract_batch: byte offset of every chunk's own [counts | status | keypoints | descriptors] block in d_out / h_out
    // views, filled by orbx_create: the workspace arrays, and the whole-batch layout of d_out / h_out
    OrbxWork work;
    orbx_keypoint *d_kps = nullptr; uint8_t *d_desc = nullptr; int32_t *d_counts = nullptr, *d_status = nullptr;
    orbx_keypoint *h_kps = nullptr; uint8_t *h_desc = nullptr; int32_t *h_counts = nullptr, *h_status = nullptr;
    int fmt = ORBX_FMT_GRAY8;        // input format (orbx_set_input_format)
    int inflight = 0, inflight_frames = 0;      // orbx_extract_begin / orbx_extract_end
    // orbx_extract_begin replays one HIP graph per shape (upload, ~10 kernels, download) instead of ~12 launches
    int graph_fmt = 0; int graph_w = 0, graph_h = 0, graph_seen_w = 0, graph_seen_h = 0; bool graph_off = false; int graph_fails = 0;
    // orbx_extract_batch in chunks: staging threads, two streams, one HIP graph per chunk (kernels + download) per shape
    int batch_chunk = 16;
    int bg_w = 0, bg_h = 0, bg_n = 0, bg_chunk = 0; bool bg_off = false;
    int profiling = 0; float stage_ms[4] = {0, 0, 0, 0}; long long ring_calls = 0;

    // ---- what the handle owns.  Members die in reverse order: the staging threads stop first, then the graphs, the blocks and the
    // events go, the streams last ----
    DevStream stream, aux[ORBX_MAX_SUB - 1];
    DevEvent ev_fork, ev_join[ORBX_MAX_SUB - 1], ev[5];
    std::vector<OrbxRingSlot> ring;             // profiling == 2: the stage events of the last ORBX_PROF_RING calls, recorded and never waited
                                                // for by the library; all ORBX_PROF_RING slots or none (orbx_set_profiling)
    std::vector<OrbxChunkEvents> chunk_ev;      // grown by orbx_ensure_chunk_events
    DevBuf<uint8_t> d_input, d_pyr;
    DevBuf<int> d_tab_i; DevBuf<short2> d_tab_s;
    DevBuf<uint32_t> d_cells;                   // per-cell (level, row, column) table of the current plan
    DevBuf<int4> d_bands, d_tiles;
    DevBuf<OrbxCand> w_cand, w_sel; DevBuf<OrbxNode> w_arena; DevBuf<uint32_t> w_owner, w_cand_count, w_nk, w_ncand, w_errflags;   // OrbxWork's arrays
    DevBuf<uint8_t> d_out; PinBuf<uint8_t> h_out, h_in;   // d_out / h_out: the one block the eight output views point into
    // A colour frame is converted into d_input by one kernel ahead of the pyramid; the host entry points stage and upload it through
    // h_color / d_color (both or neither: orbx_ensure_color, at the first colour call; pitches follow the call's width)
    DevBuf<uint8_t> d_color; PinBuf<uint8_t> h_color;
    PinBuf<uint8_t> h_pyr;                      // staging of orbx_download_pyramid (orbx_ensure_pyr_staging)
    DevGraphExec graph_exec;
    std::vector<DevGraphExec> bgraph;
    std::unique_ptr<StagePool> pool;
};

// orbx_workspace.cc.  Each lazy resource has one ensure function: on failure the resource is empty, the call returns ORBX_E_HIP
// naming it, and the next call tries again.
std::recursive_mutex &orbx_capture_mutex();
int orbx_ensure_color(orbx_extractor *h);
int orbx_ensure_pyr_staging(orbx_extractor *h, size_t need);
int orbx_ensure_chunk_events(orbx_extractor *h, int nchunks);

// Colour input.  The host entry points stage a colour frame with a pitch of its own row bytes rounded up to 64 (so every staged row is
// aligned for the kernel's wide loads, and a BGR upload is 3x the grey one, not 4x); both blocks are sized for 4 channels at the
// handle's maximum shape, which every smaller frame and every 3-channel frame fits.
static inline int color_pitch(int W, int cn) { return (int)align_up((size_t)W * cn, 64); }
static inline size_t color_frame(int W, int H, int cn) { return align_up((size_t)color_pitch(W, cn) * H, 256); }
