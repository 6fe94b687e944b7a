// orbm_bow_body.h -- SearchByBoW's selection for one pair of equal vocabulary nodes (src/ORBmatcher.cc:199-232 of WChen09/My-SLAM) as
// a device function: bow_walk() is the body of one wave of k_bow_select_batch (orbm_bow.hip), which finds a work item's arrays in
// the one block a call uploads and serves the one-candidate and the batch entry points alike.
//
// The node's SERIAL-side features are visited in list order (the loop is sequential in the reference because a feature taken by an
// earlier one is skipped, :209), staged 64 at a time in wave-private LDS; the lanes hold the node's LANE-side features (position =
// chunk * 64 + lane, a "taken" bit per chunk in a register, the first BOW_REG_CHUNKS chunks in registers); key = distance << 16 |
// position, so that min() is "smallest distance, first in list".  A lane-side feature lives in exactly one node, so the waves of
// one table do not interact.  No block-wide barrier: whole waves leave early, and the waves of a workgroup may serve different
// tables.
#pragma once
#include "orbm_accept.h"

#define BOW_NONE ((256u << 16) | 0xFFFFu)
#define BOW_MAX_NODE_FEATURES 4096      // 64 chunks of 64 lanes
#define BOW_REG_CHUNKS 4                // lane-side features 0..255 of a node stay in registers
#define BOW_WAVES (M_THREADS / 64)

struct BowStage {                       // wave-private staging of one workgroup
    uint4 q[BOW_WAVES][64][2];
    int ikf[BOW_WAVES][64];
};

// sd / ld: the descriptors of the serial and of the lane side; s_idx[p.x .. p.y) / l_idx[p.z .. p.w): the node's feature indices
// (into sd / ld, valid and out); valid: NULL or one byte per serial-side feature (:193-197); out[lane-side feature] = the
// serial-side feature that took it, or -1: the wave writes the entries of its own node and no other.
__device__ __forceinline__ void bow_walk(BowStage &st, int wv, int lane, const uint4 *__restrict__ sd, const uint4 *__restrict__ ld,
                                         const int32_t *__restrict__ s_idx, const int32_t *__restrict__ l_idx, const int4 p,
                                         const uint8_t *__restrict__ valid, float nnratio, int th, int32_t *__restrict__ out)
{
    const int nF = p.w - p.z;
    const int nch = (nF + 63) >> 6;
    uint4 ta[BOW_REG_CHUNKS], tb[BOW_REG_CHUNKS];
#pragma unroll
    for (int ch = 0; ch < BOW_REG_CHUNKS; ch++) {
        const int pos = ch * 64 + lane;
        const int fi = pos < nF ? l_idx[p.z + pos] : 0;
        const uint4 *T = ld + 2 * (long long)fi;
        ta[ch] = T[0]; tb[ch] = T[1];
    }
    for (int pos = lane; pos < nF; pos += 64) out[l_idx[p.z + pos]] = -1;     // this wave owns these entries
    unsigned long long taken = 0;
    for (int c0 = p.x; c0 < p.y; c0 += 64) {
        const int nb = min(64, p.y - c0);
        {
            int ikf = -1;
            if (lane < nb) {
                ikf = s_idx[c0 + lane];
                if (valid && !valid[ikf]) ikf = -1;      // :193-197
            }
            const uint4 *Q = sd + 2 * (long long)max(ikf, 0);
            st.q[wv][lane][0] = Q[0]; st.q[wv][lane][1] = Q[1];
            st.ikf[wv][lane] = ikf;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): this wave's LDS writes have landed
        for (int j = 0; j < nb; j++) {
            const int ikf = st.ikf[wv][j];
            if (ikf < 0) continue;               // wave-uniform
            const uint4 q0 = st.q[wv][j][0], q1 = st.q[wv][j][1];
            uint32_t bk = BOW_NONE, sk = BOW_NONE;
#pragma unroll
            for (int ch = 0; ch < BOW_REG_CHUNKS; ch++) {
                const int pos = ch * 64 + lane;
                const uint32_t key = ((uint32_t)hamming256(q0, q1, ta[ch], tb[ch]) << 16) | (uint32_t)pos;
                const uint32_t k2 = (pos < nF && !((taken >> ch) & 1ull)) ? key : BOW_NONE;
                sk = med3u(bk, sk, k2); bk = min(bk, k2);
            }
            for (int ch = BOW_REG_CHUNKS; ch < nch; ch++) {
                const int pos = ch * 64 + lane;
                if (pos < nF && !((taken >> ch) & 1ull)) {
                    const uint4 *Tj = ld + 2 * (long long)l_idx[p.z + pos];
                    const uint32_t key = ((uint32_t)hamming256(q0, q1, Tj[0], Tj[1]) << 16) | (uint32_t)pos;
                    sk = med3u(bk, sk, key); bk = min(bk, key);
                }
            }
            uint32_t B, S2;
            wave_best2<0>(bk, sk, B, S2);            // the winner's position is unique: every other lane offers its best
            const int best1 = (int)(B >> 16), best2 = (int)(S2 >> 16);
            if (best1 <= th && (float)best1 < __fmul_rn(nnratio, (float)best2)) {     // :228-232 (th = TH_LOW), :598-600 (th = TH_LOW - 1)
                const int pos = (int)(B & 0xFFFFu);
                if (lane == (pos & 63)) {
                    taken |= 1ull << (pos >> 6);
                    out[l_idx[p.z + pos]] = ikf;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();         // the next batch overwrites the staging
    }
}
