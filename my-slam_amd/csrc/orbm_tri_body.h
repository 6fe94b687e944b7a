// orbm_tri_body.h -- the arithmetic of one CreateNewMapPoints match (src/LocalMapping.cc:293-433 of WChen09/My-SLAM) as device
// functions: tri_one() decides a match and gives its point, tri_load() reads what it needs of one feature, tri_lanes() is the kernel
// body around them.  Shared by k_triangulate (orbm_triangulate.hip, a caller's match list) and k_triangulate_queries
// (orbm_newpoints.hip, the matches the batched search left on the device): the two kernels differ only in where a lane fetches its
// pair.  Conventions: orbm_triangulate.hip's header comment.
#pragma once
#include "orbm_internal.h"
#include "orbm_svd4_body.h"   // D4, the 4x4 Jacobi, tri_dot3, tri_arow: shared with the Initializer's CheckRT
#include "sincos_cr.h"

#define TRI_THREADS 64

// cv::gemm's small-matrix path, the float sum of one row (orbm_internal.h gemm3)
__device__ __forceinline__ float tri_sum3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}
// cos(2*atan2(mb/2, depth)) of :314 / :316 with the float overloads, each function correctly rounded
__device__ __forceinline__ float tri_cos_stereo(float mb, float depth)
{
    const float half = __fdiv_rn(mb, 2.0f);
    const float at = (float)atan2((double)half, (double)depth);
    const float ang = __fmul_rn(2.0f, at);
    float cs, sn;
    sincos_cr(fabsf(ang), &cs, &sn);    // |ang| <= 2 pi, cos is even
    return cs;
}

struct TriView {                        // what :293-298 and UnprojectStereo read of one feature
    float x, y, raw_x, raw_y, ur, depth;
    int oct;
};

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631): false where the reference returns an empty matrix
__device__ __forceinline__ bool tri_unproject(const orbm_camera *__restrict__ C, const TriView &f, float X[3])
{
    const float z = f.depth;
    if (!(z > 0)) return false;
    const float x = __fmul_rn(__fmul_rn(__fsub_rn(f.raw_x, C->cx), z), C->invfx);
    const float y = __fmul_rn(__fmul_rn(__fsub_rn(f.raw_y, C->cy), z), C->invfy);
    // Twc.rowRange(0,3).colRange(0,3) = Rcw^T, Twc.rowRange(0,3).col(3) = Ow (src/KeyFrame.cc:66-70)
    X[0] = (float)((double)tri_sum3(C->Rcw[0], C->Rcw[3], C->Rcw[6], x, y, z) + (double)C->Ow[0]);
    X[1] = (float)((double)tri_sum3(C->Rcw[1], C->Rcw[4], C->Rcw[7], x, y, z) + (double)C->Ow[1]);
    X[2] = (float)((double)tri_sum3(C->Rcw[2], C->Rcw[5], C->Rcw[8], x, y, z) + (double)C->Ow[2]);
    return true;
}

// the reprojection test of one view (:365-389 / :392-415); mbf is mpCurrentKeyFrame's in both (:382, :408)
__device__ __forceinline__ bool tri_reprojection_fails(const orbm_camera *__restrict__ C, const TriView &f, bool stereo, float mbf,
                                                       const float X[3], float z)
{
    const float sigma2 = C->level_sigma2[f.oct];
    const float xc = (float)(tri_dot3(C->Rcw[0], C->Rcw[1], C->Rcw[2], X[0], X[1], X[2]) + (double)C->tcw[0]);
    const float yc = (float)(tri_dot3(C->Rcw[3], C->Rcw[4], C->Rcw[5], X[0], X[1], X[2]) + (double)C->tcw[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(C->fx, xc), invz), C->cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(C->fy, yc), invz), C->cy);
    const float ex = __fsub_rn(u, f.x), ey = __fsub_rn(v, f.y);
    const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (!stereo) return (double)e2 > 5.991 * (double)sigma2;
    const float u_r = __fsub_rn(u, __fmul_rn(mbf, invz));
    const float er = __fsub_rn(u_r, f.ur);
    return (double)__fadd_rn(e2, __fmul_rn(er, er)) > 7.8 * (double)sigma2;
}

__device__ __forceinline__ int tri_one(const orbm_camera *__restrict__ C1, const orbm_camera *__restrict__ C2, const TriView &f1,
                                       const TriView &f2, float X[3])
{
    const bool st1 = f1.ur >= 0, st2 = f2.ur >= 0;                                              // :295, :299
    // Check parallax between rays :302-307
    const float xn1x = __fmul_rn(__fsub_rn(f1.x, C1->cx), C1->invfx), xn1y = __fmul_rn(__fsub_rn(f1.y, C1->cy), C1->invfy);
    const float xn2x = __fmul_rn(__fsub_rn(f2.x, C2->cx), C2->invfx), xn2y = __fmul_rn(__fsub_rn(f2.y, C2->cy), C2->invfy);
    const float r1x = tri_sum3(C1->Rcw[0], C1->Rcw[3], C1->Rcw[6], xn1x, xn1y, 1.0f);
    const float r1y = tri_sum3(C1->Rcw[1], C1->Rcw[4], C1->Rcw[7], xn1x, xn1y, 1.0f);
    const float r1z = tri_sum3(C1->Rcw[2], C1->Rcw[5], C1->Rcw[8], xn1x, xn1y, 1.0f);
    const float r2x = tri_sum3(C2->Rcw[0], C2->Rcw[3], C2->Rcw[6], xn2x, xn2y, 1.0f);
    const float r2y = tri_sum3(C2->Rcw[1], C2->Rcw[4], C2->Rcw[7], xn2x, xn2y, 1.0f);
    const float r2z = tri_sum3(C2->Rcw[2], C2->Rcw[5], C2->Rcw[8], xn2x, xn2y, 1.0f);
    const double n1 = sqrt(tri_dot3(r1x, r1y, r1z, r1x, r1y, r1z)), n2 = sqrt(tri_dot3(r2x, r2y, r2z, r2x, r2y, r2z));
    const float cos_rays = (float)(tri_dot3(r1x, r1y, r1z, r2x, r2y, r2z) / (n1 * n2));
    float cos_st1 = __fadd_rn(cos_rays, 1.0f), cos_st2 = cos_st1;                               // :309-311
    if (st1) cos_st1 = tri_cos_stereo(C1->mb, f1.depth);                                        // :313-316
    else if (st2) cos_st2 = tri_cos_stereo(C2->mb, f2.depth);
    const float cos_st = cos_st2 < cos_st1 ? cos_st2 : cos_st1;                                 // std::min :318
    int accepted;
    if (cos_rays < cos_st && cos_rays > 0 && (st1 || st2 || (double)cos_rays < 0.9998)) {       // :321
        // Linear Triangulation Method :324-328; column j of A = element j of the four rows
        const D4 u0 = {(double)tri_arow(xn1x, C1->Rcw[6], C1->Rcw[0]), (double)tri_arow(xn1y, C1->Rcw[6], C1->Rcw[3]),
                       (double)tri_arow(xn2x, C2->Rcw[6], C2->Rcw[0]), (double)tri_arow(xn2y, C2->Rcw[6], C2->Rcw[3])};
        const D4 u1 = {(double)tri_arow(xn1x, C1->Rcw[7], C1->Rcw[1]), (double)tri_arow(xn1y, C1->Rcw[7], C1->Rcw[4]),
                       (double)tri_arow(xn2x, C2->Rcw[7], C2->Rcw[1]), (double)tri_arow(xn2y, C2->Rcw[7], C2->Rcw[4])};
        const D4 u2 = {(double)tri_arow(xn1x, C1->Rcw[8], C1->Rcw[2]), (double)tri_arow(xn1y, C1->Rcw[8], C1->Rcw[5]),
                       (double)tri_arow(xn2x, C2->Rcw[8], C2->Rcw[2]), (double)tri_arow(xn2y, C2->Rcw[8], C2->Rcw[5])};
        const D4 u3 = {(double)tri_arow(xn1x, C1->tcw[2], C1->tcw[0]), (double)tri_arow(xn1y, C1->tcw[2], C1->tcw[1]),
                       (double)tri_arow(xn2x, C2->tcw[2], C2->tcw[0]), (double)tri_arow(xn2y, C2->tcw[2], C2->tcw[1])};
        const D4 v = smallest_right_singular_vector(u0, u1, u2, u3);                            // in place of :331-333
        if ((float)v.d == 0) return ORBM_TRI_W_ZERO;                                            // :335
        X[0] = (float)(v.a / v.d); X[1] = (float)(v.b / v.d); X[2] = (float)(v.c / v.d);        // :339
        accepted = ORBM_TRI_SVD;
    } else if (st1 && cos_st1 < cos_st2) {                                                      // :342
        if (!tri_unproject(C1, f1, X)) return ORBM_TRI_UNDEFINED;
        accepted = ORBM_TRI_STEREO1;
    } else if (st2 && cos_st2 < cos_st1) {                                                      // :346
        if (!tri_unproject(C2, f2, X)) return ORBM_TRI_UNDEFINED;
        accepted = ORBM_TRI_STEREO2;
    } else
        return ORBM_TRI_LOW_PARALLAX;                                                           // :351
    // Check triangulation in front of cameras :356-362
    const float z1 = (float)(tri_dot3(C1->Rcw[6], C1->Rcw[7], C1->Rcw[8], X[0], X[1], X[2]) + (double)C1->tcw[2]);
    if (z1 <= 0) return ORBM_TRI_BEHIND1;
    const float z2 = (float)(tri_dot3(C2->Rcw[6], C2->Rcw[7], C2->Rcw[8], X[0], X[1], X[2]) + (double)C2->tcw[2]);
    if (z2 <= 0) return ORBM_TRI_BEHIND2;
    if (tri_reprojection_fails(C1, f1, st1, C1->mbf, X, z1)) return ORBM_TRI_REPROJ1;           // :365-389
    if (tri_reprojection_fails(C2, f2, st2, C1->mbf, X, z2)) return ORBM_TRI_REPROJ2;           // :392-415
    // Check scale consistency :418-433
    const float a0 = __fsub_rn(X[0], C1->Ow[0]), a1 = __fsub_rn(X[1], C1->Ow[1]), a2 = __fsub_rn(X[2], C1->Ow[2]);
    const float b0 = __fsub_rn(X[0], C2->Ow[0]), b1 = __fsub_rn(X[1], C2->Ow[1]), b2 = __fsub_rn(X[2], C2->Ow[2]);
    const float dist1 = (float)sqrt(tri_dot3(a0, a1, a2, a0, a1, a2)), dist2 = (float)sqrt(tri_dot3(b0, b1, b2, b0, b1, b2));
    if (dist1 == 0 || dist2 == 0) return ORBM_TRI_ZERO_DIST;
    const float ratio_dist = __fdiv_rn(dist2, dist1);
    const float ratio_octave = __fdiv_rn(C1->scale_factors[f1.oct], C2->scale_factors[f2.oct]);
    const float ratio_factor = __fmul_rn(1.5f, C1->scale_factor);                               // :234
    if (__fmul_rn(ratio_dist, ratio_factor) < ratio_octave || ratio_dist > __fmul_rn(ratio_octave, ratio_factor)) return ORBM_TRI_SCALE;
    return accepted;
}

__device__ __forceinline__ TriView tri_load(const orbx_keypoint *__restrict__ kps, const float2 *__restrict__ keys,
                                            const float *__restrict__ ur, const float *__restrict__ depth, long long i)
{
    TriView f;
    f.x = kps[i].x; f.y = kps[i].y; f.oct = kps[i].octave;
    const float2 raw = keys[i];
    f.raw_x = raw.x; f.raw_y = raw.y; f.ur = ur[i]; f.depth = depth[i];
    return f;
}

// The body of both triangulation kernels: lane k decides pair k of n.  fetch(k, idx1, idx2, view) gives the lane's pair and returns
// false when there is none (ORBM_TRI_NO_MATCH); a pair whose indices or octaves do not fit the key frames is ORBM_TRI_BAD_INDEX (the
// host entry points have checked them: reached only through the device-pointer form).  The camera blocks are read at wave-uniform
// addresses (scalar loads): the lanes of a wave are served one second view at a time.
template <class Fetch>
__device__ __forceinline__ void tri_lanes(int k, int n, Fetch fetch,
                                          const orbm_camera *__restrict__ cam1, const orbx_keypoint *__restrict__ kps1,
                                          const float2 *__restrict__ keys1, const float *__restrict__ ur1, const float *__restrict__ depth1, int n1,
                                          const orbm_camera *__restrict__ cams2, int ncams2, const int32_t *__restrict__ off2,
                                          const orbx_keypoint *__restrict__ kps2, const float2 *__restrict__ keys2,
                                          const float *__restrict__ ur2, const float *__restrict__ depth2,
                                          uint8_t *__restrict__ status, float *__restrict__ x3d)
{
    int idx1 = 0, idx2 = 0, v = 0;
    uint32_t view = 0xFFFFFFFFu;                    // 0xFFFFFFFF: nothing (left) to do in this lane
    int st = ORBM_TRI_NO_MATCH;
    float X[3] = {0.f, 0.f, 0.f};
    TriView f1 = {};
    if (k < n && fetch(k, idx1, idx2, v)) {
        st = ORBM_TRI_BAD_INDEX;
        if (v >= 0 && v < ncams2 && idx1 >= 0 && idx1 < n1 && idx2 >= 0) {
            f1 = tri_load(kps1, keys1, ur1, depth1, idx1);
            if (f1.oct >= 0 && f1.oct < min(cam1->nlevels, ORBX_MAX_LEVELS)) view = (uint32_t)v;
        }
    }
    // the second views of this wave, one at a time; a pass retires every lane of its view, so there are at most 64
    for (int pass = 0; pass < 64; pass++) {
        const uint32_t vmin = wave_min_u32(view);
        if (vmin == 0xFFFFFFFFu) break;
        if (view == vmin) {
            // every active lane holds vmin here; taken through readfirstlane the index is a scalar for the compiler as well (inside
            // this branch it puts the lane's own `view` in vmin's place, and the camera block's address would become a vector)
            const uint32_t vu = (uint32_t)__builtin_amdgcn_readfirstlane((int)view);
            view = 0xFFFFFFFFu;
            const orbm_camera *__restrict__ cam2 = cams2 + vu;
            const int base = off2[vu], count = off2[vu + 1] - base;
            if (idx2 < count) {
                const TriView f2 = tri_load(kps2, keys2, ur2, depth2, (long long)base + idx2);
                if (f2.oct >= 0 && f2.oct < min(cam2->nlevels, ORBX_MAX_LEVELS)) st = tri_one(cam1, cam2, f1, f2, X);
            }
        }
    }
    if (k < n) {
        const bool ok = st <= ORBM_TRI_STEREO2;
        status[k] = (uint8_t)st;
        x3d[3 * (long long)k] = ok ? X[0] : 0.f; x3d[3 * (long long)k + 1] = ok ? X[1] : 0.f; x3d[3 * (long long)k + 2] = ok ? X[2] : 0.f;
    }
}
