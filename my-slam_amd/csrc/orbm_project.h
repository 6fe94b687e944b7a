// orbm_project.h -- the per-point projection arithmetic that Frame::isInFrustum (orbm_frustum.hip) and ORBmatcher::Fuse
// (orbm_fuse.hip) share, written once: cv::gemm's small-matrix path, Mat::dot / cv::norm in double,
// MapPoint::PredictScale with the correctly rounded logf and the UNDEFINED rule.
//
// The functions are __host__ __device__: the device side spells every float operation with the __f*_rn intrinsics (no
// contraction whatever the flags), the host side is the same expression in plain C++ (the library is built with
// -ffp-contract=off).  orbm_fuse_views answers a batch without a single key-frame feature on the host through them.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PJ_ADD(a, b) __fadd_rn((a), (b))
#define PJ_SUB(a, b) __fsub_rn((a), (b))
#define PJ_MUL(a, b) __fmul_rn((a), (b))
#define PJ_DIV(a, b) __fdiv_rn((a), (b))
#else
#define PJ_ADD(a, b) ((a) + (b))
#define PJ_SUB(a, b) ((a) - (b))
#define PJ_MUL(a, b) ((a) * (b))
#define PJ_DIV(a, b) ((a) / (b))
#endif

// cv::gemm's small-matrix path for one row of Rcw*P+tcw (orbm_internal.h gemm_row)
__host__ __device__ __forceinline__ float fru_gemm_row(const float *__restrict__ R, float t, float x, float y, float z)
{
    const float t0 = PJ_ADD(PJ_ADD(PJ_MUL(R[0], x), PJ_MUL(R[1], y)), PJ_MUL(R[2], z));
    return (float)((double)t0 + (double)t);
}
// Mat::dot / the squares of cv::norm: float products are exact in double, the sum is double
__host__ __device__ __forceinline__ double fru_dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}
// MapPoint::PredictScale (src/MapPoint.cc:385-417; the Frame and the KeyFrame overload are the same text): float division, logf
// (correctly rounded: the fp64 log rounded to float once), float division, ceil.  false = ORBM_*_UNDEFINED: no int holds the
// ceil (NaN and +-inf included), the conversion of :393 / :410 is undefined in C++.
__host__ __device__ __forceinline__ bool fru_predict_scale(float mf_max, float dist, float log_scale_factor, int nlevels, int &level)
{
    const float ratio = PJ_DIV(mf_max, dist);                                           // :390 / :407
    const float lg = (float)log((double)ratio);                                         // logf, correctly rounded
    const float c = ceilf(PJ_DIV(lg, log_scale_factor));                                // :393 / :410
    if (!(c >= -2147483648.0f && c < 2147483648.0f)) return false;
    level = (int)c;
    if (level < 0) level = 0;                                                           // :394-397 / :411-414
    else if (level >= nlevels) level = nlevels - 1;
    return true;
}
