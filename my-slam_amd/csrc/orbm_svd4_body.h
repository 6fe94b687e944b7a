// orbm_svd4_body.h -- the 4x4 linear-triangulation pieces shared by CreateNewMapPoints (orbm_tri_body.h: k_triangulate,
// k_triangulate_queries) and the monocular Initializer's CheckRT (orbp_init_body.h: host solver and k_init_check_rt): the right
// singular vector of the smallest singular value by a one-sided Jacobi in double, one element of `x*P.row(2)-P.row(0)`, and the
// double-accumulating dot of three float pairs.  + - * / sqrt only, every sum in one written order: host and device agree byte for
// byte under the build's -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define SVD4_HD __host__ __device__ __forceinline__
#else
#define SVD4_HD static inline
#endif

#define TRI_MAX_SWEEPS 12
// a column pair is left alone once |p.q| <= TRI_TOL |p| |q| (2^-50)
#define TRI_TOL 8.8817841970012523e-16

struct D4 { double a, b, c, d; };

SVD4_HD double d4_dot(const D4 &p, const D4 &q) { return ((p.a * q.a + p.b * q.b) + p.c * q.c) + p.d * q.d; }

// one Jacobi rotation of the column pair (p, q) of U, applied to V as well; false when the pair is already orthogonal
SVD4_HD bool jacobi_pair(D4 &up, D4 &uq, D4 &vp, D4 &vq)
{
    const double alpha = d4_dot(up, up), beta = d4_dot(uq, uq), gamma = d4_dot(up, uq);
    if (!(__builtin_fabs(gamma) > TRI_TOL * __builtin_sqrt(alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = __builtin_copysign(1.0, zeta) / (__builtin_fabs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / __builtin_sqrt(1.0 + t * t), s = c * t;
    D4 n;
    n.a = c * up.a - s * uq.a; uq.a = s * up.a + c * uq.a; up.a = n.a;
    n.b = c * up.b - s * uq.b; uq.b = s * up.b + c * uq.b; up.b = n.b;
    n.c = c * up.c - s * uq.c; uq.c = s * up.c + c * uq.c; up.c = n.c;
    n.d = c * up.d - s * uq.d; uq.d = s * up.d + c * uq.d; up.d = n.d;
    n.a = c * vp.a - s * vq.a; vq.a = s * vp.a + c * vq.a; vp.a = n.a;
    n.b = c * vp.b - s * vq.b; vq.b = s * vp.b + c * vq.b; vp.b = n.b;
    n.c = c * vp.c - s * vq.c; vq.c = s * vp.c + c * vq.c; vp.c = n.c;
    n.d = c * vp.d - s * vq.d; vq.d = s * vp.d + c * vq.d; vp.d = n.d;
    return true;
}

// the right singular vector of the smallest singular value of the 4x4 matrix with columns u0..u3 (the first column of minimal
// norm after the sweeps)
SVD4_HD D4 smallest_right_singular_vector(D4 u0, D4 u1, D4 u2, D4 u3)
{
    D4 v0 = {1.0, 0.0, 0.0, 0.0}, v1 = {0.0, 1.0, 0.0, 0.0}, v2 = {0.0, 0.0, 1.0, 0.0}, v3 = {0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < TRI_MAX_SWEEPS; sweep++) {
        bool any = jacobi_pair(u0, u1, v0, v1);
        any |= jacobi_pair(u0, u2, v0, v2);
        any |= jacobi_pair(u0, u3, v0, v3);
        any |= jacobi_pair(u1, u2, v1, v2);
        any |= jacobi_pair(u1, u3, v1, v3);
        any |= jacobi_pair(u2, u3, v2, v3);
        if (!any) break;                // every further sweep would leave every pair alone as well
    }
    double best = d4_dot(u0, u0);
    D4 v = v0;
    const double s1 = d4_dot(u1, u1), s2 = d4_dot(u2, u2), s3 = d4_dot(u3, u3);
    if (s1 < best) { best = s1; v = v1; }
    if (s2 < best) { best = s2; v = v2; }
    if (s3 < best) { best = s3; v = v3; }
    return v;
}

// Mat::dot / the squares of cv::norm: float products are exact in double, the sum is double
SVD4_HD double tri_dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}
// one element of `alpha*rowA - rowB` (LocalMapping.cc:325-328, Initializer.cc:738-741): MatOp_AddEx hands alpha != 1, beta = -1 to
// cv::addWeighted, whose 32f kernel works in double and adds gamma = 0; alpha == 1 is cv::subtract in float
SVD4_HD float tri_arow(float alpha, float a, float b)
{
    if (alpha == 1.0f) return a - b;
    return (float)(((double)a * (double)alpha + (double)b * -1.0) + 0.0);
}
