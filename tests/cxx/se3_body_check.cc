// se3_body_check.cc -- the quaternion / SE3 group of my-slam_amd/csrc/orbp_se3_body.h by itself.  Built stand-alone under
// AddressSanitizer and UBSan by tests/test_se3_body_cxx.py (CPU only).  EPS is the unit roundoff 2^-53; every bound below is a count
// of the roundings on the path times EPS, for entries of magnitude at most 1 (rotations) or times the lengths involved (translations).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "orbp_se3_body.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)
static const double EPS = 1.1102230246251565e-16;
static const double PI = 3.141592653589793;

// Eigen's Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>) in its index form: the
// statement of the algorithm that quat_from_R writes out per case.  Returns the branch: 0 = trace, 1 + i = diagonal entry i
static int ref_quat_from_R(const double *R, Quat &q)
{
    double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        tr = std::sqrt(tr + 1.0);
        q.qw = 0.5 * tr;
        tr = 0.5 / tr;
        q.qx = (R[7] - R[5]) * tr; q.qy = (R[2] - R[6]) * tr; q.qz = (R[3] - R[1]) * tr;
        return 0;
    }
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double v[3];
    tr = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    v[i] = 0.5 * tr;
    tr = 0.5 / tr;
    q.qw = (R[3 * k + j] - R[3 * j + k]) * tr;
    v[j] = (R[3 * j + i] + R[3 * i + j]) * tr;
    v[k] = (R[3 * k + i] + R[3 * i + k]) * tr;
    q.qx = v[0]; q.qy = v[1]; q.qz = v[2];
    return 1 + i;
}

// the six axes of the checks: x, y, z and each 0.05 off towards the next
static void axis(int a, double *ax)
{
    ax[0] = ax[1] = ax[2] = 0;
    ax[a % 3] = 1;
    if (a >= 3) ax[(a + 1) % 3] = 0.05;
    const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    for (int i = 0; i < 3; i++) ax[i] /= n;
}
static void rodrigues(const double *ax, double ang, double *R)
{
    const double K[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    const double s = std::sin(ang), c = 1 - std::cos(ang);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R[3 * i + j] = (i == j) + s * K[3 * i + j] + c * (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j]);
}
// the rotation of a quaternion of any length, in long double: I + (2 / |q|^2) (w [v]x + [v]x^2)
static void rot_ld(const Quat &q, long double *R)
{
    const long double x = q.qx, y = q.qy, z = q.qz, w = q.qw, s = 2 / (x * x + y * y + z * z + w * w);
    R[0] = 1 - s * (y * y + z * z); R[1] = s * (x * y - w * z); R[2] = s * (x * z + w * y);
    R[3] = s * (x * y + w * z); R[4] = 1 - s * (x * x + z * z); R[5] = s * (y * z - w * x);
    R[6] = s * (x * z - w * y); R[7] = s * (y * z + w * x); R[8] = 1 - s * (x * x + y * y);
}

int main()
{
    // 1. quat_from_R against the index form: the same arithmetic, so the same bits, in all four branches
    const double angles[7] = {0, 1e-6, 0.3, 2.2, 2.9, 3.1, PI};
    int branch[4] = {0, 0, 0, 0};
    for (int a = 0; a < 6; a++)
        for (int k = 0; k < 7; k++) {
            double ax[3], R[9];
            axis(a, ax);
            rodrigues(ax, angles[k], R);
            Quat want, got;
            branch[ref_quat_from_R(R, want)]++;
            quat_from_R(R, got);
            CHECK(memcmp(&want, &got, sizeof want) == 0);
        }
    printf("quat_from_R branches: trace %d, x %d, y %d, z %d\n", branch[0], branch[1], branch[2], branch[3]);
    CHECK(branch[0] > 0 && branch[1] > 0 && branch[2] > 0 && branch[3] > 0);
    CHECK(branch[0] + branch[1] + branch[2] + branch[3] == 42);

    // 2. quat_normalize flips a negative w and leaves a unit quaternion
    {
        Quat q;
        q.qx = 0.3; q.qy = -0.4; q.qz = 1.2; q.qw = -0.5;
        quat_normalize(q);
        CHECK(q.qw > 0 && q.qx < 0 && q.qy > 0 && q.qz < 0);
        CHECK(std::fabs(q.qx * q.qx + q.qy * q.qy + q.qz * q.qz + q.qw * q.qw - 1) <= 8 * EPS);
    }

    // 3. se3_exp on either side of theta = 1e-5 and up to 3
    const double thetas[9] = {0, 1e-9, 9.999e-6, 1.0001e-5, 1e-3, 0.3, 2.2, 2.9, 3.0};
    const double ups[3] = {0.7, -1.1, 0.4};
    const double up_len = std::sqrt(0.7 * 0.7 + 1.1 * 1.1 + 0.4 * 0.4);
    double worst_orth = 0, worst_w = 0, worst_t = 0;
    for (int a = 0; a < 6; a++)
        for (int k = 0; k < 9; k++) {
            const double th = thetas[k];
            double ax[3], u[6], m[6];
            axis(a, ax);
            for (int i = 0; i < 3; i++) { u[i] = th * ax[i]; u[3 + i] = ups[i]; m[i] = -u[i]; m[3 + i] = -u[3 + i]; }
            const Se3 E = se3_exp(u), M = se3_exp(m);
            // quat_to_R(exp) is orthonormal.  |q|^2 = 1 + d with |d| <= 10 EPS after quat_normalize (the sum of squares 4, its
            // root 1, the divisions 1 each, counted twice in the squares); toRotationMatrix of such a q is Rot + d (Rot - I), so
            // R^T R = I + d (2 I - Rot - Rot^T), entries <= 4 |d| = 40 EPS; an entry of R carries 4 more roundings of magnitude <= 1
            // and enters R^T R (summed in long double here) in 3 products on either side: 24 EPS.  64 EPS bounds both.
            double R[9];
            quat_to_R(E, R);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    long double s = 0;
                    for (int l = 0; l < 3; l++) s += (long double)R[3 * l + i] * R[3 * l + j];
                    worst_orth = std::fmax(worst_orth, (double)fabsl(s - (i == j)));
                }
            // exp(u) * exp(-u): the rotation.  Omega(-u) = -Omega(u) and Omega^2 are exact, so R(-u) is R(u) with its antisymmetric
            // part negated bit for bit and exp(-u).r is the conjugate of exp(u).r bit for bit; the vector part of q conj(q) then
            // cancels exactly and w = s / sqrt(s * s) is within 2 roundings of 1.
            const Se3 P = se3_mul(E, M);
            CHECK(M.qx == -E.qx && M.qy == -E.qy && M.qz == -E.qz && M.qw == E.qw);
            CHECK(P.qx == 0 && P.qy == 0 && P.qz == 0);
            worst_w = std::fmax(worst_w, std::fabs(P.qw - 1));
            // exp(u) * exp(-u): the translation V(u) v - R V(-u) v vanishes only through R(theta) V(-theta) = V(theta), which ties
            // b = (1 - cos theta) / theta^2 to the other coefficients.  1 - cos theta carries the rounding of cos, 1.5 EPS absolute, so b
            // is off by 2 EPS / theta^2 and the translation by 2 db theta |v| = 4 EPS |v| / theta; the other roundings (c, whose
            // cancellation costs 2 EPS |v|, the products of V, quat_rotate's 32, the unit-norm defect's 20) stay below 64 EPS |v|.
            // Both constants are doubled.  Below 1e-5 g2o takes R = V = I + Omega + Omega^2, which is not the group's exponential:
            // there the translation is (Omega + ...) v, first order in theta, and is bounded by 2 theta |v| instead.
            const double t = std::fmax(std::fabs(P.t0), std::fmax(std::fabs(P.t1), std::fabs(P.t2)));
            if (th < 1e-5) CHECK(t <= 2 * th * up_len + 128 * EPS * up_len);
            else {
                CHECK(t <= (8 / th + 128) * EPS * up_len);
                worst_t = std::fmax(worst_t, t / ((8 / th + 128) * EPS * up_len));
            }
        }
    printf("se3_exp: |R^T R - I| <= %.3g EPS, |w - 1| <= %.3g EPS, translation at most %.3g of its bound\n", worst_orth / EPS,
           worst_w / EPS, worst_t);
    CHECK(worst_orth <= 64 * EPS);
    CHECK(worst_w <= 4 * EPS);

    // 4. se3_mul against the 4 x 4 product in long double.  A component of the quaternion product carries 4 products and 3 sums of
    // magnitude <= 2 (10 EPS) and the normalisation 5 more; a rotation's entries move by at most 4 |dq|_2 <= 8 * 15 EPS = 120 EPS.
    // The translation is quat_rotate's 32 EPS |t_b| (three cross products and sums of magnitude <= 3 |t_b|), the unit-norm defect
    // of a, 20 EPS |t_b|, and the final sum's EPS (|t_a| + |t_b|).  128 EPS and 64 EPS (|t_a| + |t_b|) bound them.
    double worst_R = 0, worst_T = 0;
    for (int a = 0; a < 6; a++)
        for (int k = 2; k < 9; k++) {
            double ax[3], bx[3], u[6], v[6];
            axis(a, ax);
            axis((a + 2) % 6, bx);
            for (int i = 0; i < 3; i++) { u[i] = thetas[k] * ax[i]; u[3 + i] = ups[i]; v[i] = thetas[10 - k] * bx[i]; v[3 + i] = 2 * ups[(i + 1) % 3]; }
            const Se3 A = se3_exp(u), B = se3_exp(v), P = se3_mul(A, B);
            long double RA[9], RB[9], RP[9];
            rot_ld(A, RA); rot_ld(B, RB); rot_ld(P, RP);
            const long double tb[3] = {B.t0, B.t1, B.t2}, ta[3] = {A.t0, A.t1, A.t2}, tp[3] = {P.t0, P.t1, P.t2};
            const double len = std::sqrt(A.t0 * A.t0 + A.t1 * A.t1 + A.t2 * A.t2) + std::sqrt(B.t0 * B.t0 + B.t1 * B.t1 + B.t2 * B.t2);
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) {
                    const long double s = RA[3 * i] * RB[j] + RA[3 * i + 1] * RB[3 + j] + RA[3 * i + 2] * RB[6 + j];
                    worst_R = std::fmax(worst_R, (double)fabsl(s - RP[3 * i + j]));
                }
                const long double s = RA[3 * i] * tb[0] + RA[3 * i + 1] * tb[1] + RA[3 * i + 2] * tb[2] + ta[i];
                worst_T = std::fmax(worst_T, (double)fabsl(s - tp[i]) / len);
            }
            CHECK(P.qw >= 0);
        }
    printf("se3_mul: rotation within %.3g EPS, translation within %.3g EPS (|t_a| + |t_b|)\n", worst_R / EPS, worst_T / EPS);
    CHECK(worst_R <= 128 * EPS);
    CHECK(worst_T <= 64 * EPS);

    // 5. se3_from_Tcw and se3_to_Tcw are each other's inverse up to the float cast, and se3_map is R x + t
    {
        double ax[3], u[6];
        axis(4, ax);
        for (int i = 0; i < 3; i++) { u[i] = 2.9 * ax[i]; u[3 + i] = ups[i]; }
        const Se3 E = se3_exp(u);
        float T[16];
        se3_to_Tcw(E, T);
        const Se3 F = se3_from_Tcw(T);
        CHECK(std::fabs(F.qx - E.qx) < 1e-6 && std::fabs(F.qy - E.qy) < 1e-6 && std::fabs(F.qz - E.qz) < 1e-6 && std::fabs(F.qw - E.qw) < 1e-6);
        CHECK(T[12] == 0 && T[13] == 0 && T[14] == 0 && T[15] == 1 && F.t0 == (double)(float)E.t0);
        const double x[3] = {0.5, -2.0, 7.0};
        double o[3], R[9];
        se3_map(E, x, o);
        quat_to_R(E, R);
        for (int i = 0; i < 3; i++) {
            const double t = i == 0 ? E.t0 : i == 1 ? E.t1 : E.t2;
            CHECK(std::fabs(o[i] - (R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2] + t)) <= 64 * EPS * 8);
        }
    }

    if (failures) return 1;
    printf("se3_body_check ok\n");
    return 0;
}
