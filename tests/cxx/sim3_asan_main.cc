// sim3_asan_main.cc -- a stand-alone driver of orbp_sim3_* (include/orbp.h) for AddressSanitizer / UBSan: tests/test_sim3_cxx.py
// compiles it together with csrc/orbp_sim3.cc and csrc/orbp.cc with -fsanitize=address,undefined and runs it on the CPU.  It goes
// through create / draw / hypothesis / attach_results / iterate / find / get_estimated / destroy on two planted cases (64
// correspondences with 16 outliers and free scale; 21 correspondences, fixed scale) and on the empty and the too-small solver.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/orbp.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct Lcg { unsigned s; };
static int lcg_next(void *ctx) { Lcg *g = (Lcg *)ctx; g->s = (1103515245u * g->s + 12345u) & 0x7fffffffu; return (int)g->s; }
static double uni(Lcg &g, double a, double b) { return a + (b - a) * (lcg_next(&g) / 2147483648.0); }

static const float K1[4] = {525.f, 530.f, 319.5f, 239.5f}, K2[4] = {718.856f, 716.3f, 607.19f, 185.2f};

static void run_case(int n, int n_out, bool fix, unsigned seed)
{
    Lcg g{seed};
    const double s = fix ? 1.0 : 1.4, w[3] = {0.1, -0.2, 0.15}, t[3] = {0.2, -0.1, 0.05};
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), c = cos(th), sn = sin(th), x = w[0] / th, y = w[1] / th, z = w[2] / th;
    const double R[9] = {c + (1 - c) * x * x, (1 - c) * x * y - sn * z, (1 - c) * x * z + sn * y, (1 - c) * x * y + sn * z, c + (1 - c) * y * y,
                         (1 - c) * y * z - sn * x, (1 - c) * x * z - sn * y, (1 - c) * y * z + sn * x, c + (1 - c) * z * z};
    std::vector<float> x1(3 * n), x2(3 * n), s1(n), s2(n);
    for (int i = 0; i < n; i++) {
        const double d = uni(g, 3, 9), p[3] = {uni(g, -0.4, 0.4) * d, uni(g, -0.25, 0.25) * d, d};
        double q[3];
        for (int k = 0; k < 3; k++) q[k] = s * (R[3 * k] * p[0] + R[3 * k + 1] * p[1] + R[3 * k + 2] * p[2]) + t[k];
        if (i < n_out) q[0] += 300.0 / K1[0] * q[2];
        for (int k = 0; k < 3; k++) { x2[3 * i + k] = (float)p[k]; x1[3 * i + k] = (float)q[k]; }
        s1[i] = powf(1.2f, 2.f * (i % 8)); s2[i] = powf(1.2f, 2.f * ((i / 8) % 8));
    }
    orbp_sim3 *a = nullptr, *b = nullptr;
    CHECK(orbp_sim3_create(&a, n, x1.data(), x2.data(), s1.data(), s2.data(), K1, K2, fix) == 0);
    CHECK(orbp_sim3_create(&b, n, x1.data(), x2.data(), s1.data(), s2.data(), K1, K2, fix) == 0);
    Lcg ga{seed + 1}, gb{seed + 1};
    orbp_sim3_set_rand(a, lcg_next, &ga, 0x7fffffff);
    orbp_sim3_set_rand(b, lcg_next, &gb, 0x7fffffff);
    CHECK(orbp_sim3_set_ransac_parameters(a, 0.99, 20, 300) == 0 && orbp_sim3_set_ransac_parameters(b, 0.99, 20, 300) == 0);
    int max_its = 0;
    orbp_sim3_get_ransac_state(b, nullptr, &max_its, nullptr, nullptr, nullptr);
    // b: draw everything, evaluate with orbp_sim3_hypothesis, attach, replay; a: evaluate in place
    std::vector<int32_t> tri(3 * (size_t)max_its + 3);
    const int h = orbp_sim3_draw(b, max_its + 7, tri.data());
    CHECK(h == (n >= 20 ? max_its : 0) && orbp_sim3_queued(b, nullptr) == h);
    const int W = (n + 31) / 32;
    std::vector<int32_t> counts(h + 1);
    std::vector<float> sRt(13 * (size_t)h + 1);
    std::vector<uint32_t> masks((size_t)W * h + 1, 0u);
    std::vector<uint8_t> inl(n + 1), inl2(n + 1);
    for (int k = 0; k < h; k++) {
        CHECK(orbp_sim3_hypothesis(b, &tri[3 * k], &sRt[13 * k + 1], &sRt[13 * k + 10], &sRt[13 * k], inl.data(), &counts[k]) == 0);
        for (int i = 0; i < n; i++) if (inl[i]) masks[(size_t)W * k + i / 32] |= 1u << (i % 32);
    }
    CHECK(orbp_sim3_attach_results(b, h, counts.data(), sRt.data(), masks.data()) == 0);
    int poses = 0;
    for (int call = 0; call < 400; call++) {
        int nm_a = 0, nm_b = 0, na = 0, nb = 0;
        float Ta[16], Tb[16];
        const int ra = orbp_sim3_iterate(a, 5, &nm_a, inl.data(), &na, Ta), rb = orbp_sim3_iterate(b, 5, &nm_b, inl2.data(), &nb, Tb);
        CHECK(ra == rb && nm_a == nm_b && na == nb && !memcmp(inl.data(), inl2.data(), n));
        if (ra == 1) {
            poses++;
            CHECK(!memcmp(Ta, Tb, sizeof Ta) && na == n - n_out);
            for (int i = 0; i < n; i++) CHECK(inl[i] == (i >= n_out));
            float Re[9], te[3], se;
            CHECK(orbp_sim3_get_estimated(a, Re, te, &se) == 1 && fabs(se - s) < 1e-3);
        }
        if (nm_a) break;
    }
    CHECK(n > 20 ? poses > 0 : poses == 0);
    int na = 0;
    float T[16];
    orbp_sim3_set_ransac_parameters(a, 0.99, 20, 300);
    CHECK(orbp_sim3_find(a, inl.data(), &na, T) == (n > 20 ? 1 : 0));
    const int32_t bad[3] = {0, 1, n};
    float Rr[9], tt[3], ss;
    CHECK(orbp_sim3_hypothesis(a, bad, Rr, tt, &ss, inl.data(), &na) < 0);
    orbp_sim3_destroy(a);
    orbp_sim3_destroy(b);
    printf("n=%d outliers=%d fix=%d: %d hypotheses, %d poses\n", n, n_out, (int)fix, h, poses);
}

int main()
{
    run_case(64, 16, false, 5);
    run_case(21, 0, true, 6);
    run_case(20, 0, false, 7);          // n == minInliers: one iteration, no pose
    run_case(2, 0, true, 8);            // n < minInliers: nothing is drawn
    run_case(0, 0, false, 9);
    orbp_sim3_destroy(nullptr);
    if (g_fail) { printf("sim3_asan_main: %d checks failed\n", g_fail); return 1; }
    printf("sim3_asan_main ok\n");
    return 0;
}
