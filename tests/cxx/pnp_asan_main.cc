// pnp_asan_main.cc -- a stand-alone driver of orbp_pnp_* (include/orbp.h) for AddressSanitizer / UBSan: tests/test_pnp_batch_cpu.py
// compiles it together with csrc/orbp.cc with -fsanitize=address,undefined and runs it on the CPU.  It goes through create / draw /
// queued / get_problem / hypothesis / attach_results / iterate / set_ransac_parameters / destroy on planted scenes: sample sizes 4,
// 6 and 9 (9: the heap path only the host has), a queue that grows over several draws, results for a part of the queue (refused),
// a pose in the middle of the queue, the too-small and the empty solver.
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

static const float K[4] = {718.856f, 716.3f, 607.19f, 185.2f};

static void run_case(int n, int n_wrong, int min_set, int min_inliers, unsigned seed)
{
    Lcg g{seed};
    const double w[3] = {0.1, -0.2, 0.15}, t[3] = {0.2, -0.1, 0.05};
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), c = cos(th), sn = sin(th), x = w[0] / th, y = w[1] / th, z = w[2] / th;
    const double R[9] = {c + (1 - c) * x * x, (1 - c) * x * y - sn * z, (1 - c) * x * z + sn * y, (1 - c) * x * y + sn * z, c + (1 - c) * y * y,
                         (1 - c) * y * z - sn * x, (1 - c) * x * z - sn * y, (1 - c) * y * z + sn * x, c + (1 - c) * z * z};
    std::vector<float> p2d(2 * n + 1), p3d(3 * n + 1), s2(n + 1);
    for (int i = 0; i < n; i++) {
        const double d = uni(g, 4, 40), pc[3] = {uni(g, -0.4, 0.4) * d, uni(g, -0.2, 0.2) * d, d};
        double pw[3];
        for (int k = 0; k < 3; k++) pw[k] = R[k] * (pc[0] - t[0]) + R[3 + k] * (pc[1] - t[1]) + R[6 + k] * (pc[2] - t[2]);
        for (int k = 0; k < 3; k++) p3d[3 * i + k] = (float)pw[k];
        const double du = (30 + (i * 13) % 50) * (i & 1 ? 1 : -1), dv = (30 + (i * 29) % 50) * (i & 2 ? 1 : -1);      // each wrong match its own way
        p2d[2 * i] = (float)(K[0] * pc[0] / pc[2] + K[2] + (i < n_wrong ? du : 0));
        p2d[2 * i + 1] = (float)(K[1] * pc[1] / pc[2] + K[3] + (i < n_wrong ? dv : 0));
        s2[i] = powf(1.2f, 2.f * (i % 8));
    }
    orbp_pnp *a = nullptr, *b = nullptr;
    CHECK(orbp_pnp_create(&a, n, p2d.data(), s2.data(), p3d.data(), K[0], K[1], K[2], K[3]) == 0);
    CHECK(orbp_pnp_create(&b, n, p2d.data(), s2.data(), p3d.data(), K[0], K[1], K[2], K[3]) == 0);
    Lcg ga{seed + 1}, gb{seed + 1};
    orbp_pnp_set_rand(a, lcg_next, &ga, 0x7fffffff);
    orbp_pnp_set_rand(b, lcg_next, &gb, 0x7fffffff);
    CHECK(orbp_pnp_set_ransac_parameters(a, 0.99, min_inliers, 300, min_set, 0.5f, 5.991f) == 0);
    CHECK(orbp_pnp_set_ransac_parameters(b, 0.99, min_inliers, 300, min_set, 0.5f, 5.991f) == 0);
    int max_its = 0, eff_min = 0;
    orbp_pnp_get_ransac_state(b, &eff_min, &max_its, nullptr, nullptr);
    std::vector<float> q2(2 * n + 1), q3(3 * n + 1), qe(n + 1);
    float qK[4];
    int32_t ms = 0;
    CHECK(orbp_pnp_get_problem(b, q2.data(), q3.data(), qe.data(), qK, &ms) == n && ms == min_set && !memcmp(qK, K, sizeof K));
    CHECK(n == 0 || (!memcmp(q2.data(), p2d.data(), 8 * n) && !memcmp(q3.data(), p3d.data(), 12 * n)));
    // b: draw in three steps (the queue grows), evaluate with orbp_pnp_hypothesis, attach, replay; a: evaluate in place
    const int expect = n >= eff_min ? (max_its > 5 ? max_its : 5) : 0;
    std::vector<int32_t> first((size_t)min_set * (expect + 1));
    const int h1 = orbp_pnp_draw(b, 5, first.data());
    CHECK(h1 == expect && orbp_pnp_draw(b, 5, nullptr) == 0);
    const int h2 = orbp_pnp_draw(b, expect + 3, nullptr), h3 = orbp_pnp_draw(b, expect + 40, nullptr);
    CHECK(h2 == (expect ? 3 : 0) && h3 == (expect ? 37 : 0));
    const int h = orbp_pnp_queued(b, nullptr);
    CHECK(h == h1 + h2 + h3);
    std::vector<int32_t> sets((size_t)min_set * h + 1);
    CHECK(orbp_pnp_queued(b, sets.data()) == h && (h == 0 || !memcmp(sets.data(), first.data(), sizeof(int32_t) * min_set * h1)));
    const int W = (n + 31) / 32;
    std::vector<int32_t> counts(h + 1);
    std::vector<double> Rt(12 * (size_t)h + 1);
    std::vector<uint32_t> masks((size_t)W * h + 1, 0u);
    std::vector<uint8_t> inl(n + 1), inl2(n + 1);
    for (int k = 0; k < h; k++) {
        CHECK(orbp_pnp_hypothesis(b, &sets[(size_t)min_set * k], &Rt[12 * k], &Rt[12 * k + 9], inl.data(), &counts[k]) == 0);
        for (int i = 0; i < n; i++) if (inl[i]) masks[(size_t)W * k + i / 32] |= 1u << (i % 32);
    }
    if (h > 1) CHECK(orbp_pnp_attach_results(b, h - 1, counts.data(), Rt.data(), masks.data()) < 0);      // a part of the queue
    CHECK(orbp_pnp_attach_results(b, h, counts.data(), Rt.data(), masks.data()) == 0);
    int poses = 0, calls = 0;
    for (; calls < 400; calls++) {
        int nm_a = 0, nm_b = 0, na = 0, nb = 0;
        float Ta[16], Tb[16];
        memset(inl.data(), 0, n + 1); memset(inl2.data(), 0, n + 1);
        const int ra = orbp_pnp_iterate(a, 5, &nm_a, inl.data(), &na, Ta), rb = orbp_pnp_iterate(b, 5, &nm_b, inl2.data(), &nb, Tb);
        int ia = 0, ib = 0;
        orbp_pnp_get_ransac_state(a, nullptr, nullptr, nullptr, &ia);
        orbp_pnp_get_ransac_state(b, nullptr, nullptr, nullptr, &ib);
        CHECK(ra == rb && nm_a == nm_b && na == nb && ia == ib && !memcmp(inl.data(), inl2.data(), n));
        if (ra == 1) {
            poses++;
            CHECK(!memcmp(Ta, Tb, sizeof Ta));
            for (int i = 0; i < n_wrong; i++) CHECK(!inl[i]);
        }
        if (nm_a || nm_b) break;
    }
    CHECK(calls < 400);
    // new parameters drop what is left of the queue; the solver goes on drawing for itself
    CHECK(orbp_pnp_set_ransac_parameters(b, 0.99, min_inliers, 300, min_set, 0.5f, 5.991f) == 0 && orbp_pnp_queued(b, nullptr) == 0);
    int na = 0;
    float T[16];
    orbp_pnp_find(b, inl.data(), &na, T);
    if (n > 0) {
        std::vector<int32_t> bad(min_set);
        for (int k = 0; k < min_set; k++) bad[k] = k;
        bad[min_set - 1] = n;
        double Rr[9], tt[3];
        CHECK(orbp_pnp_hypothesis(a, bad.data(), Rr, tt, inl.data(), &na) < 0);
        bad[min_set - 1] = 0;
        CHECK(orbp_pnp_hypothesis(a, bad.data(), Rr, tt, inl.data(), &na) < 0);
    }
    orbp_pnp_destroy(a);
    orbp_pnp_destroy(b);
    printf("n=%d wrong=%d min_set=%d: %d hypotheses, %d calls, %d poses\n", n, n_wrong, min_set, h, calls + 1, poses);
}

int main()
{
    run_case(60, 20, 4, 10, 5);          // poses in the middle of the queue
    run_case(90, 36, 6, 10, 6);
    run_case(70, 20, 9, 10, 7);          // a sample the kernel does not take: heap storage around the same body
    run_case(50, 20, 4, 45, 8);          // no hypothesis reaches min_inliers: every iteration runs
    run_case(33, 0, 4, 33, 9);           // n == min_inliers: one iteration
    run_case(5, 0, 4, 10, 10);           // n < min_inliers: nothing is drawn
    run_case(0, 0, 4, 10, 11);
    orbp_pnp_destroy(nullptr);
    if (g_fail) { printf("pnp_asan_main: %d checks failed\n", g_fail); return 1; }
    printf("pnp_asan_main ok\n");
    return 0;
}
