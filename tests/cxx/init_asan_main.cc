// init_asan_main.cc -- a stand-alone driver of orbp_init_* (include/orbp.h) for AddressSanitizer / UBSan: tests/test_initializer_cxx.py
// compiles it together with csrc/orbp_init.cc and csrc/orbp.cc with -fsanitize=address,undefined and runs it on the CPU.  It goes
// through create / set_current / draw / hypothesis / attach_results / find / motions / check_rt / check_rt_matches /
// attach_check_rt / plan_check_rt / initialize / destroy on planted scenes (points in a volume and on a plane, a fifth of the
// matches wrong), on a second current frame of the same handle, on 7 matches, on no iterations and on empty frames.
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

static const float FX = 517.3f, FY = 516.5f, CX = 318.6f, CY = 255.3f;

struct Scene { std::vector<float> k1, k2; std::vector<int32_t> m; int n1; };

static Scene make(int n, bool plane, int n_wrong, unsigned seed)
{
    Lcg g{seed};
    const double th = 0.09, c = cos(th), s = sin(th), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {-1.0, 0.05, 0.03};
    Scene sc;
    sc.n1 = n + n / 4 + 2;
    sc.k1.resize(2 * sc.n1 + 2); sc.k2.resize(2 * sc.n1 + 2); sc.m.assign(sc.n1 + 1, -1);
    for (int i = 0; i < sc.n1; i++) {
        const double x = uni(g, -3, 3), y = uni(g, -2, 2), z = plane ? 6 + 1.0 * x - 0.5 * y : uni(g, 4, 10), p[3] = {x, y, z};
        double q[3];
        for (int k = 0; k < 3; k++) q[k] = R[3 * k] * p[0] + R[3 * k + 1] * p[1] + R[3 * k + 2] * p[2] + t[k];
        const int j = sc.n1 - 1 - i;
        sc.k1[2 * i] = (float)(FX * p[0] / p[2] + CX + uni(g, -0.2, 0.2)); sc.k1[2 * i + 1] = (float)(FY * p[1] / p[2] + CY + uni(g, -0.2, 0.2));
        sc.k2[2 * j] = (float)(FX * q[0] / q[2] + CX + uni(g, -0.2, 0.2)) + (i < n_wrong ? 35.f : 0.f);
        sc.k2[2 * j + 1] = (float)(FY * q[1] / q[2] + CY + uni(g, -0.2, 0.2)) - (i < n_wrong ? 80.f : 0.f);
        if (i < n) sc.m[i] = j;
    }
    return sc;
}

static void run_case(int n, bool plane, int n_wrong, int iterations, bool expect, unsigned seed)
{
    const Scene sc = make(n, plane, n_wrong, seed);
    orbp_init *a = nullptr, *b = nullptr;
    CHECK(orbp_init_create(&a, sc.k1.data(), sc.n1, FX, FY, CX, CY, 1.0f, iterations) == 0);
    CHECK(orbp_init_create(&b, sc.k1.data(), sc.n1, FX, FY, CX, CY, 1.0f, iterations) == 0);
    Lcg ga{seed + 1}, gb{seed + 1};
    orbp_init_set_rand(a, lcg_next, &ga, 0x7fffffff);
    orbp_init_set_rand(b, lcg_next, &gb, 0x7fffffff);
    const int N = orbp_init_set_current(a, sc.k2.data(), sc.n1, sc.m.data());
    CHECK(N == n && orbp_init_set_current(b, sc.k2.data(), sc.n1, sc.m.data()) == n);
    std::vector<float> Ra(9), ta(3), Pa(3 * sc.n1 + 3), Rb(9), tb(3), Pb(3 * sc.n1 + 3);
    std::vector<uint8_t> Ta(sc.n1 + 1), Tb(sc.n1 + 1);
    if (n < 8) {
        CHECK(orbp_init_draw(a, nullptr) < 0 && orbp_init_initialize(a, Ra.data(), ta.data(), Pa.data(), Ta.data()) < 0);
        orbp_init_destroy(a); orbp_init_destroy(b);
        printf("n=%d: refused\n", n);
        return;
    }
    // a: everything in place.  b: draw, evaluate every hypothesis, attach, plan, CheckRT per match, attach, initialize
    const int ok_a = orbp_init_initialize(a, Ra.data(), ta.data(), Pa.data(), Ta.data());
    CHECK(ok_a == (expect ? 1 : 0));
    std::vector<int32_t> sets(8 * (size_t)iterations + 8);
    CHECK(orbp_init_draw(b, sets.data()) == iterations);
    const int H = 2 * iterations, W = (N + 31) / 32;
    std::vector<float> sm(10 * (size_t)H + 1);
    std::vector<int32_t> counts(H + 1);
    std::vector<uint32_t> masks((size_t)W * H + 1, 0u);
    std::vector<uint8_t> inl(N + 1);
    for (int h = 0; h < H; h++) {
        CHECK(orbp_init_hypothesis(b, h / iterations, &sets[8 * (size_t)(h % iterations)], &sm[10 * (size_t)h + 1], &sm[10 * (size_t)h], inl.data(), &counts[h]) == 0);
        for (int i = 0; i < N; i++) if (inl[i]) masks[(size_t)W * h + i / 32] |= 1u << (i % 32);
    }
    CHECK(orbp_init_attach_results(b, H, sm.data(), counts.data(), masks.data()) == 0);
    CHECK(orbp_init_attach_results(b, H + 1, sm.data(), counts.data(), masks.data()) < 0);
    float M[9], Rt[96], score = 0;
    int model = -1, nm = 0, best = -2;
    CHECK(orbp_init_find(b, 1, M, &score, inl.data(), &best) == (iterations ? 1 : 0));
    CHECK(orbp_init_plan_check_rt(b, &model, M, inl.data(), Rt, &nm) == nm && (nm == 0 || nm == 4 || nm == 8));
    if (nm) {
        std::vector<uint8_t> st((size_t)nm * N + 1);
        std::vector<float> cs((size_t)nm * N + 1), pp(3 * (size_t)nm * N + 3);
        CHECK(orbp_init_check_rt_matches(b, nm, Rt, inl.data(), st.data(), cs.data(), pp.data()) == 0);
        float par = 0; int ng = 0, cnt = 0;
        CHECK(orbp_init_check_rt(b, Rt, Rt + 9, inl.data(), Pb.data(), Tb.data(), &par, &ng) == 0);
        for (int i = 0; i < N; i++) cnt += st[i] <= 1;
        CHECK(cnt == ng);
        CHECK(orbp_init_attach_check_rt(b, nm, Rt, inl.data(), st.data(), cs.data(), pp.data()) == 0);
        float Rt2[96]; int nm2 = 0;
        CHECK(orbp_init_motions(b, model, M, Rt2, &nm2) == 1 && nm2 == nm && !memcmp(Rt, Rt2, 48 * (size_t)nm));
    }
    std::fill(Pb.begin(), Pb.end(), 0.f); std::fill(Tb.begin(), Tb.end(), 0);
    const int ok_b = orbp_init_initialize(b, Rb.data(), tb.data(), Pb.data(), Tb.data());
    CHECK(ok_a == ok_b);
    if (ok_a == 1) CHECK(Ra == Rb && ta == tb && Pa == Pb && Ta == Tb && fabs(Ra[0] - cos(0.09)) < 0.05);
    const int32_t bad[8] = {0, 1, 2, 3, 4, 5, 6, N};
    CHECK(orbp_init_hypothesis(a, 0, bad, M, &score, inl.data(), &nm) < 0 && orbp_init_hypothesis(a, 2, sets.data(), M, &score, inl.data(), &nm) < 0);
    // another current frame on the same handle: fewer matches, nothing of the first pair is left
    std::vector<int32_t> m2(sc.m);
    for (int i = 0; i < sc.n1; i += 3) m2[i] = -1;
    const int N2 = orbp_init_set_current(a, sc.k2.data(), sc.n1, m2.data());
    CHECK(N2 < N && orbp_init_find(a, 0, M, &score, inl.data(), &best) < 0);           // nothing drawn for this pair yet
    if (N2 >= 8) CHECK(orbp_init_initialize(a, Ra.data(), ta.data(), Pa.data(), Ta.data()) >= 0);
    orbp_init_destroy(a);
    orbp_init_destroy(b);
    printf("n=%d plane=%d wrong=%d iterations=%d: initialised %d, model %d\n", n, (int)plane, n_wrong, iterations, ok_a, model);
}

int main()
{
    run_case(150, false, 30, 200, true, 5);
    run_case(150, true, 30, 200, true, 6);
    run_case(65, false, 0, 50, true, 7);
    run_case(9, true, 0, 5, false, 8);
    run_case(8, false, 0, 1, false, 9);
    run_case(7, false, 0, 5, false, 10);
    run_case(64, false, 0, 0, false, 11);      // no iterations: SH == SF == 0, refused
    orbp_init *e = nullptr;
    CHECK(orbp_init_create(&e, nullptr, 0, FX, FY, CX, CY, 1.0f, 5) == 0);
    CHECK(orbp_init_set_current(e, nullptr, 0, nullptr) == 0 && orbp_init_draw(e, nullptr) < 0);
    orbp_init_destroy(e);
    orbp_init_destroy(nullptr);
    CHECK(orbp_init_create(&e, nullptr, 3, FX, FY, CX, CY, 1.0f, 5) < 0 && e == nullptr);
    if (g_fail) { printf("init_asan_main: %d checks failed\n", g_fail); return 1; }
    printf("init_asan_main ok\n");
    return 0;
}
