// optimize_sim3_asan_main.cc -- drives orbp_optimize_sim3 and orbp_sim3_from_rts (include/orbp.h) stand-alone, for a build of
// csrc/orbp_sim3opt.cc under AddressSanitizer and UBSan on the CPU (tests/test_optimize_sim3_cxx.py).  The arrays are sized exactly
// (heap vectors of n entries, no slack), so a read or write past a correspondence array is caught.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/orbp.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct Lcg { unsigned s; };
static double uni(Lcg &g, double a, double b)
{
    g.s = (1103515245u * g.s + 12345u) & 0x7fffffffu;
    return a + (b - a) * (g.s / 2147483648.0);
}
static void rodrigues(const double *w, double *R)
{
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), c = cos(th), s = sin(th), x = w[0] / th, y = w[1] / th, z = w[2] / th;
    const double r[9] = {c + (1 - c) * x * x, (1 - c) * x * y - s * z, (1 - c) * x * z + s * y, (1 - c) * x * y + s * z, c + (1 - c) * y * y,
                         (1 - c) * y * z - s * x, (1 - c) * x * z - s * y, (1 - c) * y * z + s * x, c + (1 - c) * z * z};
    memcpy(R, r, sizeof r);
}

// n pairs under a planted S12 (x1 = s R x2 + t), n_wrong gross outliers first; the start is the truth moved a little
static int run(int n, int n_wrong, bool fix, double scale, unsigned seed, double *S_out, double *S_start, std::vector<uint8_t> &flags)
{
    Lcg g{seed};
    const float K1[4] = {718.856f, 718.856f, 607.1928f, 185.2157f}, K2[4] = {517.306408f, 516.469215f, 318.643040f, 255.313989f};
    double R[9], t[3];
    const double w[3] = {uni(g, -0.1, 0.1), uni(g, -0.1, 0.1), uni(g, 0.02, 0.1)};
    rodrigues(w, R);
    for (int k = 0; k < 3; k++) t[k] = uni(g, -0.5, 0.5);
    std::vector<float> x1(3 * n), x2(3 * n), o1(2 * n), o2(2 * n), s1(n), s2(n);
    for (int i = 0; i < n; i++) {
        const double a[3] = {uni(g, -4, 4), uni(g, -2, 2), uni(g, 5, 20)}, d[3] = {a[0] - t[0], a[1] - t[1], a[2] - t[2]};
        double b[3];
        for (int k = 0; k < 3; k++) b[k] = (R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2]) / scale;
        for (int k = 0; k < 3; k++) { x1[3 * i + k] = (float)a[k]; x2[3 * i + k] = (float)b[k]; }
        o1[2 * i] = (float)(K1[0] * a[0] / a[2] + K1[2] + uni(g, -1, 1) + (i < n_wrong ? 50.0 : 0.0));
        o1[2 * i + 1] = (float)(K1[1] * a[1] / a[2] + K1[3] + uni(g, -1, 1));
        o2[2 * i] = (float)(K2[0] * b[0] / b[2] + K2[2] + uni(g, -1, 1));
        o2[2 * i + 1] = (float)(K2[1] * b[1] / b[2] + K2[3] + uni(g, -1, 1));
        s1[i] = (float)(1.0 / pow(1.44, (int)uni(g, 0, 7.99)));
        s2[i] = (float)(1.0 / pow(1.44, (int)uni(g, 0, 7.99)));
    }
    float Rf[9], tf[3];
    double dR[9], R0[9];
    const double dw[3] = {0.02, -0.03, 0.01};
    rodrigues(dw, dR);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R0[3 * r + c] = dR[3 * r] * R[c] + dR[3 * r + 1] * R[3 + c] + dR[3 * r + 2] * R[6 + c];
    for (int k = 0; k < 9; k++) Rf[k] = (float)R0[k];
    for (int k = 0; k < 3; k++) tf[k] = (float)(t[k] + 0.02);
    CHECK(orbp_sim3_from_rts(Rf, tf, (float)(fix ? scale : scale * 1.03), S_out) == 0);
    memcpy(S_start, S_out, 8 * sizeof(double));
    flags.assign(n, 7);
    return orbp_optimize_sim3(n, x1.data(), x2.data(), o1.data(), o2.data(), s1.data(), s2.data(), K1, K2, 10.f, fix ? 1 : 0, S_out, flags.data());
}

int main()
{
    const int sizes[] = {0, 1, 9, 10, 14, 64, 257, 600};
    for (int n : sizes)
        for (int v = 0; v < 4; v++) {
            const bool fix = v & 1, wrong = v & 2;
            const double scale = v == 3 ? 1.0 : 1.3;
            double S[8], S0[8];
            std::vector<uint8_t> flags;
            const int n_wrong = wrong ? (n == 14 ? 6 : n / 5) : 0;
            const int n_in = run(n, n_wrong, fix, scale, 100u + 7u * n + v, S, S0, flags);
            CHECK(n_in >= 0 && n_in <= n - n_wrong);
            for (uint8_t f : flags) CHECK(f == 0 || f == 1);
            for (int i = 0; i < n_wrong; i++) CHECK(flags[i] == 1);
            int kept = 0;
            for (uint8_t f : flags) kept += !f;
            if (n_in > 0) CHECK(kept == n_in);
            if (n - n_wrong < 10) {                            // :1211-1212: S12 comes back as it went in
                CHECK(n_in == 0 && !memcmp(S, S0, sizeof S));
            } else {
                CHECK(n_in >= (n - n_wrong) * 8 / 10);
                if (fix) CHECK(S[7] == (double)(float)scale);
                else CHECK(fabs(S[7] - scale) < 0.02);
                for (int k = 0; k < 8; k++) CHECK(std::isfinite(S[k]));
            }
        }
    // bad arguments
    double S[8] = {0, 0, 0, 1, 0, 0, 0, 1};
    const float K[4] = {500, 500, 320, 240};
    CHECK(orbp_optimize_sim3(-1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, K, K, 10.f, 1, S, nullptr) < 0);
    CHECK(orbp_optimize_sim3(3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, K, K, 10.f, 1, S, nullptr) < 0);
    CHECK(orbp_optimize_sim3(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, K, K, 10.f, 1, S, nullptr) == 0);
    S[4] = NAN;
    CHECK(orbp_optimize_sim3(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, K, K, 10.f, 1, S, nullptr) < 0);
    CHECK(strstr(orbp_last_error(), "finite") != nullptr);
    if (g_fail) { printf("optimize_sim3_asan_main: %d checks failed\n", g_fail); return 1; }
    printf("optimize_sim3_asan_main ok\n");
    return 0;
}
