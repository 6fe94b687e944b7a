// lba_asan_main.cc -- drives orbp_local_bundle_adjustment (csrc/orbp_lba.cc) stand-alone under AddressSanitizer and UBSan on the
// CPU, as optimize_sim3_asan_main.cc does for orbp_optimize_sim3: host code only, its own main, exactly sized heap arrays, so a read
// or write one element past any input or output is reported.  Built by tests/test_lba_cxx.py from this file, orbp_lba.cc and orbp.cc.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2654435761u + 88172645463325252ull) {}
    double uniform() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; }
    double uniform(double a, double b) { return a + (b - a) * uniform(); }
    double normal() { double v = 0; for (int i = 0; i < 12; i++) v += uniform(); return v - 6.0; }
};

// exactly sized arrays on the heap
template <class T> struct Arr {
    std::unique_ptr<T[]> p; size_t n;
    explicit Arr(const std::vector<T> &v) : p(v.empty() ? nullptr : new T[v.size()]), n(v.size()) { if (n) memcpy(p.get(), v.data(), n * sizeof(T)); }
    T *get() const { return p.get(); }
};

struct Problem {
    int n_local, n_fixed, n_points;
    std::vector<uint8_t> local_fixed;
    std::vector<float> Tcw, cam, xw, obs, ur, inv;
    std::vector<int32_t> off, kf;
};

// key frames side by side looking down z (identity rotations, the free ones a few centimetres off), points 6 .. 20 m ahead
static Problem make(int n_local, int n_fixed, int n_points, int id0, double outliers, uint64_t seed)
{
    Rng rng(seed);
    Problem P;
    P.n_local = n_local; P.n_fixed = n_fixed; P.n_points = n_points;
    const int NK = n_local + n_fixed;
    std::vector<double> cx(NK);
    for (int k = 0; k < NK; k++) {
        cx[k] = rng.uniform(-1.5, 1.5);
        const bool fixed = k >= n_local || k == id0;
        if (k < n_local) P.local_fixed.push_back(k == id0);
        for (int i = 0; i < 16; i++) P.Tcw.push_back(i % 5 == 0 ? 1.f : 0.f);
        P.Tcw[16 * k + 3] = (float)(-cx[k] + (fixed ? 0 : rng.normal() * 0.03));
        P.Tcw[16 * k + 7] = (float)(fixed ? 0 : rng.normal() * 0.03);
        const float c[5] = {718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f};
        P.cam.insert(P.cam.end(), c, c + 5);
    }
    P.off.push_back(0);
    for (int p = 0; p < n_points; p++) {
        double X[3] = {rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(6, 20)};
        X[0] *= X[2] / 20;
        for (int i = 0; i < 3; i++) P.xw.push_back((float)(X[i] + rng.normal() * 0.03));
        const int deg = NK < 2 ? NK : 2 + (int)(rng.uniform() * (NK - 1));
        const int first = (int)(rng.uniform() * NK);
        for (int d = 0; d < deg; d++) {
            const int k = (first + d) % NK;
            double u = 718.856 * (X[0] - cx[k]) / X[2] + 607.1928 + rng.normal() * 0.7, v = 718.856 * X[1] / X[2] + 185.2157 + rng.normal() * 0.7;
            double r = u - 386.1448 / X[2];
            if (rng.uniform() < outliers) { u += rng.uniform(30, 80); v -= rng.uniform(30, 80); }
            P.kf.push_back(k);
            P.obs.push_back((float)u); P.obs.push_back((float)v);
            P.ur.push_back(rng.uniform() < 0.5 || r < 0 ? -1.f : (float)r);
            P.inv.push_back((float)(1.0 / pow(1.2, 2 * (int)(rng.uniform() * 8))));
        }
        P.off.push_back((int32_t)P.kf.size());
    }
    return P;
}

static int run(const Problem &P, const uint8_t *stop, orbp_lba_stats *st, std::vector<float> *T_out = nullptr, std::vector<uint8_t> *erase_out = nullptr)
{
    const Arr<uint8_t> lf(P.local_fixed);
    const Arr<float> Tcw(P.Tcw), cam(P.cam), obs(P.obs), ur(P.ur), inv(P.inv);
    const Arr<int32_t> off(P.off), kf(P.kf);
    Arr<float> xw(P.xw), T(std::vector<float>(16 * (size_t)P.n_local, 7.25f));
    Arr<uint8_t> erase(std::vector<uint8_t>(P.kf.size(), 0x5A));
    const orbp_lba_problem flat = {P.n_local, P.n_fixed, P.n_points, lf.get(), Tcw.get(), cam.get(), off.get(), kf.get(), obs.get(), ur.get(), inv.get()};
    const int rc = orbp_local_bundle_adjustment(&flat, T.get(), xw.get(), erase.get(), stop, st);
    if (T_out) T_out->assign(T.get(), T.get() + T.n);
    if (erase_out) erase_out->assign(erase.get(), erase.get() + erase.n);
    return rc;
}

int main()
{
    orbp_lba_stats st;
    const int shapes[][4] = {{1, 2, 1, -1}, {2, 1, 64, -1}, {3, 0, 65, 2}, {11, 6, 257, -1}, {2, 1, 0, -1}, {1, 2, 30, 0}, {0, 0, 0, -1}};
    for (const auto &s : shapes) {
        const Problem P = make(s[0], s[1], s[2], s[3], 0.1, 11 + s[2]);
        std::vector<float> T;
        std::vector<uint8_t> erase;
        memset(&st, 0x5A, sizeof st);
        const int rc = run(P, nullptr, &st, &T, &erase);
        CHECK(rc == ORBP_LBA_DONE, "%d local, %d fixed, %d points: %d %s", s[0], s[1], s[2], rc, orbp_last_error());
        CHECK(st.iterations[0] >= 0 && st.iterations[0] <= 5 && st.iterations[1] <= 10 && st.trials[0] <= 50 && st.trials[1] <= 100, "stats");
        for (uint8_t e : erase) CHECK(e == 0 || e == 1, "erase flag %d", e);
        for (float v : T) CHECK(std::isfinite(v) && v != 7.25f, "pose entry %g", v);
        CHECK(run(P, nullptr, nullptr) == ORBP_LBA_DONE, "stats may be NULL");
        const uint8_t up = 1, down = 0;
        memset(&st, 0x5A, sizeof st);
        CHECK(run(P, &up, &st, &T, &erase) == ORBP_LBA_STOPPED, "stop at entry");
        for (float v : T) CHECK(v == 7.25f, "stop at entry wrote a pose");
        for (uint8_t e : erase) CHECK(e == 0x5A, "stop at entry wrote a flag");
        CHECK(((const uint8_t *)&st)[0] == 0x5A, "stop at entry wrote the stats");
        CHECK(run(P, &down, &st) == ORBP_LBA_DONE, "stop flag down");
    }
    {   // refused before any work
        Problem P = make(2, 1, 20, -1, 0.0, 5);
        Problem Q = P; Q.kf[3] = 3;
        CHECK(run(Q, nullptr, &st) == ORBX_E_INVALID, "key frame out of range");
        Q = P; Q.kf[1] = Q.kf[0];
        CHECK(run(Q, nullptr, &st) == ORBX_E_INVALID, "key frame twice");
        Q = P; Q.off[2] = Q.off[1] - 1;
        CHECK(run(Q, nullptr, &st) == ORBX_E_INVALID, "edge_off not monotone");
        Q = P; Q.Tcw[5] = NAN;
        CHECK(run(Q, nullptr, &st) == ORBX_E_INVALID, "pose not finite");
        Q = P; Q.xw[7] = INFINITY;
        CHECK(run(Q, nullptr, &st) == ORBX_E_INVALID, "point not finite");
        Q = P; Q.n_fixed = -1;
        CHECK(run(Q, nullptr, &st) == ORBX_E_INVALID, "negative count");
        CHECK(orbp_local_bundle_adjustment(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_E_INVALID, "NULL problem");
    }
    if (!failures) printf("lba_asan_main ok\n");
    return failures ? 1 : 0;
}
