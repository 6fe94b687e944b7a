// orbp_sim3.cc -- Sim3Solver (src/Sim3Solver.cc of WChen09/My-SLAM) behind include/orbp.h: the RANSAC state machine on the host,
// every hypothesis through orbm_sim3_body.h, the text the kernel of orbm_sim3.hip runs as well.  Plain C++, no device code.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbm_sim3_body.h"
#include "orbp_internal.h"

static int pfail(int code, const char *fmt, ...)
{
    char text[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    orbp_set_error(text);
    return code;
}

static int sim3_libc_rand(void *) { return rand(); }

struct orbp_sim3 {
    int N = 0;
    std::vector<float> x1, x2, e1, e2;         // mvX3Dc1 / mvX3Dc2, mvnMaxError1 / 2 (as floats)
    Sim3Cam K1, K2;
    bool fix_scale = false;
    double prob = 0.99; int min_inliers = 6, max_its = 300;
    float eps = 0;
    int n_iter = 0, n_best = 0;                 // mnIterations, mnBestInliers
    bool has_best = false;
    Sim3Hyp best;                               // mBestT12 / Rotation / Translation / Scale
    std::vector<uint8_t> inl_i, inl_best;       // mvbInliersi, mvbBestInliers
    int (*rnd)(void *) = sim3_libc_rand; void *rnd_ctx = nullptr; double rnd_max = RAND_MAX;
    // drawn, not yet consumed triples: queue[3 * head ..]; the first att_n of them have results (att_*, entry 0 = queue entry att_base)
    std::vector<int32_t> queue; size_t head = 0;
    size_t att_base = 0, att_n = 0;
    std::vector<int32_t> att_counts; std::vector<float> att_sRt; std::vector<uint32_t> att_masks;

    int words() const { return (N + 31) / 32; }
    size_t queued() const { return queue.size() / 3 - head; }
    int random_int(int lo, int hi)              // DUtils::Random::RandomInt, Random.cpp:47-50
    {
        const int d = hi - lo + 1;
        return int(((double)rnd(rnd_ctx) / (rnd_max + 1.0)) * d) + lo;
    }
    void draw_one(int32_t *tri)                 // :163-177
    {
        std::vector<int> avail(N);
        for (int i = 0; i < N; i++) avail[i] = i;
        for (int i = 0; i < 3; ++i) {
            const int r = random_int(0, (int)avail.size() - 1);
            tri[i] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    void from_triple(const int32_t *tri, Sim3Hyp &h) const
    {
        float P1[3][3], P2[3][3];
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < 3; i++) { P1[k][i] = x1[3 * (size_t)tri[k] + i]; P2[k][i] = x2[3 * (size_t)tri[k] + i]; }
        sim3_from_triple(P1, P2, fix_scale, h);
    }
    int check_inliers(const Sim3Hyp &h, uint8_t *inl) const
    {
        int n = 0;
        for (int i = 0; i < N; i++) {
            inl[i] = sim3_check_one(h, &x1[3 * (size_t)i], &x2[3 * (size_t)i], K1, K2, e1[i], e2[i]);
            n += inl[i];
        }
        return n;
    }
    void clear_queue() { queue.clear(); head = 0; att_base = att_n = 0; att_counts.clear(); att_sRt.clear(); att_masks.clear(); }
};

extern "C" int orbp_sim3_set_ransac_parameters(orbp_sim3 *s, double probability, int min_inliers, int max_iterations)
{
    if (!s) return pfail(ORBX_E_INVALID, "solver is NULL");
    s->prob = probability; s->min_inliers = min_inliers; s->max_its = max_iterations;
    const int N = s->N;
    s->eps = (float)s->min_inliers / N;
    int nit;
    if (s->min_inliers >= N) nit = 1;           // == N: :130-131; > N: defined here (orbp.h)
    else {
        // an infinite / out-of-range quotient converts as x86's cvttsd2si does in the reference build: INT_MIN, clamped to 1 below
        const double v = std::ceil(std::log(1 - s->prob) / std::log(1 - std::pow((double)s->eps, 3)));
        nit = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT_MIN;
    }
    s->max_its = std::max(1, std::min(nit, s->max_its));
    s->n_iter = 0;
    s->clear_queue();
    return 0;
}

extern "C" int orbp_sim3_create(orbp_sim3 **out, int n, const float *x3dc1, const float *x3dc2, const float *sigma2_1,
                                const float *sigma2_2, const float *K1, const float *K2, int fix_scale)
{
    if (!out) return pfail(ORBX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 0 || !K1 || !K2 || (n > 0 && (!x3dc1 || !x3dc2 || !sigma2_1 || !sigma2_2))) return pfail(ORBX_E_INVALID, "bad correspondences");
    orbp_sim3 *s = new orbp_sim3();
    s->N = n;
    if (n) { s->x1.assign(x3dc1, x3dc1 + 3 * (size_t)n); s->x2.assign(x3dc2, x3dc2 + 3 * (size_t)n); }
    s->e1.resize(n); s->e2.resize(n);
    for (int i = 0; i < n; i++) { s->e1[i] = sim3_max_error(sigma2_1[i]); s->e2[i] = sim3_max_error(sigma2_2[i]); }
    s->K1 = {K1[0], K1[1], K1[2], K1[3]}; s->K2 = {K2[0], K2[1], K2[2], K2[3]};
    s->fix_scale = fix_scale != 0;
    s->inl_i.assign(n, 0); s->inl_best.assign(n, 0);
    memset(&s->best, 0, sizeof s->best);
    orbp_sim3_set_ransac_parameters(s, 0.99, 6, 300);       // the constructor's SetRansacParameters() (:111)
    *out = s;
    return 0;
}

extern "C" void orbp_sim3_destroy(orbp_sim3 *s) { delete s; }

extern "C" void orbp_sim3_set_rand(orbp_sim3 *s, int (*fn)(void *), void *ctx, int rand_max)
{
    if (!s) return;
    if (fn) { s->rnd = fn; s->rnd_ctx = ctx; s->rnd_max = rand_max; }
    else { s->rnd = sim3_libc_rand; s->rnd_ctx = nullptr; s->rnd_max = RAND_MAX; }
}

extern "C" void orbp_sim3_get_ransac_state(const orbp_sim3 *s, int *min_inliers, int *max_its, float *epsilon, int *iterations_done,
                                           int *best_inliers)
{
    if (!s) return;
    if (min_inliers) *min_inliers = s->min_inliers;
    if (max_its) *max_its = s->max_its;
    if (epsilon) *epsilon = s->eps;
    if (iterations_done) *iterations_done = s->n_iter;
    if (best_inliers) *best_inliers = s->n_best;
}

extern "C" int orbp_sim3_get_problem(const orbp_sim3 *s, float *x3dc1, float *x3dc2, float *max_err1, float *max_err2, float *K1, float *K2,
                                     int32_t *fix_scale)
{
    if (!s || !K1 || !K2 || !fix_scale || (s->N > 0 && (!x3dc1 || !x3dc2 || !max_err1 || !max_err2))) return pfail(ORBX_E_INVALID, "NULL argument");
    if (s->N) {
        memcpy(x3dc1, s->x1.data(), sizeof(float) * 3 * s->N); memcpy(x3dc2, s->x2.data(), sizeof(float) * 3 * s->N);
        memcpy(max_err1, s->e1.data(), sizeof(float) * s->N); memcpy(max_err2, s->e2.data(), sizeof(float) * s->N);
    }
    const float k1[4] = {s->K1.fx, s->K1.fy, s->K1.cx, s->K1.cy}, k2[4] = {s->K2.fx, s->K2.fy, s->K2.cx, s->K2.cy};
    memcpy(K1, k1, sizeof k1); memcpy(K2, k2, sizeof k2);
    *fix_scale = s->fix_scale ? 1 : 0;
    return s->N;
}

extern "C" int orbp_sim3_draw(orbp_sim3 *s, int n_iterations, int32_t *triples)
{
    if (!s || n_iterations < 0) return pfail(ORBX_E_INVALID, "bad arguments");
    if (s->N < s->min_inliers || s->N < 3) return 0;
    const long long left = (long long)s->max_its - s->n_iter - (long long)s->queued();
    const int n = (int)std::max(0ll, std::min<long long>(n_iterations, left));
    for (int k = 0; k < n; k++) {
        int32_t tri[3];
        s->draw_one(tri);
        s->queue.insert(s->queue.end(), tri, tri + 3);
        if (triples) memcpy(triples + 3 * (size_t)k, tri, sizeof tri);
    }
    return n;
}

extern "C" int orbp_sim3_queued(const orbp_sim3 *s, int32_t *triples)
{
    if (!s) return pfail(ORBX_E_INVALID, "solver is NULL");
    const size_t n = s->queued();
    if (triples && n) memcpy(triples, s->queue.data() + 3 * s->head, n * 3 * sizeof(int32_t));
    return (int)n;
}

extern "C" int orbp_sim3_hypothesis(const orbp_sim3 *s, const int32_t *triple, float *R, float *t, float *scale, uint8_t *inliers,
                                    int *n_inliers)
{
    if (!s || !triple || !R || !t || !scale || !n_inliers || (s->N > 0 && !inliers)) return pfail(ORBX_E_INVALID, "NULL argument");
    for (int k = 0; k < 3; k++)
        if (triple[k] < 0 || triple[k] >= s->N) return pfail(ORBX_E_INVALID, "triple index %d outside [0, %d)", triple[k], s->N);
    Sim3Hyp h;
    s->from_triple(triple, h);
    memcpy(R, h.R, sizeof h.R); memcpy(t, h.t, sizeof h.t); *scale = h.s;
    *n_inliers = s->check_inliers(h, inliers);
    return 0;
}

extern "C" int orbp_sim3_attach_results(orbp_sim3 *s, int n_hyp, const int32_t *counts, const float *sRt, const uint32_t *masks)
{
    if (!s || n_hyp < 0) return pfail(ORBX_E_INVALID, "bad arguments");
    if ((size_t)n_hyp != s->queued()) return pfail(ORBX_E_INVALID, "%d results for %zu queued triples", n_hyp, s->queued());
    if (n_hyp > 0 && (!counts || !sRt || !masks)) return pfail(ORBX_E_INVALID, "NULL argument");
    const size_t W = (size_t)s->words();
    s->att_base = s->head; s->att_n = (size_t)n_hyp;
    s->att_counts.assign(counts, counts + n_hyp);
    s->att_sRt.assign(sRt, sRt + 13 * (size_t)n_hyp);
    s->att_masks.assign(masks, masks + W * (size_t)n_hyp);
    return 0;
}

static void sim3_fill_T(const Sim3Hyp &h, float *T)
{
    memcpy(T, h.T12, sizeof h.T12);
    T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
}

extern "C" int orbp_sim3_iterate(orbp_sim3 *s, int n_iterations, int *no_more, uint8_t *inliers, int *n_inliers, float *T12)
{
    if (!s || !no_more || !n_inliers || !T12 || (s->N > 0 && !inliers)) return pfail(ORBX_E_INVALID, "NULL argument");
    const int N = s->N;
    *no_more = 0; *n_inliers = 0;               // :142-144
    for (int i = 0; i < N; i++) inliers[i] = 0;
    if (N < s->min_inliers || N < 3) { *no_more = 1; return 0; }
    int cur = 0;
    const size_t W = (size_t)s->words();
    while (s->n_iter < s->max_its && cur < n_iterations) {
        cur++; s->n_iter++;
        int32_t tri[3];
        Sim3Hyp h;
        int n_i;
        if (s->queued()) {
            const size_t at = s->head++;
            memcpy(tri, &s->queue[3 * at], sizeof tri);
            if (at >= s->att_base && at - s->att_base < s->att_n) {      // replay
                const size_t k = at - s->att_base;
                const float *r = &s->att_sRt[13 * k];
                h.s = r[0]; memcpy(h.R, r + 1, sizeof h.R); memcpy(h.t, r + 10, sizeof h.t);
                sim3_transforms(h);
                const uint32_t *mk = &s->att_masks[W * k];
                for (int i = 0; i < N; i++) s->inl_i[i] = (mk[i >> 5] >> (i & 31)) & 1u;
                n_i = s->att_counts[k];
            } else {
                s->from_triple(tri, h);
                n_i = s->check_inliers(h, s->inl_i.data());
            }
            if (!s->queued()) s->clear_queue();
        } else {
            s->draw_one(tri);
            s->from_triple(tri, h);
            n_i = s->check_inliers(h, s->inl_i.data());
        }
        if (n_i >= s->n_best) {                 // :183-200
            s->inl_best = s->inl_i;
            s->n_best = n_i;
            s->best = h;
            s->has_best = true;
            if (n_i > s->min_inliers) {
                *n_inliers = n_i;
                memcpy(inliers, s->inl_i.data(), N);
                sim3_fill_T(h, T12);
                if (s->n_iter >= s->max_its) *no_more = 1;
                return 1;
            }
        }
    }
    if (s->n_iter >= s->max_its) *no_more = 1;
    return 0;
}

extern "C" int orbp_sim3_find(orbp_sim3 *s, uint8_t *inliers, int *n_inliers, float *T12)
{
    int flag = 0;
    if (!s) return pfail(ORBX_E_INVALID, "solver is NULL");
    return orbp_sim3_iterate(s, s->max_its, &flag, inliers, n_inliers, T12);
}

extern "C" int orbp_sim3_get_estimated(const orbp_sim3 *s, float *R, float *t, float *scale)
{
    if (!s || !R || !t || !scale) return pfail(ORBX_E_INVALID, "NULL argument");
    if (!s->has_best) return 0;
    memcpy(R, s->best.R, sizeof s->best.R); memcpy(t, s->best.t, sizeof s->best.t); *scale = s->best.s;
    return 1;
}

extern "C" double orbp_sim3_math(int fn, double a, double b)
{
    double sn = 0, cs = 0;
    if (fn == 0) return sim3_atan2_pos(a, b);
    sim3_sincos(a, sn, cs);
    return fn == 1 ? sn : cs;
}
