// orbp.cc -- the host-side PnP solver behind include/orbp.h (EPnP RANSAC) and the error text of all of orbp.h.
// Plain C++, fp64, no device code.  Each function names the reference lines it follows; the linear algebra the reference borrows
// from OpenCV / Eigen is written here.  One EPnP hypothesis (csrc/orbp_epnp_body.h) is shared with the kernel of orbm_pnp.hip, which
// evaluates the hypotheses of all Relocalization candidates at once; the RANSAC state machine and Refine stay here.  The motion-only
// pose optimisation is orbp_pose.cc.
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
#include "orbp_epnp_body.h"
#include "orbp_internal.h"

static thread_local char g_perr[256] = "";
static int pfail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_perr, sizeof g_perr, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *orbp_last_error(void) { return g_perr; }
void orbp_set_error(const char *text) { snprintf(g_perr, sizeof g_perr, "%s", text); }

// -------------------------------------------------------------------------------------------------
// EPnP (PnPsolver.cc:346-957): the arithmetic is csrc/orbp_epnp_body.h, the text the kernel of orbm_pnp.hip runs as well.
// This wrapper owns the per-point arrays of an n-point solve (Refine, orbp_epnp); a RANSAC sample uses the same path.
// -------------------------------------------------------------------------------------------------
namespace {
struct Epnp {
    double fu, fv, uc, vc;
    int n = 0;
    std::vector<double> pws, us, alphas, pcs;

    void reset() { n = 0; pws.clear(); us.clear(); }
    void add(double X, double Y, double Z, double u, double v)
    {
        pws.push_back(X); pws.push_back(Y); pws.push_back(Z);
        us.push_back(u); us.push_back(v);
        n++;
    }
    double compute_pose(double R[3][3], double t[3])       // :458-508
    {
        alphas.resize((size_t)4 * n);
        pcs.resize((size_t)3 * n);
        EpnpProblem p;
        p.fu = fu; p.fv = fv; p.uc = uc; p.vc = vc; p.n = n;
        p.pws = pws.data(); p.us = us.data(); p.alphas = alphas.data(); p.pcs = pcs.data();
        EpnpWork wk;
        return epnp_compute_pose(p, wk, &R[0][0], t);
    }
};
}   // namespace

extern "C" double orbp_epnp(int n, const double *pws, const double *us, double fu, double fv, double uc, double vc,
                            double *R, double *t)
{
    if (n < 4 || !pws || !us || !R || !t) { pfail(ORBX_E_INVALID, "orbp_epnp: n >= 4 and non-NULL buffers"); return -1.0; }
    Epnp e;
    e.fu = fu; e.fv = fv; e.uc = uc; e.vc = vc;
    for (int i = 0; i < n; i++) e.add(pws[3 * i], pws[3 * i + 1], pws[3 * i + 2], us[2 * i], us[2 * i + 1]);
    double Rm[3][3];
    const double err = e.compute_pose(Rm, t);
    memcpy(R, Rm, sizeof Rm);
    return err;
}

// -------------------------------------------------------------------------------------------------
// RANSAC driver (PnPsolver.cc:66-344)
// -------------------------------------------------------------------------------------------------
static int libc_rand(void *) { return rand(); }

struct orbp_pnp {
    Epnp e;
    int N = 0;
    std::vector<float> p2d, sigma2, p3d, max_error;
    std::vector<uint8_t> inl_i, inl_best, inl_refined;
    double Ri[3][3], ti[3];
    double prob = 0.99; int min_inliers = 8, max_its = 300, min_set = 4; float eps = 0.4f;
    int n_inl_i = 0, n_iter = 0, n_best = 0, n_refined = 0;
    float best_T[16], refined_T[16];
    int (*rnd)(void *) = libc_rand; void *rnd_ctx = nullptr; double rnd_max = RAND_MAX;

    int random_int(int lo, int hi)            // DUtils::Random::RandomInt, Random.cpp:47-50
    {
        const int d = hi - lo + 1;
        return int(((double)rnd(rnd_ctx) / (rnd_max + 1.0)) * d) + lo;
    }
    void pose_to_T(float *T) const            // :206-212
    {
        for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.f : 0.f;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T[4 * i + j] = (float)Ri[i][j];
            T[4 * i + 3] = (float)ti[i];
        }
    }
    // drawn, not yet consumed samples: queue[min_set * head ..]; att_n of them, from queue entry att_base on, have results
    std::vector<int32_t> queue; size_t head = 0;
    size_t att_base = 0, att_n = 0;
    std::vector<int32_t> att_counts; std::vector<double> att_Rt; std::vector<uint32_t> att_masks;

    int words() const { return (N + 31) / 32; }
    size_t queued() const { return queue.size() / (size_t)min_set - head; }
    void clear_queue() { queue.clear(); head = 0; att_base = att_n = 0; att_counts.clear(); att_Rt.clear(); att_masks.clear(); }
    void draw_one(int32_t *idx)               // draw without replacement (:193-204)
    {
        std::vector<int> avail(N);
        for (int i = 0; i < N; i++) avail[i] = i;
        for (int i = 0; i < min_set; ++i) {
            const int r = random_int(0, (int)avail.size() - 1);
            idx[i] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    void check_inliers()                      // :312-344, with its float/double mix
    {
        n_inl_i = 0;
        for (int i = 0; i < N; i++) {
            inl_i[i] = epnp_check_one(&Ri[0][0], ti, e.fu, e.fv, e.uc, e.vc, &p3d[3 * (size_t)i], &p2d[2 * (size_t)i], max_error[i]);
            n_inl_i += inl_i[i];
        }
    }
    void add_corr(int idx) { e.add(p3d[3 * idx], p3d[3 * idx + 1], p3d[3 * idx + 2], p2d[2 * idx], p2d[2 * idx + 1]); }
    void evaluate(const int32_t *idx)         // compute_pose on the sample + CheckInliers -> Ri, ti, inl_i, n_inl_i (:206-210)
    {
        e.reset();
        for (int i = 0; i < min_set; i++) add_corr(idx[i]);
        e.compute_pose(Ri, ti);
        check_inliers();
    }
    bool refine()                             // :260-309
    {
        e.reset();
        for (int i = 0; i < N; i++)
            if (inl_best[i]) add_corr(i);
        e.compute_pose(Ri, ti);
        check_inliers();
        n_refined = n_inl_i;
        inl_refined = inl_i;
        if (n_inl_i > min_inliers) { pose_to_T(refined_T); return true; }
        return false;
    }
};

extern "C" int orbp_pnp_set_ransac_parameters(orbp_pnp *s, double probability, int min_inliers, int max_iterations,
                                              int min_set, float epsilon, float th2)
{
    if (!s) return pfail(ORBX_E_INVALID, "solver is NULL");
    if (min_set < 4) return pfail(ORBX_E_INVALID, "min_set %d < 4: EPnP needs four points", min_set);
    s->clear_queue();                          // samples drawn ahead belong to the old parameters
    s->prob = probability; s->min_inliers = min_inliers; s->max_its = max_iterations; s->eps = epsilon; s->min_set = min_set;
    const int N = s->N;                        // :128-157
    int nmin = (int)(N * s->eps);
    if (nmin < s->min_inliers) nmin = s->min_inliers;
    if (nmin < min_set) nmin = min_set;
    s->min_inliers = nmin;
    if (s->eps < (float)s->min_inliers / N) s->eps = (float)s->min_inliers / N;
    int nit;
    if (s->min_inliers == N) nit = 1;
    else {
        // double -> int of a NaN / infinite / out-of-range quotient (epsilon > 1 when N < minInliers, epsilon ~ 0) is what
        // x86's cvttsd2si makes of it in the reference build: INT_MIN, which the clamp below turns into one iteration
        const double v = std::ceil(std::log(1 - s->prob) / std::log(1 - std::pow((double)s->eps, 3)));
        nit = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT_MIN;
    }
    s->max_its = std::max(1, std::min(nit, s->max_its));
    for (int i = 0; i < N; i++) s->max_error[i] = s->sigma2[i] * th2;
    return 0;
}

extern "C" int orbp_pnp_create(orbp_pnp **out, int n, const float *p2d, const float *sigma2, const float *p3d,
                               float fx, float fy, float cx, float cy)
{
    if (!out) return pfail(ORBX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 0 || (n > 0 && (!p2d || !sigma2 || !p3d))) return pfail(ORBX_E_INVALID, "bad correspondences");
    orbp_pnp *s = new orbp_pnp();
    s->N = n;
    s->p2d.assign(p2d, p2d + 2 * (size_t)n); s->sigma2.assign(sigma2, sigma2 + n); s->p3d.assign(p3d, p3d + 3 * (size_t)n);
    s->max_error.resize(n); s->inl_i.assign(n, 0); s->inl_best.assign(n, 0); s->inl_refined.assign(n, 0);
    s->e.fu = fx; s->e.fv = fy; s->e.uc = cx; s->e.vc = cy;
    orbp_pnp_set_ransac_parameters(s, 0.99, 8, 300, 4, 0.4f, 5.991f);     // the constructor's SetRansacParameters() (:108)
    *out = s;
    return 0;
}

extern "C" void orbp_pnp_destroy(orbp_pnp *s) { delete s; }

extern "C" void orbp_pnp_set_rand(orbp_pnp *s, int (*fn)(void *), void *ctx, int rand_max)
{
    if (!s) return;
    if (fn) { s->rnd = fn; s->rnd_ctx = ctx; s->rnd_max = rand_max; }
    else { s->rnd = libc_rand; s->rnd_ctx = nullptr; s->rnd_max = RAND_MAX; }
}

extern "C" void orbp_pnp_get_ransac_state(const orbp_pnp *s, int *min_inliers, int *max_its, float *epsilon, int *iterations_done)
{
    if (!s) return;
    if (min_inliers) *min_inliers = s->min_inliers;
    if (max_its) *max_its = s->max_its;
    if (epsilon) *epsilon = s->eps;
    if (iterations_done) *iterations_done = s->n_iter;
}

extern "C" int orbp_pnp_iterate(orbp_pnp *s, int n_iterations, int *no_more, uint8_t *inliers, int *n_inliers, float *Tcw)
{
    if (!s || !no_more || !inliers || !n_inliers || !Tcw) return pfail(ORBX_E_INVALID, "NULL argument");
    *no_more = 0; *n_inliers = 0;              // :168-170
    const int N = s->N;
    if (N < s->min_inliers) { *no_more = 1; return 0; }
    std::vector<int32_t> idx(s->min_set);
    const size_t W = (size_t)s->words();
    int cur = 0;
    while (s->n_iter < s->max_its || cur < n_iterations) {
        cur++; s->n_iter++;
        if (s->queued()) {                             // a sample drawn ahead (orbp_pnp_draw): the oldest first
            const size_t at = s->head++;
            if (at >= s->att_base && at - s->att_base < s->att_n) {      // with results: mRi, mti, mvbInliersi, mnInliersi restored
                const size_t k = at - s->att_base;
                memcpy(s->Ri, &s->att_Rt[12 * k], sizeof s->Ri);
                memcpy(s->ti, &s->att_Rt[12 * k + 9], sizeof s->ti);
                const uint32_t *mk = &s->att_masks[W * k];
                for (int i = 0; i < N; i++) s->inl_i[i] = (mk[i >> 5] >> (i & 31)) & 1u;
                s->n_inl_i = s->att_counts[k];
            } else {
                memcpy(idx.data(), &s->queue[(size_t)s->min_set * at], sizeof(int32_t) * s->min_set);
                s->evaluate(idx.data());
            }
            if (!s->queued()) s->clear_queue();
        } else {
            s->draw_one(idx.data());
            s->evaluate(idx.data());
        }
        if (s->n_inl_i >= s->min_inliers) {
            if (s->n_inl_i > s->n_best) {
                s->inl_best = s->inl_i;
                s->n_best = s->n_inl_i;
                s->pose_to_T(s->best_T);
            }
            if (s->refine()) {                         // note: refines on the best set so far, not on this draw's
                *n_inliers = s->n_refined;
                memcpy(inliers, s->inl_refined.data(), N);
                memcpy(Tcw, s->refined_T, sizeof(float) * 16);
                return 1;
            }
        }
    }
    if (s->n_iter >= s->max_its) {
        *no_more = 1;
        if (s->n_best >= s->min_inliers) {
            *n_inliers = s->n_best;
            memcpy(inliers, s->inl_best.data(), N);
            memcpy(Tcw, s->best_T, sizeof(float) * 16);
            return 1;
        }
    }
    return 0;
}

extern "C" int orbp_pnp_get_problem(const orbp_pnp *s, float *p2d, float *p3d, float *max_err, float *K, int32_t *min_set)
{
    if (!s || !K || !min_set || (s->N > 0 && (!p2d || !p3d || !max_err))) return pfail(ORBX_E_INVALID, "NULL argument");
    if (s->N) {
        memcpy(p2d, s->p2d.data(), sizeof(float) * 2 * s->N); memcpy(p3d, s->p3d.data(), sizeof(float) * 3 * s->N);
        memcpy(max_err, s->max_error.data(), sizeof(float) * s->N);
    }
    K[0] = (float)s->e.fu; K[1] = (float)s->e.fv; K[2] = (float)s->e.uc; K[3] = (float)s->e.vc;      // they came in as floats
    *min_set = s->min_set;
    return s->N;
}

extern "C" int orbp_pnp_draw(orbp_pnp *s, int n_iterations, int32_t *samples)
{
    if (!s || n_iterations < 0) return pfail(ORBX_E_INVALID, "bad arguments");
    if (s->N < s->min_inliers) return 0;
    // iterate's loop is `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` (:182)
    // so iterate(n_iterations) consumes max(max_its - iterations_done, n_iterations) sets unless a pose comes back earlier
    const long long consumes = std::max<long long>((long long)s->max_its - s->n_iter, n_iterations);
    const int n = (int)std::max<long long>(consumes - (long long)s->queued(), 0);
    for (int k = 0; k < n; k++) {
        const size_t at = s->queue.size();
        s->queue.resize(at + s->min_set);
        s->draw_one(&s->queue[at]);
        if (samples) memcpy(samples + (size_t)s->min_set * k, &s->queue[at], sizeof(int32_t) * s->min_set);
    }
    return n;
}

extern "C" int orbp_pnp_queued(const orbp_pnp *s, int32_t *samples)
{
    if (!s) return pfail(ORBX_E_INVALID, "solver is NULL");
    const size_t n = s->queued();
    if (samples && n) memcpy(samples, s->queue.data() + (size_t)s->min_set * s->head, n * s->min_set * sizeof(int32_t));
    return (int)n;
}

extern "C" int orbp_pnp_hypothesis(const orbp_pnp *s, const int32_t *sample, double *R, double *t, uint8_t *inliers, int *n_inliers)
{
    if (!s || !sample || !R || !t || !n_inliers || (s->N > 0 && !inliers)) return pfail(ORBX_E_INVALID, "NULL argument");
    for (int k = 0; k < s->min_set; k++) {
        if (sample[k] < 0 || sample[k] >= s->N) return pfail(ORBX_E_INVALID, "sample index %d outside [0, %d)", sample[k], s->N);
        for (int j = 0; j < k; j++)
            if (sample[j] == sample[k]) return pfail(ORBX_E_INVALID, "sample index %d repeated", sample[k]);
    }
    Epnp e;
    e.fu = s->e.fu; e.fv = s->e.fv; e.uc = s->e.uc; e.vc = s->e.vc;
    for (int k = 0; k < s->min_set; k++) {
        const size_t i = (size_t)sample[k];
        e.add(s->p3d[3 * i], s->p3d[3 * i + 1], s->p3d[3 * i + 2], s->p2d[2 * i], s->p2d[2 * i + 1]);
    }
    double Rm[3][3];
    e.compute_pose(Rm, t);
    memcpy(R, Rm, sizeof Rm);
    int n = 0;
    for (int i = 0; i < s->N; i++) {
        inliers[i] = epnp_check_one(R, t, e.fu, e.fv, e.uc, e.vc, &s->p3d[3 * (size_t)i], &s->p2d[2 * (size_t)i], s->max_error[i]);
        n += inliers[i];
    }
    *n_inliers = n;
    return 0;
}

extern "C" int orbp_pnp_attach_results(orbp_pnp *s, int n_hyp, const int32_t *counts, const double *Rt, const uint32_t *masks)
{
    if (!s || n_hyp < 0) return pfail(ORBX_E_INVALID, "bad arguments");
    if ((size_t)n_hyp != s->queued()) return pfail(ORBX_E_INVALID, "%d results for %zu queued samples", n_hyp, s->queued());
    if (n_hyp > 0 && (!counts || !Rt || !masks)) return pfail(ORBX_E_INVALID, "NULL argument");
    const size_t W = (size_t)s->words();
    s->att_base = s->head; s->att_n = (size_t)n_hyp;
    s->att_counts.assign(counts, counts + n_hyp);
    s->att_Rt.assign(Rt, Rt + 12 * (size_t)n_hyp);
    s->att_masks.assign(masks, masks + W * (size_t)n_hyp);
    return 0;
}

extern "C" int orbp_pnp_find(orbp_pnp *s, uint8_t *inliers, int *n_inliers, float *Tcw)
{
    int flag = 0;
    if (!s) return pfail(ORBX_E_INVALID, "solver is NULL");
    return orbp_pnp_iterate(s, s->max_its, &flag, inliers, n_inliers, Tcw);
}
