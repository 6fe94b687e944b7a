// orbp.cc -- host-side pose solvers behind include/orbp.h (EPnP RANSAC + motion-only pose optimisation).
// Plain C++, fp64, no device code.  Each function names the reference lines it follows; the linear algebra the reference borrows
// from OpenCV / Eigen is written here.  One EPnP hypothesis (csrc/orbp_epnp_body.h) is shared with the kernel of orbm_pnp.hip, which
// evaluates the hypotheses of all Relocalization candidates at once; the RANSAC state machine, Refine and PoseOptimization stay here.
#include <algorithm>
#include <cfloat>
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

// -------------------------------------------------------------------------------------------------
// Motion-only pose optimisation (Optimizer.cc:239-451 on g2o)
// -------------------------------------------------------------------------------------------------
namespace {
struct Quat { double w, x, y, z; };
struct Se3 { Quat r; double t[3]; };

static Quat quat_from_R(const double R[9])    // Eigen's Quaterniond(Matrix3d) (Shepperd), as g2o::SE3Quat(R, t) uses
{
    Quat q;
    double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        tr = std::sqrt(tr + 1.0);
        q.w = 0.5 * tr;
        tr = 0.5 / tr;
        q.x = (R[7] - R[5]) * tr; q.y = (R[2] - R[6]) * tr; q.z = (R[3] - R[1]) * tr;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double v[3];
        tr = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        v[i] = 0.5 * tr;
        tr = 0.5 / tr;
        q.w = (R[3 * k + j] - R[3 * j + k]) * tr;
        v[j] = (R[3 * j + i] + R[3 * i + j]) * tr;
        v[k] = (R[3 * k + i] + R[3 * i + k]) * tr;
        q.x = v[0]; q.y = v[1]; q.z = v[2];
    }
    return q;
}
static void quat_normalize(Quat &q)           // se3quat.h:280-285
{
    if (q.w < 0) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
    const double n = std::sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    q.w /= n; q.x /= n; q.y /= n; q.z /= n;
}
static Quat quat_mul(const Quat &a, const Quat &b)
{
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
static void quat_rotate(const Quat &q, const double v[3], double out[3])      // Eigen: v + w uv + q.vec x uv, uv = 2 q.vec x v
{
    double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    out[0] = v[0] + q.w * uv[0] + (q.y * uv[2] - q.z * uv[1]);
    out[1] = v[1] + q.w * uv[1] + (q.z * uv[0] - q.x * uv[2]);
    out[2] = v[2] + q.w * uv[2] + (q.x * uv[1] - q.y * uv[0]);
}
static void quat_to_R(const Quat &q, double R[9])
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
static void se3_map(const Se3 &T, const double x[3], double out[3])
{
    quat_rotate(T.r, x, out);
    out[0] += T.t[0]; out[1] += T.t[1]; out[2] += T.t[2];
}
static Se3 se3_exp(const double u[6])          // se3quat.h:223-257 (omega first, then upsilon)
{
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double theta = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0) + O[i] + O2[i]; V[i] = R[i]; }
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
        const double c = (theta - std::sin(theta)) / std::pow(theta, 3);
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0) + a * O[i] + b * O2[i]; V[i] = (i % 4 == 0) + b * O[i] + c * O2[i]; }
    }
    Se3 T;
    T.r = quat_from_R(R);
    quat_normalize(T.r);
    for (int i = 0; i < 3; i++) T.t[i] = V[3 * i] * up[0] + V[3 * i + 1] * up[1] + V[3 * i + 2] * up[2];
    return T;
}
static Se3 se3_mul(const Se3 &a, const Se3 &b)  // se3quat.h:104-110
{
    Se3 r = a;
    double rt[3];
    quat_rotate(a.r, b.t, rt);
    r.t[0] += rt[0]; r.t[1] += rt[1]; r.t[2] += rt[2];
    r.r = quat_mul(a.r, b.r);
    quat_normalize(r.r);
    return r;
}

// 6x6 symmetric positive definite solve (the reference: Eigen LDLT inside g2o::LinearSolverDense)
static bool ldlt_solve6(const double H[36], const double b[6], double x[6])
{
    double L[36] = {0}, D[6];
    for (int j = 0; j < 6; j++) {
        double d = H[6 * j + j];
        for (int k = 0; k < j; k++) d -= L[6 * j + k] * L[6 * j + k] * D[k];
        if (!(std::fabs(d) > 0) || !std::isfinite(d)) return false;
        D[j] = d;
        L[6 * j + j] = 1;
        for (int i = j + 1; i < 6; i++) {
            double s = H[6 * i + j];
            for (int k = 0; k < j; k++) s -= L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = s / d;
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) { double s = b[i]; for (int k = 0; k < i; k++) s -= L[6 * i + k] * y[k]; y[i] = s; }
    for (int i = 0; i < 6; i++) y[i] /= D[i];
    for (int i = 5; i >= 0; i--) { double s = y[i]; for (int k = i + 1; k < 6; k++) s -= L[6 * k + i] * x[k]; x[i] = s; }
    return true;
}

struct Edge {
    int idx; bool stereo;
    double obs[3], xw[3], info;
    double err[3];         // _error: refreshed only where g2o refreshes it
    double pc[3];          // the point in the camera frame at the estimate compute_error last saw
    bool robust; int level;
};

struct PoseProblem {
    double fx, fy, cx, cy, bf;
    std::vector<Edge> edges;
    std::vector<int> active;
    Se3 est;
    double delta_mono, delta_stereo;

    void compute_error(Edge &e) const         // types_six_dof_expmap.h:153-157,184-188; .cpp:290-306
    {
        double *p = e.pc;
        se3_map(est, e.xw, p);
        if (!e.stereo) {
            e.err[0] = e.obs[0] - (p[0] / p[2] * fx + cx);
            e.err[1] = e.obs[1] - (p[1] / p[2] * fy + cy);
            e.err[2] = 0;
        } else {
            const float invz = 1.0f / (float)p[2];
            const double u = p[0] * invz * fx + cx;
            e.err[0] = e.obs[0] - u;
            e.err[1] = e.obs[1] - (p[1] * invz * fy + cy);
            e.err[2] = e.obs[2] - (u - bf * invz);
        }
    }
    static double chi2(const Edge &e) { return (e.err[0] * e.err[0] + e.err[1] * e.err[1] + e.err[2] * e.err[2]) * e.info; }
    void huber(const Edge &e, double c2, double rho[2]) const      // robust_kernel_impl.cpp:78-91
    {
        const double delta = e.stereo ? delta_stereo : delta_mono, dsqr = delta * delta;
        if (c2 <= dsqr) { rho[0] = c2; rho[1] = 1.; }
        else { const double s = std::sqrt(c2); rho[0] = 2 * s * delta - dsqr; rho[1] = delta / s; }
    }
    void compute_active_errors() { for (int k : active) compute_error(edges[k]); }
    double active_robust_chi2() const
    {
        double sum = 0;
        for (int k : active) {
            const Edge &e = edges[k];
            const double c2 = chi2(e);
            if (e.robust) { double rho[2]; huber(e, c2, rho); sum += rho[0]; }
            else sum += c2;
        }
        return sum;
    }
    // linearizeOplus (.cpp:266-288,335-364) + constructQuadraticForm (base_unary_edge.hpp:43-72).  Called right after
    // compute_active_errors() at the same estimate, so the camera-frame points cached there are the ones g2o maps again.
    void build_system(double H[36], double b[6]) const
    {
        double Hu[21] = {0};
        for (int i = 0; i < 6; i++) b[i] = 0;
        for (int k : active) {
            const Edge &e = edges[k];
            const double x = e.pc[0], y = e.pc[1], invz = 1.0 / e.pc[2], invz_2 = invz * invz;
            double J[3][6];
            J[0][0] = x * y * invz_2 * fx; J[0][1] = -(1 + (x * x * invz_2)) * fx; J[0][2] = y * invz * fx;
            J[0][3] = -invz * fx; J[0][4] = 0; J[0][5] = x * invz_2 * fx;
            J[1][0] = (1 + y * y * invz_2) * fy; J[1][1] = -x * y * invz_2 * fy; J[1][2] = -x * invz * fy;
            J[1][3] = 0; J[1][4] = -invz * fy; J[1][5] = y * invz_2 * fy;
            if (e.stereo) {
                J[2][0] = J[0][0] - bf * y * invz_2; J[2][1] = J[0][1] + bf * x * invz_2; J[2][2] = J[0][2];
                J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - bf * invz_2;
            }
            double w = 1.0;
            if (e.robust) { double rho[2]; huber(e, chi2(e), rho); w = rho[1]; }
            const double wi = w * e.info;
            // b -= rho' J^T Omega e and H += J^T (rho' Omega) J, upper triangle; written out per row count so the
            // compiler sees fixed trip counts (the sums keep the order 0 + row0 + row1 (+ row2))
            double wJ[3][6];
            for (int r = 0; r < 6; r++) { wJ[0][r] = J[0][r] * wi; wJ[1][r] = J[1][r] * wi; }
            if (!e.stereo) {
                int u = 0;
                for (int r = 0; r < 6; r++) {
                    const double g = J[0][r] * e.info * e.err[0] + J[1][r] * e.info * e.err[1];
                    b[r] -= w * g;
                    for (int c = r; c < 6; c++, u++) Hu[u] += wJ[0][r] * J[0][c] + wJ[1][r] * J[1][c];
                }
            } else {
                for (int r = 0; r < 6; r++) wJ[2][r] = J[2][r] * wi;
                int u = 0;
                for (int r = 0; r < 6; r++) {
                    const double g = J[0][r] * e.info * e.err[0] + J[1][r] * e.info * e.err[1] + J[2][r] * e.info * e.err[2];
                    b[r] -= w * g;
                    for (int c = r; c < 6; c++, u++) Hu[u] += wJ[0][r] * J[0][c] + wJ[1][r] * J[1][c] + wJ[2][r] * J[2][c];
                }
            }
        }
        int u = 0;
        for (int r = 0; r < 6; r++)
            for (int c = r; c < 6; c++, u++) H[6 * r + c] = H[6 * c + r] = Hu[u];
    }

    // OptimizationAlgorithmLevenberg::solve driven by SparseOptimizer::optimize (sparse_optimizer.cpp:354-420)
    void optimize(int iterations)
    {
        double lambda = 0, ni = 2;
        int n_bad = 0;
        // g2o recomputes the active errors and their robust chi2 at the top of every iteration; right after an accepted
        // step they are exactly what the trial left on the edges, so that pass is skipped (same values, same sum)
        bool fresh = false;
        double carried = 0;
        for (int it = 0; it < iterations; it++) {
            if (!fresh) { compute_active_errors(); carried = active_robust_chi2(); }
            double current = carried, temp = current;
            const double ini = current;
            double H[36], b[6], x[6];
            build_system(H, b);
            if (it == 0) {
                double mx = 0;
                for (int j = 0; j < 6; j++) mx = std::max(std::fabs(H[7 * j]), mx);
                lambda = 1e-5 * mx; ni = 2; n_bad = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                const Se3 backup = est;
                double Hl[36];
                memcpy(Hl, H, sizeof Hl);
                for (int j = 0; j < 6; j++) Hl[7 * j] += lambda;
                for (int j = 0; j < 6; j++) x[j] = 0;
                const bool ok2 = ldlt_solve6(Hl, b, x);
                est = se3_mul(se3_exp(x), est);
                compute_active_errors();
                temp = active_robust_chi2();
                if (!ok2) temp = DBL_MAX;
                rho = current - temp;
                double scale = 0;
                for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                scale += 1e-3;
                rho /= scale;
                if (rho > 0 && std::isfinite(temp)) {
                    double alpha = 1. - std::pow((2 * rho - 1), 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha);
                    ni = 2;
                    current = temp;
                    fresh = true; carried = temp;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    est = backup;          // the edges keep the trial's errors, as in g2o
                    fresh = false;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) return;
            if ((ini - current) * 1e3 < ini) n_bad++; else n_bad = 0;
            if (n_bad >= 3) return;
        }
    }
};
}   // namespace

extern "C" int orbp_pose_optimization(int n, const float *obs, const float *u_right, const float *inv_sigma2, const float *xw,
                                      float fx, float fy, float cx, float cy, float bf, float *Tcw, uint8_t *outlier)
{
    if (n < 0 || !Tcw || !outlier || (n > 0 && (!obs || !inv_sigma2 || !xw))) return pfail(ORBX_E_INVALID, "bad arguments");
    PoseProblem P;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.bf = bf;
    P.delta_mono = (float)std::sqrt(5.991); P.delta_stereo = (float)std::sqrt(7.815);     // const float delta* (:270-271)
    double R0[9], t0[3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R0[3 * i + j] = Tcw[4 * i + j]; t0[i] = Tcw[4 * i + 3]; }
    Se3 init;
    init.r = quat_from_R(R0);
    quat_normalize(init.r);
    memcpy(init.t, t0, sizeof t0);
    P.est = init;
    P.edges.resize(n);
    for (int i = 0; i < n; i++) {
        Edge &e = P.edges[i];
        e.idx = i; e.stereo = u_right && u_right[i] >= 0;
        e.obs[0] = obs[2 * i]; e.obs[1] = obs[2 * i + 1]; e.obs[2] = e.stereo ? u_right[i] : 0;
        for (int j = 0; j < 3; j++) e.xw[j] = xw[3 * i + j];
        e.info = inv_sigma2[i];
        e.err[0] = e.err[1] = e.err[2] = 0;
        e.robust = true; e.level = 0;
        outlier[i] = 0;
    }
    if (n < 3) return 0;                        // :363-364
    const float chi2_mono = 5.991f, chi2_stereo = 7.815f;
    int n_bad = 0;
    for (int it = 0; it < 4; it++) {
        P.est = init;                           // every round restarts from pFrame->mTcw (:375)
        P.active.clear();
        for (int i = 0; i < n; i++)
            if (P.edges[i].level == 0) P.active.push_back(i);
        if (!P.active.empty()) P.optimize(10);
        n_bad = 0;
        for (int i = 0; i < n; i++) {
            Edge &e = P.edges[i];
            if (outlier[i]) P.compute_error(e);
            const float c2 = (float)PoseProblem::chi2(e);
            if (c2 > (e.stereo ? chi2_stereo : chi2_mono)) { outlier[i] = 1; e.level = 1; n_bad++; }
            else { outlier[i] = 0; e.level = 0; }
            if (it == 2) e.robust = false;
        }
        if (n < 10) break;                      // optimizer.edges().size() < 10 (:443-444)
    }
    double R[9];
    quat_to_R(P.est.r, R);
    for (int i = 0; i < 16; i++) Tcw[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Tcw[4 * i + j] = (float)R[3 * i + j];
        Tcw[4 * i + 3] = (float)P.est.t[i];
    }
    return n - n_bad;
}
