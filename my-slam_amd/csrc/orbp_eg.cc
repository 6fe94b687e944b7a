// orbp_eg.cc -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044 of WChen09/My-SLAM, on g2o) over the flat problem of
// include/orbp.h: orbp_optimize_essential_graph.  The edges' arithmetic is csrc/orbp_eg_body.h, the Levenberg loop lm_optimize
// (csrc/orbp_lm_body.h) with the user's initial lambda of :794.  This file owns the argument checks, the sums in edge order (g2o's
// active edges are sorted by id, which is insertion order) and the linear solve: BlockSolver_7_3 has Hpp alone, and the essential
// graph's Hpp is a band (spanning tree and covisibility) plus a few long rows (loop edges), so it is kept as an envelope.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_internal.h"
#include "orbp_eg_body.h"
#include "orbp_lm_body.h"

int orbp_eg_check(const orbp_eg_problem *p, int n_iterations, const float *Tcw, const float *xw, char *text, int text_size)
{
    const size_t ts = (size_t)text_size;
#define EG_BAD(...) do { snprintf(text, ts, "optimize_essential_graph: " __VA_ARGS__); return ORBX_E_INVALID; } while (0)
    if (!p) EG_BAD("NULL problem");
    if (p->n_kfs < 0 || p->n_edges < 0 || p->n_points < 0) EG_BAD("negative count");
    if (n_iterations < 0 || n_iterations > ORBP_BA_MAX_ITERATIONS) EG_BAD("n_iterations %d outside [0, %d]", n_iterations, ORBP_BA_MAX_ITERATIONS);
    if (p->n_kfs && (!p->Scw || !p->Snc || !Tcw)) EG_BAD("NULL Scw, Snc or Tcw");
    if (p->n_edges && (!p->edge_i || !p->edge_j || !p->edge_corrected)) EG_BAD("NULL edge array");
    if (p->n_points && (!p->ref || !xw)) EG_BAD("NULL ref or xw");
    if (p->fixed < -1 || p->fixed >= p->n_kfs) EG_BAD("fixed = %d with %d key frames", p->fixed, p->n_kfs);
    for (int k = 0; k < p->n_kfs; k++)
        for (int side = 0; side < 2; side++) {
            const double *S = (side ? p->Snc : p->Scw) + 8 * (size_t)k;
            for (int j = 0; j < 8; j++)
                if (!std::isfinite(S[j])) EG_BAD("%s of key frame %d is not finite", side ? "Snc" : "Scw", k);
            if (!(S[7] > 0)) EG_BAD("%s of key frame %d has scale %g", side ? "Snc" : "Scw", k, S[7]);
        }
    for (int e = 0; e < p->n_edges; e++) {
        const int i = p->edge_i[e], j = p->edge_j[e];
        if (i < 0 || i >= p->n_kfs || j < 0 || j >= p->n_kfs) EG_BAD("edge %d joins %d and %d of %d key frames", e, i, j, p->n_kfs);
        if (i == j) EG_BAD("edge %d joins key frame %d with itself", e, i);
    }
    for (int q = 0; q < p->n_points; q++)
        if (p->ref[q] < -1 || p->ref[q] >= p->n_kfs) EG_BAD("point %d has reference %d of %d key frames", q, p->ref[q], p->n_kfs);
#undef EG_BAD
    return ORBX_OK;
}

static thread_local int eg_dense = 0;
extern "C" void orbp_eg_set_dense(int dense) { eg_dense = dense; }

namespace {
// "the passes of a problem" for lm_optimize on the host
struct EgHost {
    const orbp_eg_problem *p;
    int n, nf, N, E;                        // key frames, free ones, unknowns = 7 nf, edges
    bool fix_scale;
    std::vector<int32_t> free_of;           // key frame -> its place among the free ones, or -1
    std::vector<S3oSim> est, backup, meas;
    std::vector<double> err, Ji, Jj;        // 7, 49, 49 an edge
    // the envelope: row r holds the columns first[r] .. r at val[start[r]] ..; H and b as assembled, L the factor of a trial
    std::vector<int32_t> first;
    std::vector<size_t> start;
    std::vector<double> H, L, b, x;
    double chi2_initial = 0;

    void prepare(const orbp_eg_problem *pr)
    {
        p = pr; n = p->n_kfs; E = p->n_edges; fix_scale = p->fix_scale != 0;
        free_of.assign(n, -1);
        nf = 0;
        for (int k = 0; k < n; k++)
            if (k != p->fixed) free_of[k] = nf++;
        N = 7 * nf;
        est.resize(n);
        for (int k = 0; k < n; k++) est[k] = eg_load(p->Scw + 8 * (size_t)k);
        meas.resize(E);
        for (int e = 0; e < E; e++) {       // :857-867, :889-914: Sji = Sjw * Swi
            const double *S = p->edge_corrected[e] ? p->Scw : p->Snc;
            meas[e] = s3o_mul(eg_load(S + 8 * (size_t)p->edge_j[e]), s3o_inverse(eg_load(S + 8 * (size_t)p->edge_i[e])));
        }
        err.assign(7 * (size_t)E, 0.); Ji.assign(49 * (size_t)E, 0.); Jj.assign(49 * (size_t)E, 0.);
        std::vector<int32_t> lo(nf);
        for (int f = 0; f < nf; f++) lo[f] = eg_dense ? 0 : f;
        for (int e = 0; e < E; e++) {
            const int a = free_of[p->edge_i[e]], c = free_of[p->edge_j[e]];
            if (a >= 0 && c >= 0) lo[std::max(a, c)] = std::min(lo[std::max(a, c)], std::min(a, c));
        }
        first.resize(N); start.resize((size_t)N + 1);
        start[0] = 0;
        for (int r = 0; r < N; r++) {
            first[r] = 7 * lo[r / 7];
            start[r + 1] = start[r] + (size_t)(r - first[r] + 1);
        }
        H.resize(start[N]); L.resize(start[N]); b.resize(N); x.assign(N, 0.);
    }
    double &at(std::vector<double> &M, int r, int c) { return M[start[r] + (size_t)(c - first[r])]; }
    bool stop() const { return false; }
    double errors()                         // computeActiveErrors + activeChi2, in edge order
    {
        double chi = 0;
        for (int e = 0; e < E; e++) {
            eg_error(meas[e], est[p->edge_i[e]], s3o_inverse(est[p->edge_j[e]]), &err[7 * (size_t)e]);
            chi += eg_chi2(&err[7 * (size_t)e]);
        }
        return chi;
    }
    void linearize(bool first_it, bool with_errors, double &chi, double &maxdiag)
    {
        // the errors are computed either way: after an accepted trial they are the trial's, term for term
        const double c = errors();
        if (with_errors) chi = c;
        if (first_it) chi2_initial = c;
        maxdiag = 0;                        // computeLambdaInit returns the user's value
        std::fill(H.begin(), H.end(), 0.); std::fill(b.begin(), b.end(), 0.);
        for (int e = 0; e < E; e++) {
            const int vi = p->edge_i[e], vj = p->edge_j[e], fi = free_of[vi], fj = free_of[vj];
            double *A = &Ji[49 * (size_t)e], *B = &Jj[49 * (size_t)e];
            for (int side = 0; side < 2; side++) {
                if ((side ? fj : fi) < 0) continue;
                double *J = side ? B : A;
                for (int d = 0; d < 7; d++) {
                    double plus[7], minus[7];
                    eg_lin_error(meas[e], est[vi], est[vj], 14 * side + 1 + 2 * d, fix_scale, plus);
                    eg_lin_error(meas[e], est[vi], est[vj], 14 * side + 2 + 2 * d, fix_scale, minus);
                    for (int r = 0; r < 7; r++) J[7 * r + d] = eg_jac(plus[r], minus[r]);
                }
            }
            const double *er = &err[7 * (size_t)e];
            for (int side = 0; side < 2; side++) {
                const int f = side ? fj : fi;
                if (f < 0) continue;
                const double *J = side ? B : A;
                for (int a = 0; a < 7; a++) {
                    b[7 * f + a] += eg_b_term(J, er, a);
                    for (int c2 = 0; c2 <= a; c2++) at(H, 7 * f + a, 7 * f + c2) += eg_h_term(J, J, a, c2);
                }
            }
            if (fi >= 0 && fj >= 0) {       // the block below the diagonal: rows of the later vertex
                const double *Jr = fi > fj ? A : B, *Jc = fi > fj ? B : A;
                const int fr = std::max(fi, fj), fc = std::min(fi, fj);
                for (int a = 0; a < 7; a++)
                    for (int c2 = 0; c2 < 7; c2++) at(H, 7 * fr + a, 7 * fc + c2) += eg_h_term(Jr, Jc, a, c2);
            }
        }
    }
    // (H + lambda I) = L L^T inside the envelope, L y = b, L^T x = y; every entry and every sum as the dense factorisation of
    // the bundle adjustments (LbaHost::cholesky_solve) computes them, minus the terms that are structurally zero
    bool solve(double lambda)
    {
        for (int i = 0; i < N; i++) {
            for (int j = first[i]; j < i; j++) {
                double s = at(H, i, j);
                for (int k = std::max(first[i], first[j]); k < j; k++) s -= at(L, j, k) * at(L, i, k);
                at(L, i, j) = s / at(L, j, j);
            }
            double d = at(H, i, i) + lambda;
            for (int k = first[i]; k < i; k++) d -= at(L, i, k) * at(L, i, k);
            if (!(d > 0) || !std::isfinite(d)) return false;
            at(L, i, i) = std::sqrt(d);
        }
        for (int i = 0; i < N; i++) {
            double s = b[i];
            for (int k = first[i]; k < i; k++) s -= at(L, i, k) * x[k];
            x[i] = s / at(L, i, i);
        }
        // the last row that reaches column i bounds the scan of that column
        std::vector<int32_t> last(N);
        for (int i = 0; i < N; i++) last[i] = i;
        for (int r = 0; r < N; r++)
            for (int c = first[r]; c < r; c++) last[c] = r;
        for (int i = N - 1; i >= 0; i--) {
            double s = x[i];
            for (int k = i + 1; k <= last[i]; k++)
                if (first[k] <= i) s -= at(L, k, i) * x[k];
            x[i] = s / at(L, i, i);
        }
        return true;
    }
    void trial(double lambda, double &chi, double &scale, bool &ok)
    {
        backup = est;                       // push
        ok = solve(lambda);
        if (!ok) std::fill(x.begin(), x.end(), 0.);
        scale = 0;
        for (int i = 0; i < N; i++) scale += lm_scale_term(x[i], b[i], lambda);
        for (int k = 0; k < n; k++)
            if (free_of[k] >= 0) est[k] = s3o_oplus(est[k], &x[7 * (size_t)free_of[k]], fix_scale);
        chi = errors();
    }
    void accept() {}
    void reject() { est = backup; }
};
}   // namespace

extern "C" int orbp_optimize_essential_graph(const orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw, double *Scw_out,
                                             orbp_eg_stats *stats)
{
    char text[200];
    if (orbp_eg_check(p, n_iterations, Tcw, xw, text, (int)sizeof text) != ORBX_OK) {
        orbp_set_error(text);
        return ORBX_E_INVALID;
    }
    EgHost h;
    h.prepare(p);
    LmRun run = {0, 0, 0, 0};
    if (h.E > 0 && h.nf > 0) lm_optimize(h, n_iterations, run, 1e-16);      // :794, :986-987
    if (run.iterations == 0) h.chi2_initial = h.errors();
    for (int k = 0; k < h.n; k++) {                                         // :992-1010
        eg_to_Tcw(h.est[k], Tcw + 16 * (size_t)k);
        if (Scw_out) eg_store(Scw_out + 8 * (size_t)k, h.est[k]);
    }
    for (int q = 0; q < p->n_points; q++)                                   // :1013-1043
        if (p->ref[q] >= 0) eg_correct_point(eg_load(p->Scw + 8 * (size_t)p->ref[q]), h.est[p->ref[q]], xw + 3 * (size_t)q);
    if (stats) *stats = {run.iterations, run.trials, run.lambda, h.chi2_initial, run.iterations ? run.chi2 : h.chi2_initial};
    return 0;
}
