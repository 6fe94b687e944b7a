// orbp_lm_body.h -- g2o's Levenberg loop by itself (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-164 with this
// fork's _nBad stop :154-161, computeLambdaInit :166-180, computeScale :182-189; driven by SparseOptimizer::optimize,
// core/sparse_optimizer.cpp:354-419): one text for the host solvers (orbp_lba/ba/eg.cc) and the GPU drivers (orbm_lba/eg.hip)
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define LM_HD __host__ __device__ __forceinline__
#define LM_UNROLL _Pragma("unroll")
#else
#define LM_HD static inline
#define LM_UNROLL
#endif
// the bound of lm_optimize's loop over iterations: LocalBundleAdjustment asks for 5 and 10, BundleAdjustment for up to
// ORBP_BA_MAX_ITERATIONS (include/orbp.h, the same number); the loop runs min(iterations, this) of them
#define LM_MAX_ITERATIONS 100
#define LM_MAX_TRIALS 10        // _maxTrialsAfterFailure
// one unknown's term of computeScale (optimization_algorithm_levenberg.cpp:186); constexpr: host and device under hipcc
constexpr double lm_scale_term(double x, double b, double lambda) { return x * (lambda * x + b); }
// What one optimize() did: g2o's counters and the state the caller reports (orbp_lba_stats)
struct LmRun { int iterations, trials; double lambda, chi2; };

// OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize(iterations), as s3o_optimize (orbp_sim3opt_body.h) is for
// one vertex, over "the passes of a problem".  Host code on both paths: the host solver's passes add in edge order, the GPU path's
// passes are kernel launches that add in their trees and hand back one small block a trial.
//   ctx.stop()                                  terminate()
//   ctx.linearize(first, errors, chi, maxdiag)  errors: computeActiveErrors + activeRobustChi2 into chi; always buildSystem; first:
//                                               computeLambdaInit's maximum over the diagonals of the free poses and points.  After
//                                               an accepted trial the edges hold that trial's errors and the chi2 g2o sums again at
//                                               the top of the next iteration is the trial's, term for term: it is carried instead.
//                                               After a rejected trial that ended its iteration (rho is NaN) they are computed anew.
//   ctx.trial(lambda, chi, scale, ok)           push, setLambda, solve, update, restoreDiagonal, computeActiveErrors,
//                                               activeRobustChi2, computeScale (without its + 1e-3)
//   ctx.accept() / ctx.reject()                 discardTop / pop: the edges keep the trial's errors either way
// user_lambda_init > 0 is setUserLambdaInit's value, which computeLambdaInit returns instead of tau * maxdiag (:168-169;
// OptimizeEssentialGraph sets 1e-16, orbp_eg_body.h).
template <class Ctx>
static inline void lm_optimize(Ctx &ctx, int iterations, LmRun &run, double user_lambda_init = 0)
{
    double lambda = 0, ni = 2, current = 0;
    int n_bad = 0;
    bool fresh = false;                                     // the edges hold the errors of the current estimates
    run.iterations = run.trials = 0;
    run.lambda = run.chi2 = 0;
    for (int it = 0; it < LM_MAX_ITERATIONS; it++) {
        if (it >= iterations || ctx.stop()) break;
        double chi = 0, maxdiag = 0;
        ctx.linearize(it == 0, !fresh, chi, maxdiag);
        if (!fresh) current = chi;
        if (it == 0) { lambda = user_lambda_init > 0 ? user_lambda_init : 1e-5 * maxdiag; ni = 2; n_bad = 0; }    // _tau = 1e-5
        const double ini = current;
        double rho = 0;
        int qmax = 0;
        do {
            double temp = 0, scale = 0;
            bool ok2 = false;
            ctx.trial(lambda, temp, scale, ok2);
            if (!ok2) temp = 1.7976931348623157e308;
            rho = current - temp;
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(temp)) {
                const double t = 2 * rho - 1;
                double alpha = 1. - t * t * t;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                current = temp;
                fresh = true;
                ctx.accept();
            } else {
                lambda *= ni;
                ni *= 2;
                fresh = false;
                ctx.reject();
            }
            qmax++;
            run.trials++;
        } while (rho < 0 && qmax < LM_MAX_TRIALS && !ctx.stop());
        run.iterations++;
        run.lambda = lambda;
        run.chi2 = current;
        if (qmax == LM_MAX_TRIALS || rho == 0) break;
        if ((ini - current) * 1e3 < ini) n_bad++; else n_bad = 0;
        if (n_bad >= 3) break;
    }
}

// N x N LDL^T solve of (H + lambda I) x = b on the upper triangle Hu, row-major (the reference: Eigen's LDLT inside
// g2o::LinearSolverDense), for the one vertex of PoseOptimization (N = 6) and of OptimizeSim3 (N = 7); false, and x = 0, where a
// pivot is zero or not finite
template <int N>
LM_HD bool lm_ldlt_solve(const double *Hu, double lambda, const double *b, double *x)
{
    double H[N * N], L[N * N], D[N], y[N];
    {
        int u = 0;
        LM_UNROLL
        for (int r = 0; r < N; r++)
            LM_UNROLL
            for (int c = r; c < N; c++, u++) H[N * r + c] = H[N * c + r] = Hu[u];
    }
    LM_UNROLL
    for (int j = 0; j < N; j++) H[(N + 1) * j] += lambda;
    bool ok = true;
    LM_UNROLL
    for (int j = 0; j < N; j++) {
        double d = H[N * j + j];
        LM_UNROLL
        for (int k = 0; k < j; k++) d -= L[N * j + k] * L[N * j + k] * D[k];
        if (!(fabs(d) > 0) || !isfinite(d)) ok = false;
        D[j] = d;
        LM_UNROLL
        for (int i = j + 1; i < N; i++) {
            double s = H[N * i + j];
            LM_UNROLL
            for (int k = 0; k < j; k++) s -= L[N * i + k] * L[N * j + k] * D[k];
            L[N * i + j] = s / d;
        }
    }
    LM_UNROLL
    for (int i = 0; i < N; i++) {
        double s = b[i];
        LM_UNROLL
        for (int k = 0; k < i; k++) s -= L[N * i + k] * y[k];
        y[i] = s;
    }
    LM_UNROLL
    for (int i = 0; i < N; i++) y[i] /= D[i];
    LM_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        double s = y[i];
        LM_UNROLL
        for (int k = i + 1; k < N; k++) s -= L[N * k + i] * x[k];
        x[i] = s;
    }
    if (!ok)
        LM_UNROLL
        for (int i = 0; i < N; i++) x[i] = 0;
    return ok;
}
