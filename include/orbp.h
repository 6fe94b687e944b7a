/*
 * orbp.h -- C ABI of the host-side pose solvers of liborbx.so: "next" row N4 of SURVEY.md 8(f).
 *
 * They are plain C++ inside liborbx.so, take the outputs of the device path (orbx_extract -> orbv_* -> orbm_search_by_bow) and
 * close BASELINE config 5's loop.  SURVEY 8(f) N4 keeps one such solve on the host ("tiny dense fp64 solves"); the RANSAC
 * hypotheses of a whole Relocalization, ComputeSim3 or MonocularInitialization step are hundreds of independent ones, and those
 * have a GPU call each (orbm_pnp_hypotheses, orbm_sim3_hypotheses, orbm_init_hypotheses in include/orbm.h) that the solvers here
 * draw for and replay.  The monocular Initializer (src/Initializer.cc) is the third of them, further down.
 *
 * Reference (WChen09/My-SLAM):
 *   src/PnPsolver.cc:66-109    PnPsolver::PnPsolver          -> orbp_pnp_create   (caller drops NULL / bad MapPoints)
 *   src/PnPsolver.cc:120-158   SetRansacParameters           -> orbp_pnp_set_ransac_parameters
 *   src/PnPsolver.cc:160-164   find                          -> orbp_pnp_find
 *   src/PnPsolver.cc:166-258   iterate (RANSAC over 4-point EPnP, Refine :260-309, CheckInliers :312-344)
 *                                                            -> orbp_pnp_iterate
 *   src/PnPsolver.cc:346-1022  EPnP (Lepetit, Moreno-Noguer, Fua, IJCV 2009): control points by PCA, barycentric
 *                              coordinates, null space of M^T M, the three beta approximations, 5 Gauss-Newton
 *                              steps, absolute orientation, least mean reprojection error wins
 *                                                            -> orbp_epnp
 *   src/Optimizer.cc:239-451   Optimizer::PoseOptimization   -> orbp_pose_optimization
 *       with g2o's EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
 *       (Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h:143-215,cpp:266-364}), SE3Quat::exp
 *       (types/se3quat.h:223-257), RobustKernelHuber (core/robust_kernel_impl.cpp:78-91) and
 *       OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:66-170, including this
 *       fork's _nBad early stop :157-164) over a dense 6x6 system.
 *   Call sites: src/Tracking.cc:766-809 (TrackReferenceKeyFrame), :1348-1509 (Relocalization).
 *
 * Dependencies the reference takes from OpenCV 3.1.0 / Eigen3 (neither is in the image) are replaced by a one-sided
 * Jacobi SVD and a 6x6 LDL^T written here.  Where the reference's result depends on those libraries' internals the
 * behaviour is implementation-defined and documented in DESIGN.md ("parity unpinned"): the basis OpenCV returns for
 * the (numerically) null singular vectors of the rank-8 M^T M of a 4-point sample (any orthonormal basis of that null
 * space is a valid SVD; which one comes out is an artefact of the Jacobi sweep order, and EPnP's beta linearisations
 * depend on it), the sign of the PCA axes, and the completion of U for a rank-deficient 3x3.
 * RANSAC draws: DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) on libc rand(); the default
 * source here is the same rand() with the same formula, so a process that seeds like the reference draws like it.
 */
#ifndef ORBP_H
#define ORBP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbp_pnp orbp_pnp;

/* n correspondences: p2d = mvKeysUn[i].pt (2n floats), sigma2 = mvLevelSigma2[octave] (n), p3d = world position (3n). */
int orbp_pnp_create(orbp_pnp **out, int n, const float *p2d, const float *sigma2, const float *p3d,
                    float fx, float fy, float cx, float cy);
void orbp_pnp_destroy(orbp_pnp *s);
/* Uniform source for the RANSAC draws: fn(ctx) in [0, rand_max].  NULL restores libc rand() / RAND_MAX. */
void orbp_pnp_set_rand(orbp_pnp *s, int (*fn)(void *), void *ctx, int rand_max);
int orbp_pnp_set_ransac_parameters(orbp_pnp *s, double probability, int min_inliers, int max_iterations, int min_set,
                                   float epsilon, float th2);
/* Effective values after SetRansacParameters' adjustment (any pointer may be NULL). */
void orbp_pnp_get_ransac_state(const orbp_pnp *s, int *min_inliers, int *max_its, float *epsilon, int *iterations_done);
/* Returns 1 and fills Tcw (row-major 4x4 float), inliers[n] (0/1) and *n_inliers when a pose is returned, 0 when the
 * reference returns an empty cv::Mat (inliers untouched, *n_inliers = 0), < 0 on bad arguments. */
int orbp_pnp_iterate(orbp_pnp *s, int n_iterations, int *no_more, uint8_t *inliers, int *n_inliers, float *Tcw);
int orbp_pnp_find(orbp_pnp *s, uint8_t *inliers, int *n_inliers, float *Tcw);

/*
 * The hypotheses of a solver do not depend on each other, only on the draws: compute_pose + CheckInliers (:206-210) read the
 * problem and the sample, and only the walk that keeps the best set, calls Refine and decides what iterate returns is sequential.
 * So they can be evaluated ahead of iterate(), as for Sim3Solver below: orbp_pnp_draw performs the draws of the coming iterations
 * exactly as iterate would (:188-204) and queues the index sets; orbm_pnp_hypotheses (include/orbm.h) evaluates the queued sets of
 * many solvers in one GPU call; orbp_pnp_attach_results hands the results back, and iterate() replays them: it restores mRi, mti,
 * mvbInliersi and mnInliersi from them and runs everything after CheckInliers as written (the > mnBestInliers rule, Refine on the
 * best set so far with its strict > mRansacMinInliers, bNoMore).  Same return values, poses, flags and counts, byte for byte, as
 * evaluating in place, because host and kernel run one body (csrc/orbp_epnp_body.h).  iterate() consumes queued sets before it
 * draws new ones; a queued set without results is evaluated in place.  Refine (an n-point EPnP) stays on the host.  A solver that
 * was never drawn ahead behaves as it always did.  orbp_pnp_set_ransac_parameters drops queued sets and attached results.
 */
/* The solver as a problem of orbm_pnp_hypotheses: p2d (2n floats), p3d (3n floats), max_err (n: mvMaxError = sigma2 * th2 as the
 * float CheckInliers compares with), K = {fx, fy, cx, cy}, *min_set = mRansacMinSet.  Returns n. */
int orbp_pnp_get_problem(const orbp_pnp *s, float *p2d, float *p3d, float *max_err, float *K, int32_t *min_set);
/* Draws the index sets (min_set indices each) of the iterations a following iterate(n_iterations) consumes beyond the queued
 * ones: the reference's loop is `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` (:182), so that call runs
 * until BOTH counts are reached unless a pose comes back earlier: it consumes max(max_its - iterations_done, n_iterations) sets,
 * and the number drawn is that less the queued ones (nothing when the queue already covers the call, so calling it twice draws
 * once).  Nothing is drawn when n < min_inliers (iterate returns at once).
 * Appends the sets to the queue and to samples (min_set ints per set; may be NULL).  Returns the number of sets drawn, < 0 on bad
 * arguments. */
int orbp_pnp_draw(orbp_pnp *s, int n_iterations, int32_t *samples);
/* The queued, not yet consumed sets (min_set * return value ints into samples when it is not NULL). */
int orbp_pnp_queued(const orbp_pnp *s, int32_t *samples);
/* One hypothesis, stateless: R (9, row-major) and t (3) are mRi / mti in double, inliers[n] (0/1) and *n_inliers of the sample of
 * min_set distinct correspondence indices. */
int orbp_pnp_hypothesis(const orbp_pnp *s, const int32_t *sample, double *R, double *t, uint8_t *inliers, int *n_inliers);
/* Results for ALL queued sets, in queue order, in the layout of orbm_pnp_hypotheses: counts[n_hyp], Rt[12 n_hyp] (R row-major,
 * then t), masks[n_hyp * ceil(n / 32)] (bit i of a hypothesis' words = correspondence i).  n_hyp must equal orbp_pnp_queued(). */
int orbp_pnp_attach_results(orbp_pnp *s, int n_hyp, const int32_t *counts, const double *Rt, const uint32_t *masks);

/* PnPsolver::compute_pose on n >= 4 correspondences (pws 3n, us 2n doubles): R row-major, t; returns the mean
 * reprojection error of the chosen solution. */
double orbp_epnp(int n, const double *pws, const double *us, double fu, double fv, double uc, double vc,
                 double *R, double *t);

/* Optimizer::PoseOptimization.  Observation i: obs (2n floats, mvKeysUn[i].pt), u_right[i] < 0 (or u_right == NULL)
 * for a monocular edge, inv_sigma2 = mvInvLevelSigma2[octave], xw = world position (3n floats).  Tcw: in = pFrame->mTcw,
 * out = optimised pose (row-major 4x4 float).  outlier[n] receives mvbOutlier.  Returns nInitialCorrespondences - nBad
 * (0 when fewer than 3 observations: pose untouched), < 0 on bad arguments. */
int orbp_pose_optimization(int n, const float *obs, const float *u_right, const float *inv_sigma2, const float *xw,
                           float fx, float fy, float cx, float cy, float bf, float *Tcw, uint8_t *outlier);

/*
 * ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241), LoopClosing::ComputeSim3's call at src/LoopClosing.cc:327 ----
 * One free VertexSim3Expmap; both point vertices of every correspondence are fixed (:1121, :1129), so the graph is one dense 7x7
 * system and a sum over the edges.  With g2o's Sim3 (types/sim3.h), EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ
 * (types/types_seven_dof_expmap.h:130-171; their linearizeOplus is commented out, so the Jacobian is g2o's numeric one,
 * core/base_binary_edge.hpp:130-205: central differences with delta 1e-9), RobustKernelHuber and the Levenberg loop of
 * orbp_pose_optimization.  csrc/orbp_sim3opt_body.h cites each quirk at its line.
 *
 * Correspondence i (the caller gathers as :1099-1178 does and skips what the reference skips):
 *   x1c, x2c   (3n floats each) R1w * P3D1w + t1w and R2w * P3D2w + t2w as the float cv::Mat holds them
 *   obs1, obs2 (2n floats each) pKF1->mvKeysUn[i].pt and pKF2->mvKeysUn[i2].pt
 *   inv_sigma2_1, inv_sigma2_2  mvInvLevelSigma2[octave] of the two key points
 * K1, K2 = {fx, fy, cx, cy} of pKF1 and pKF2; th2 and fix_scale as the reference's arguments.
 * S12: g2oS12 in the order of g2o::Sim3::operator[] (sim3.h:239-264): qx, qy, qz, qw, tx, ty, tz, s; in and out, never normalised.
 * flags[i] = 1 where the reference sets vpMatches1[idx] = NULL, in either flagging pass (:1193-1202, :1227-1231).
 * Returns nIn; 0 with S12 untouched and the first pass's flags set when nCorrespondences - nBad < 10 (:1211-1212); ORBX_E_INVALID
 * on n < 0, a NULL pointer or a non-finite S12.
 */
int orbp_optimize_sim3(int n, const float *x1c, const float *x2c, const float *obs1, const float *obs2, const float *inv_sigma2_1,
                       const float *inv_sigma2_2, const float *K1, const float *K2, float th2, int fix_scale, double *S12,
                       uint8_t *flags);
/* g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) (src/LoopClosing.cc:326) in the order of S12 above: R row-major
 * (9 floats), t (3 floats); the quaternion is Eigen's Quaterniond(Matrix3d), not normalised. */
int orbp_sim3_from_rts(const float *R, const float *t, float s, double *out);

/*
 * ---- Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h): RANSAC over 3-point Horn solves, LoopClosing::ComputeSim3 ----
 *   src/Sim3Solver.cc:35-112   Sim3Solver::Sim3Solver   -> orbp_sim3_create (the caller does Rcw*Xw+tcw and drops NULL / bad
 *                                                          MapPoints and those without an index, :62-103)
 *   :114-138  SetRansacParameters -> orbp_sim3_set_ransac_parameters      :140-213  iterate / find -> orbp_sim3_iterate / _find
 *   :226-337  ComputeSim3 (Horn 1987) and :340-403 CheckInliers / Project -> orbp_sim3_hypothesis (csrc/orbm_sim3_body.h)
 *
 * n correspondences: x3dc1 / x3dc2 = the point in camera 1 / 2 (3n floats each), sigma2_1 / sigma2_2 = mvLevelSigma2[octave] of
 * its keypoint in key frame 1 / 2 (n each), K1 / K2 = {fx, fy, cx, cy}.  The thresholds are the reference's: mvnMaxError1/2 are
 * std::vector<size_t>, so 9.210 * sigma2 is truncated to an integer before it is compared as a float (sigma2 = 1.44 -> 13).
 *
 * The hypotheses of a solver do not depend on each other, only on the draws, so they can be evaluated ahead of iterate():
 * orbp_sim3_draw performs the draws of the next iterations exactly as iterate would (:163-177) and queues the index triples;
 * orbm_sim3_hypotheses (include/orbm.h) evaluates the queued triples of many solvers in one GPU call; orbp_sim3_attach_results
 * hands the results back, and iterate() then replays them: same counts, flags and poses, byte for byte, as evaluating in place,
 * because host and kernel run one body.  iterate() consumes queued triples before it draws new ones, with or without results.
 *
 * What OpenCV does inside cv::eigen / cv::Rodrigues / gemm is "parity unpinned" as for EPnP above (csrc/orbm_sim3_body.h lists
 * the choices).  Collinear or coincident sample points are outside the value contract (the flags are still 0/1).
 */
typedef struct orbp_sim3 orbp_sim3;
int orbp_sim3_create(orbp_sim3 **out, int n, const float *x3dc1, const float *x3dc2, const float *sigma2_1, const float *sigma2_2,
                     const float *K1, const float *K2, int fix_scale);   /* ends with SetRansacParameters() = (0.99, 6, 300) */
void orbp_sim3_destroy(orbp_sim3 *s);
/* fn(ctx) in [0, rand_max]; NULL restores libc rand() / RAND_MAX through RandomInt's formula (as orbp_pnp_set_rand). */
void orbp_sim3_set_rand(orbp_sim3 *s, int (*fn)(void *), void *ctx, int rand_max);
/* :114-138.  n == min_inliers gives 1 iteration; n < min_inliers (the reference's formula takes the log of a non-positive
 * number there) is defined as 1 iteration as well: iterate() returns at once with no_more set in that case.  Resets the
 * iteration count and drops queued triples and attached results; the best hypothesis so far stays, as in the reference. */
int orbp_sim3_set_ransac_parameters(orbp_sim3 *s, double probability, int min_inliers, int max_iterations);
void orbp_sim3_get_ransac_state(const orbp_sim3 *s, int *min_inliers, int *max_its, float *epsilon, int *iterations_done,
                                int *best_inliers);      /* any pointer may be NULL */
/* The solver as a problem of orbm_sim3_hypotheses: its correspondences x3dc1 / x3dc2 (3n floats each), max_err1 / max_err2
 * (mvnMaxError1 / 2 as the floats CheckInliers compares with, n each), the calibrations (4 floats each) and mbFixScale.
 * Returns n. */
int orbp_sim3_get_problem(const orbp_sim3 *s, float *x3dc1, float *x3dc2, float *max_err1, float *max_err2, float *K1, float *K2,
                          int32_t *fix_scale);
/* Draws the triples of the next n_iterations iterations (capped at what remains of mRansacMaxIts after the queued ones; nothing
 * when n < min_inliers or n < 3), appends them to the queue and to triples (3 per iteration; may be NULL).  Returns the number
 * of iterations drawn, < 0 on bad arguments. */
int orbp_sim3_draw(orbp_sim3 *s, int n_iterations, int32_t *triples);
/* The queued, not yet consumed triples (3 * return value ints into triples when it is not NULL). */
int orbp_sim3_queued(const orbp_sim3 *s, int32_t *triples);
/* One hypothesis, stateless: R (9, row-major), t (3), *scale, inliers[n] (0/1), *n_inliers of the triple of correspondence indices. */
int orbp_sim3_hypothesis(const orbp_sim3 *s, const int32_t *triple, float *R, float *t, float *scale, uint8_t *inliers, int *n_inliers);
/* Results for ALL queued triples, in queue order, in the layout of orbm_sim3_hypotheses: counts[n_hyp], sRt[13 n_hyp] (s, R, t),
 * masks[n_hyp * ceil(n / 32)] (bit i of a hypothesis' words = correspondence i).  n_hyp must equal orbp_sim3_queued(). */
int orbp_sim3_attach_results(orbp_sim3 *s, int n_hyp, const int32_t *counts, const float *sRt, const uint32_t *masks);
/* :140-207.  inliers[n] is cleared on every call.  Returns 1 and fills inliers, *n_inliers and T12 (row-major 4x4) when a pose
 * is returned, 0 when the reference returns an empty cv::Mat, < 0 on bad arguments.  *no_more is set on the call that reaches
 * mRansacMaxIts, also when that call returns a pose (the reference's early return reports it one call later, on a call that
 * iterates nothing; ComputeSim3 discards the candidate either way after it has used the pose).  The state survives a returned pose: iterating on continues the same RANSAC.  n < 3 sets *no_more like n < min_inliers. */
int orbp_sim3_iterate(orbp_sim3 *s, int n_iterations, int *no_more, uint8_t *inliers, int *n_inliers, float *T12);
int orbp_sim3_find(orbp_sim3 *s, uint8_t *inliers, int *n_inliers, float *T12);
/* GetEstimatedRotation / Translation / Scale: the best hypothesis so far; returns 0 before the first iteration. */
int orbp_sim3_get_estimated(const orbp_sim3 *s, float *R, float *t, float *scale);
/*
 * ---- Initializer (src/Initializer.cc, include/Initializer.h): Tracking::MonocularInitialization's two-view reconstruction ----
 *   src/Initializer.cc:33-42    Initializer::Initializer -> orbp_init_create (keys1 = mvKeysUn[i].pt of the reference frame,
 *                                                           {fx, fy, cx, cy} of mK)
 *   :44-121   Initialize        -> orbp_init_set_current + orbp_init_initialize      :82-97 the draws -> orbp_init_draw
 *   :124-223  FindHomography / FindFundamental -> orbp_init_find over orbp_init_hypothesis (csrc/orbp_init_body.h)
 *   :470-732  ReconstructF / ReconstructH -> orbp_init_motions, orbp_init_check_rt and the acceptance rules inside _initialize
 *   :749-795  Normalize (over ALL keys of a frame) -> inside orbp_init_set_current (orbp_init_normalized reads it back)
 *
 * The 2 * mMaxIterations hypotheses of a call do not depend on each other, only on the draws, and all draws come first: orbp_init_draw
 * performs them, orbm_init_hypotheses (include/orbm.h) evaluates them in one GPU call, orbp_init_attach_results hands the results
 * back and the walks replay them; likewise orbm_init_check_rt / orbp_init_attach_check_rt for the 4 or 8 CheckRT passes.  Same
 * scores, matrices, flags, motions and points, byte for byte, as evaluating in place, because host and kernels run one body.
 * What OpenCV does inside cv::SVDecomp / invert / gemm is "parity unpinned" as above (the body's header lists the choices, the sign
 * of the null vector among them).  The reference runs the two walks on two threads; the results do not depend on that.
 *
 * Defined here where the reference is not: fewer than 8 matches (RandomInt(0, -1)) is refused by orbp_init_draw and by
 * orbp_init_initialize with ORBX_E_INVALID; SH == SF == 0 (RH is NaN and the reference decomposes an empty matrix) makes
 * orbp_init_initialize return 0.  With the default source the first draw of the process calls srand(0), once (SeedRandOnce(0), :80).
 * Models: 0 = homography, 1 = fundamental matrix.  Matrices are row-major 3 x 3 floats.
 */
typedef struct orbp_init orbp_init;
int orbp_init_create(orbp_init **out, const float *keys1, int n1, float fx, float fy, float cx, float cy, float sigma, int iterations);
void orbp_init_destroy(orbp_init *s);
/* fn(ctx) in [0, rand_max]; NULL restores libc rand() / RAND_MAX through RandomInt's formula (as orbp_sim3_set_rand). */
void orbp_init_set_rand(orbp_init *s, int (*fn)(void *), void *ctx, int rand_max);
/* :49-63 and both Normalize calls: keys2 = mvKeysUn[i].pt of the current frame (2 n2 floats), matches12[n1] = vMatches12 (< 0: no
 * match).  Drops the sets and every attached result of the frame before.  Returns N = mvMatches12.size(). */
int orbp_init_set_current(orbp_init *s, const float *keys2, int n2, const int32_t *matches12);
int orbp_init_get_sizes(const orbp_init *s, int *n1, int *n2, int *n_matches, int *iterations, int *drawn);    /* any pointer may be NULL */
/* :82-97: mMaxIterations sets of 8 match indices into sets (may be NULL) and into the solver.  Returns the number of sets;
 * ORBX_E_INVALID with nothing drawn when N < 8. */
int orbp_init_draw(orbp_init *s, int32_t *sets);
/* The solver as a problem of orbm_init_hypotheses / orbm_init_check_rt: uv and pn (4 N floats each), params[24] = T1 (9), T2 (9),
 * sigma, fx, fy, cx, cy, th2 = 4 * mSigma2 (the first 19 are an orbm_init_params), the drawn sets (8 * iterations ints, when drawn),
 * m1 / m2 = mvMatches12[i].first / .second.  Any pointer may be NULL.  Returns N. */
int orbp_init_get_problem(const orbp_init *s, float *uv, float *pn, float *params, int32_t *sets, int32_t *m1, int32_t *m2);
/* vPn1 (2 n1 floats), T1, vPn2 (2 n2), T2 of the current pair; any pointer may be NULL */
int orbp_init_normalized(const orbp_init *s, float *pn1, float *T1, float *pn2, float *T2);
/* One hypothesis, stateless: M = H21i / F21i, *score = currentScore, inliers[N] (0/1) and their number. */
int orbp_init_hypothesis(const orbp_init *s, int model, const int32_t *set, float *M, float *score, uint8_t *inliers, int *n_inliers);
/* Results of ALL 2 * iterations hypotheses in the layout of orbm_init_hypotheses: the H of every set in draw order, then the F. */
int orbp_init_attach_results(orbp_init *s, int n_hyp, const float *score_M, const int32_t *counts, const uint32_t *masks);
/* The walk of :148-171 (model 0) / :199-222 (model 1): strict >, so the first of equal scores wins; over the attached results when
 * there are any, evaluating in place otherwise.  Returns 1 and the winner's matrix, score, flags and iteration, 0 when no score
 * exceeded 0 (M and inliers zero, *best_iteration = -1). */
int orbp_init_find(orbp_init *s, int model, float *M, float *score, uint8_t *inliers, int *best_iteration);
/* The candidate motions of ReconstructF (4: DecomposeE's (R1, t) (R2, t) (R1, -t) (R2, -t)) or ReconstructH (8, Faugeras) of M into
 * Rt (12 floats each: R row-major, t; room for 8).  Returns 1, or 0 at ReconstructH's d1/d2 < 1.00001 || d2/d3 < 1.00001 exit. */
int orbp_init_motions(const orbp_init *s, int model, const float *M, float *Rt, int *n_motions);
/* CheckRT (:798-907) of one motion on the host: p3d[3 n1] = vP3D, good[n1] = vbGood, *parallax, *n_good = the return value. */
int orbp_init_check_rt(const orbp_init *s, const float *R, const float *t, const uint8_t *inliers, float *p3d, uint8_t *good,
                       float *parallax, int *n_good);
/* The per-match part of CheckRT for n_motions motions, in the layout of orbm_init_check_rt (status, cos_parallax: n_motions * N,
 * p3d: 3 * n_motions * N). */
int orbp_init_check_rt_matches(const orbp_init *s, int n_motions, const float *Rt, const uint8_t *inliers, uint8_t *status,
                               float *cos_parallax, float *p3d);
/* Hands the outputs of orbm_init_check_rt back: orbp_init_initialize uses them for the motions and flags they were computed for
 * (compared by value) and computes every other CheckRT in place. */
int orbp_init_attach_check_rt(orbp_init *s, int n_motions, const float *Rt, const uint8_t *inliers, const uint8_t *status,
                              const float *cos_parallax, const float *p3d);
/* Initialize up to its CheckRT calls: both walks, RH = SH / (SH + SF) > 0.40, the motions of the chosen model.  *model, M, its
 * inlier flags (N) and Rt (room for 8 motions).  Returns the number of motions; 0 where Initialize returns false before CheckRT. */
int orbp_init_plan_check_rt(orbp_init *s, int *model, float *M, uint8_t *inliers, float *Rt, int *n_motions);
/* The whole of Initialize (:99-120) after orbp_init_set_current: draws unless drawn, both walks, the ratio, ReconstructH /
 * ReconstructF (minParallax 1.0, minTriangulated 50).  Returns 1 and fills R21 (9), t21 (3), p3d[3 n1] = vP3D and
 * triangulated[n1] = vbTriangulated; 0 when the reference returns false (outputs untouched); < 0 on bad arguments or N < 8. */
int orbp_init_initialize(orbp_init *s, float *R21, float *t21, float *p3d, uint8_t *triangulated);

/*
 * ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778), LocalMapping::Run's call at src/LocalMapping.cc:82 ----
 * Many free vertices: the local key frames (VertexSE3Expmap) and the local points (VertexSBAPointXYZ, marginalised), joined by
 * EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with a Huber kernel, solved by BlockSolver_6_3's Schur complement over the points
 * under OptimizationAlgorithmLevenberg.  The g2o lines restated are listed in csrc/orbp_lba_body.h, the text the GPU call
 * orbm_local_bundle_adjustment (include/orbm.h) runs as well; the reduced system is dense here (6K x 6K for K local key frames,
 * Cholesky in fp64; a non-positive or non-finite pivot is "solve failed", optimization_algorithm_levenberg.cpp:126-127).
 * Parity with g2o itself is unpinned (there is no Eigen to build it against): Eigen's product and inverse evaluation order, the
 * elimination order of its sparse LDL^T, and the order of the unknowns (g2o: by vertex id; here: problem order).
 *
 * The problem is flat and gathered exactly as :455-653 walks:
 *   n_local key frames in lLocalKeyFrames order (:456-468), local_fixed[i] != 0 for mnId == 0 (:529);
 *   n_fixed key frames in lFixedCameras order (:489-504);
 *   n_points points in lLocalMapPoints order (:471-486);
 *   edges in CSR by point: point p owns the edges edge_off[p] .. edge_off[p + 1], in the order its observations map is iterated
 *   (:585), skipping bad key frames (:589).  This is g2o's active-edge order and the host path's summation order.
 *   Per edge: edge_kf = the key frame's index into local-then-fixed, obs = kpUn.pt (2 floats), u_right = mvuRight (< 0: monocular,
 *   :594), inv_sigma2 = mvInvLevelSigma2[kpUn.octave].  A point holds a key frame at most once, as the map does.
 *   Per key frame (local, then fixed): Tcw = GetPose() (row-major 4 x 4 floats) and cam = {fx, fy, cx, cy, mbf}.
 * Outputs: Tcw_local (16 floats per local key frame) = Converter::toCvMat(SE3Quat) (:767); xw (3 floats per point, in = GetWorldPos(),
 * out = :775); erase[e] = 1 where :715-743 pushes the edge's pair into vToErase; stats (may be NULL).
 *
 * Kept from the reference:
 *   rounds: optimize(5), then the flagging pass :672-702 (chi2 > 5.991 / 7.815 on the double chi2(), or depth not positive, sets
 *     level 1; every edge loses its robust kernel), then initializeOptimization(0) and optimize(10) from iteration 0 again;
 *   stale errors: the final pass reads chi2() from the error the edge last stored while active (for a level-1 edge: the first
 *     round's last computeActiveErrors, a rejected trial's included); isDepthPositive() is evaluated at the final estimates;
 *   a point or key frame whose every edge is level 1 leaves the second round and keeps the first round's bits;
 *   an edge to a fixed key frame (a fixed one, or a local one with mnId == 0) contributes to its point's blocks only;
 *   stop (may be NULL): set at entry (:655-657) -> returns ORBP_LBA_STOPPED with no output written; otherwise read at the top of
 *     every iteration and in the do ... while of the trial loop; set after the first optimize (:664-666) -> the second round is
 *     skipped, the final pass and the write-back still run.
 * Returns ORBP_LBA_DONE, ORBP_LBA_STOPPED, or ORBX_E_INVALID before any work on: a NULL pointer, a negative count, an edge_kf out
 * of range or twice in a point, edge_off[0] != 0 or not monotone, a non-finite pose, point, calibration, observation or inv_sigma2.
 * A problem without edges optimises nothing and returns ORBP_LBA_DONE (poses and points written back as the reference would).  With
 * every key frame fixed the points alone are optimised.
 */
typedef struct orbp_lba_problem {
    int32_t n_local, n_fixed, n_points;
    const uint8_t *local_fixed;     /* n_local */
    const float *Tcw;               /* 16 * (n_local + n_fixed) */
    const float *cam;               /* 5 * (n_local + n_fixed) */
    const int32_t *edge_off;        /* n_points + 1 */
    const int32_t *edge_kf;         /* per edge */
    const float *obs;               /* 2 per edge */
    const float *u_right;           /* per edge */
    const float *inv_sigma2;        /* per edge */
} orbp_lba_problem;
typedef struct orbp_lba_stats {
    int32_t iterations[2], trials[2];   /* of optimize(5) and optimize(10): iterations run, Levenberg trials in them */
    double lambda, chi2;                /* _currentLambda and the active robust chi2 after the last optimize that ran */
    int32_t n_level1, second_round;     /* edges set to level 1 at :672-702; 1 when that pass and optimize(10) were reached */
} orbp_lba_stats;
enum { ORBP_LBA_DONE = 0, ORBP_LBA_STOPPED = 1 };
int orbp_local_bundle_adjustment(const orbp_lba_problem *p, float *Tcw_local, float *xw, uint8_t *erase,
                                 const volatile uint8_t *stop, orbp_lba_stats *stats);

/*
 * ---- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:41-237) ----
 * The calls at src/Tracking.cc:695 (CreateInitialMapMonocular, 20 iterations) and src/LoopClosing.cc:651
 * (RunGlobalBundleAdjustment, 10 iterations, not robust).  The same vertices, edges, Schur complement and Levenberg loop as
 * LocalBundleAdjustment above (csrc/orbp_lba_body.h, which orbm_bundle_adjustment of include/orbm.h runs as well), under a
 * different graph walk.  This host path keeps the reduced system dense (Cholesky of 6K x 6K, time growing with (6K)^3): it is
 * meant for the initial map and for machines without a GPU.  Parity with g2o itself is unpinned, as above.
 *
 * The problem is an orbp_lba_problem gathered as :71-184 walks:
 *   the "local" key frames are the non-bad vpKFs in order (:71-83), local_fixed[i] != 0 for mnId == 0 (:79); n_fixed is
 *   normally 0 and stays legal (key frames that only constrain points);
 *   the points are the non-bad vpMP in order (:89-99);
 *   a point's edges in the order GetObservations() iterates (:105), skipping bad key frames and mnId > maxKFid (:109).
 * Outputs: Tcw_local = Converter::toCvMat(SE3Quat) of every local key frame (:199-209), xw (in = GetWorldPos(), out = :222-233).
 *
 * Kept from the reference:
 *   one round: optimize(n_iterations) (:187-188) is all; no level-1 pass, no second round, no erase list;
 *   robust != 0: RobustKernelHuber with sqrt(5.99) / sqrt(7.815) held as floats (:85-86; LocalBundleAdjustment has 5.991);
 *     robust == 0: no kernel, rho is chi2 and the weight 1 (:129, :158);
 *   stop (may be NULL) has no entry check (LocalBundleAdjustment has :655): it is read at the top of every iteration
 *     (sparse_optimizer.cpp:376) and in the do ... while of the trial loop (optimization_algorithm_levenberg.cpp:149);
 *   stop set before the first read: no iteration runs, the call returns 0, the poses come back after the toSE3Quat -> toCvMat
 *     round trip and the points after float -> double -> float;
 *   a point without edges (:175-179, vbNotIncludedMP) keeps its xw bits;
 *   a key frame without edges keeps its round-tripped pose (its block of the reduced system is the identity);
 *   n_iterations: 0 optimises nothing; above ORBP_BA_MAX_ITERATIONS -> ORBX_E_INVALID (the callers pass 20 and 10);
 *   the fork's _nBad stop (optimization_algorithm_levenberg.cpp:154-161) applies.
 * Returns 0, or ORBX_E_INVALID before any work on what orbp_local_bundle_adjustment refuses, a negative n_iterations or one
 * above the bound.  stats (may be NULL): iterations run, Levenberg trials in them, _currentLambda and the active (robust) chi2.
 */
#define ORBP_BA_MAX_ITERATIONS 100
typedef struct orbp_ba_stats {
    int32_t iterations, trials;
    double lambda, chi2;
} orbp_ba_stats;
int orbp_bundle_adjustment(const orbp_lba_problem *p, int n_iterations, int robust, float *Tcw_local, float *xw,
                           const volatile uint8_t *stop, orbp_ba_stats *stats);

/*
 * ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044), LoopClosing::CorrectLoop's call at src/LoopClosing.cc:568 ----
 * A pose graph: one VertexSim3Expmap per key frame, EdgeSim3 with identity information and no robust kernel between them, numeric
 * Jacobians (delta = 1e-9), BlockSolver_7_3 on Hpp alone (no landmarks, no Schur complement) under OptimizationAlgorithmLevenberg
 * with setUserLambdaInit(1e-16), so the first lambda is 1e-16 and not tau * maxdiag.  The g2o lines restated are listed in
 * csrc/orbp_eg_body.h, the text the GPU call orbm_optimize_essential_graph (include/orbm.h) runs as well; the Levenberg loop is
 * LocalBundleAdjustment's (csrc/orbp_lm_body.h).  Parity with g2o itself is unpinned (there is no Eigen to build it against).
 *
 * The problem is flat:
 *   n_kfs key frames in g2o's hessianIndex order (mnId ascending); Scw[8 i ..] = vScw[i] (:818-832) and Snc[8 i ..] = the key
 *   frame's NonCorrectedSim3 where it has one, else a copy of Scw, both in Sim3::operator[] order qx qy qz qw tx ty tz s;
 *   fixed = the index of pLoopKF (:834), or -1; fix_scale = bFixScale (:839);
 *   n_edges edges in insertion order (:852-983): vertex 0 is edge_i, vertex 1 is edge_j; edge_corrected[e] = 1 where the
 *   measurement is Scw_j * Scw_i^-1 (the LoopConnections edges, :857-867), 0 where it is Snc_j * Snc_i^-1 (:889-972);
 *   n_points points: xw (3 floats each, in = GetWorldPos()) and ref[p] = the index of the key frame of :1020-1029, or -1.
 * Outputs: Tcw (16 floats per key frame) = [R | t / s] of the optimised Sim3 (:999-1009, the fixed key frame's too); xw =
 * correctedSwr.map(Srw.map(P)) (:1032-1040) with Srw from the input Scw; Scw_out (may be NULL; 8 doubles per key frame) = the
 * optimised Sim3; stats (may be NULL).
 *
 * Kept from the reference: optimize(n_iterations) (the reference passes 20) with the fork's _nBad stop; a quaternion is never
 * normalised; under fix_scale the seventh update of every vertex is exactly zero and the scales keep their bits.
 * Chosen here: a key frame without edges stays in the system (its pivot is lambda, its update exactly zero) where g2o leaves it
 * out of the active set; a failed solve leaves the update zero.  Two deviations the adapter (host/PnPsolver.h) relies on: a bad
 * key frame is not part of the problem, and neither is any edge that would touch it (the reference would dereference a null
 * vertex); a point with ref = -1 (its reference key frame has no vertex) keeps its position's bits (the reference maps it through
 * two identities).
 * The linear solve is an envelope (skyline) Cholesky in fp64: row r of the 7N x 7N system is stored from its first structural
 * nonzero column, and every sum runs in the order of the dense factorisation of csrc/orbp_lba_host.h, so the result is the dense
 * one's bit for bit at the cost of the sum of the squared row widths.  There is no cap on n_kfs.
 * Returns 0, or ORBX_E_INVALID before any work on: a NULL pointer, a negative count, n_iterations outside
 * [0, ORBP_BA_MAX_ITERATIONS], fixed, an edge end or a ref out of range, edge_i == edge_j, a non-finite Sim3 or a scale <= 0.
 */
typedef struct orbp_eg_problem {
    int32_t n_kfs;
    const double *Scw, *Snc;            /* 8 * n_kfs each */
    int32_t fixed, fix_scale;
    int32_t n_edges;
    const int32_t *edge_i, *edge_j;     /* per edge */
    const uint8_t *edge_corrected;      /* per edge */
    int32_t n_points;
    const int32_t *ref;                 /* per point */
} orbp_eg_problem;
typedef struct orbp_eg_stats {
    int32_t iterations, trials;         /* iterations run, Levenberg trials in them */
    double lambda;                      /* _currentLambda */
    double chi2_initial, chi2_final;    /* the active chi2 at the input estimates and at the output's */
} orbp_eg_stats;
int orbp_optimize_essential_graph(const orbp_eg_problem *p, int n_iterations, float *Tcw, float *xw, double *Scw_out,
                                  orbp_eg_stats *stats);
const char *orbp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
