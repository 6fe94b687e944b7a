// orbp_internal.h -- shared by the host solvers (orbp*.cc) and the GPU drivers that use their checks; nothing here is part of the C ABI of include/orbp.h.
#pragma once

// orbp.cc: sets the thread-local text that orbp_last_error() returns (not exported from liborbx.so)
__attribute__((visibility("hidden"))) void orbp_set_error(const char *text);

// orbp_sim3.cc, a hook for tests/test_sim3_cpu.py only: the elementary functions that orbm_sim3_body.h brings along.
// fn 0 = atan2(a, b) for a >= 0, 1 = sin(a), 2 = cos(a) for a in [0, 8].
extern "C" double orbp_sim3_math(int fn, double a, double b);

// orbp_lba.cc: the argument checks of orbp_local_bundle_adjustment, shared with orbm_local_bundle_adjustment (orbm_lba.hip).
// ORBX_OK, or ORBX_E_INVALID with its reason in text.
struct orbp_lba_problem;
__attribute__((visibility("hidden"))) int orbp_lba_check(const orbp_lba_problem *p, const float *Tcw_local, const float *xw,
                                                         const unsigned char *erase, char *text, int text_size);
// The one place where both paths read `stop`, and a hook for tests/test_lba_stop.py only: fn(arg), set per thread (NULL: none),
// is called just before every such read, so a test can set its flag between two given reads.  The reads of a call, in order:
// entry (:655-657); per iteration its top (sparse_optimizer.cpp:376) and, after each trial, the trial loop's condition where
// rho < 0 and fewer than 10 trials ran (optimization_algorithm_levenberg.cpp:149); after the first optimize (:662).
#include <stdint.h>
__attribute__((visibility("hidden"))) bool orbp_lba_read_stop(const volatile uint8_t *stop);
extern "C" void orbp_lba_set_stop_probe(void (*fn)(void *), void *arg);
// orbp_ba.cc: the argument checks of orbp_bundle_adjustment, shared with orbm_bundle_adjustment (orbm_lba.hip): those of
// orbp_lba_check and the bound of n_iterations.
__attribute__((visibility("hidden"))) int orbp_ba_check(const orbp_lba_problem *p, int n_iterations, const float *Tcw_local,
                                                        const float *xw, char *text, int text_size);
// orbp_eg.cc: the argument checks of orbp_optimize_essential_graph, shared with orbm_optimize_essential_graph (orbm_eg.hip).
struct orbp_eg_problem;
__attribute__((visibility("hidden"))) int orbp_eg_check(const orbp_eg_problem *p, int n_iterations, const float *Tcw, const float *xw,
                                                        char *text, int text_size);
// orbp_eg.cc, a hook for tests/test_eg_cpu.py only: dense != 0 makes every row of the envelope start at column 0 (per thread),
// which is the dense factorisation the envelope must reproduce bit for bit.
extern "C" void orbp_eg_set_dense(int dense);
