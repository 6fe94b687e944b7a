// orbp_internal.h -- shared by orbp.cc, orbp_sim3.cc and orbp_init.cc; nothing here is part of the C ABI of include/orbp.h.
#pragma once

// orbp.cc: sets the thread-local text that orbp_last_error() returns (not exported from liborbx.so)
__attribute__((visibility("hidden"))) void orbp_set_error(const char *text);

// orbp_sim3.cc, a hook for tests/test_sim3_cpu.py only: the elementary functions that orbm_sim3_body.h brings along.
// fn 0 = atan2(a, b) for a >= 0, 1 = sin(a), 2 = cos(a) for a in [0, 8].
extern "C" double orbp_sim3_math(int fn, double a, double b);
