#!/usr/bin/env python3
"""Cost of one Initializer::Initialize (Tracking::MonocularInitialization) of 200 iterations: the all-host path of this library
(orbp_init_*, include/orbp.h) against the draws + two GPU calls + the replayed walks (orbm_init_hypotheses, orbm_init_check_rt,
include/orbm.h), on one GPU.

Workload: tests/initializer_cases.py make_case("general", N, ...): a planted motion, points in a volume, 0.25 px noise, a fifth of
the matches wrong, N / 4 + 3 keys without a match in either frame; 200 sets, so 400 hypotheses (200 homographies, 200 fundamental
matrices), each an 8-point solve and a pass over all N matches, then the 4 CheckRT passes of ReconstructF.  Both sides do the same
work and return the same bytes (compared on scripted draws before anything is timed).
Per N, medians over --reps rounds after --warmup rounds on a warm handle, the two sides alternating inside a round, the C calls
alone on a host clock (each GPU call ends in its own synchronisation):
  host_ms       set_current, draw, initialize (both walks, the motions, every CheckRT and the rules in place)
  gpu_ms        set_current, draw, get_problem; ONE orbm_init_hypotheses; attach_results, plan_check_rt (the walks as a replay, the
                motions); ONE orbm_init_check_rt; attach_check_rt; initialize (the rules)
  gpu_calls_ms  the two GPU calls of that round alone (hypotheses_ms + check_rt_ms)
The numbers are what one run measured.

usage: tools/bench_init.py [--sizes 100,300,1000] [--reps 30] [--warmup 5] [--out profiles/init_batch.json]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import initializer_cases as ic  # noqa: E402

ITS = 200


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(pkg, m, N, reps, warmup):
    L = pkg.lib()
    case = ic.make_case("general", N, 9000 + N)
    keys2, m12 = np.ascontiguousarray(case["keys2"]), np.ascontiguousarray(case["matches12"])
    n1, n2 = case["n1"], case["n2"]
    H, W = 2 * ITS, (N + 31) // 32

    def chk(rc, err):
        if rc < 0:
            raise SystemExit("status %d: %s" % (rc, err().decode()))
        return rc

    def solver(scripted):
        return pkg.Initializer(case["keys1"], ic.K, ic.SIGMA, ITS, rand=ic.Lcg(case["seed"]) if scripted else None, rand_max=ic.RAND_MAX)

    R, t, P, tri = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros((n1, 3), np.float32), np.zeros(n1 + 1, np.uint8)
    uv, pn, params = np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros(24, np.float32)
    sets, models = np.zeros((H, 8), np.int32), np.repeat(np.array([0, 1], np.int32), ITS)
    off, hyp_off, mask_off = np.array([0, N], np.int32), np.array([0, H], np.int32), np.array([0, H * W], np.int64)
    sm, cnt, masks = np.zeros((H, 10), np.float32), np.zeros(H, np.int32), np.zeros(H * W + 1, np.uint32)
    M, Rt, inl = np.zeros(9, np.float32), np.zeros((8, 12), np.float32), np.zeros(N + 1, np.uint8)
    status, cosp, p3d = np.zeros(8 * N, np.uint8), np.zeros(8 * N, np.float32), np.zeros(24 * N, np.float32)
    model, nm = C.c_int(), C.c_int()

    def host_side(s):
        chk(L.orbp_init_set_current(s.h, p(keys2), n2, p(m12)), L.orbp_last_error)
        chk(L.orbp_init_draw(s.h, None), L.orbp_last_error)
        return chk(L.orbp_init_initialize(s.h, p(R), p(t), p(P), p(tri)), L.orbp_last_error)

    calls = [0.0, 0.0]

    def gpu_side(s):
        chk(L.orbp_init_set_current(s.h, p(keys2), n2, p(m12)), L.orbp_last_error)
        chk(L.orbp_init_draw(s.h, None), L.orbp_last_error)
        chk(L.orbp_init_get_problem(s.h, p(uv), p(pn), p(params), p(sets), None, None), L.orbp_last_error)
        sets[ITS:] = sets[:ITS]
        t0 = time.perf_counter()
        chk(L.orbm_init_hypotheses(m.h, 1, p(off), p(uv), p(pn), p(params), p(hyp_off), p(sets), p(models), p(mask_off), p(sm), p(cnt),
                                   p(masks)), L.orbm_last_error)
        calls[0] = (time.perf_counter() - t0) * 1e3
        chk(L.orbp_init_attach_results(s.h, H, p(sm), p(cnt), p(masks)), L.orbp_last_error)
        k = chk(L.orbp_init_plan_check_rt(s.h, C.byref(model), p(M), p(inl), p(Rt), C.byref(nm)), L.orbp_last_error)
        calls[1] = 0.0
        if k:
            t0 = time.perf_counter()
            chk(L.orbm_init_check_rt(m.h, N, p(uv), p(inl), C.c_void_p(params.ctypes.data + 4 * 19), C.c_float(float(params[23])), k, p(Rt),
                                     p(status), p(cosp), p(p3d)), L.orbm_last_error)
            calls[1] = (time.perf_counter() - t0) * 1e3
            chk(L.orbp_init_attach_check_rt(s.h, k, p(Rt), p(inl), p(status), p(cosp), p(p3d)), L.orbp_last_error)
        return chk(L.orbp_init_initialize(s.h, p(R), p(t), p(P), p(tri)), L.orbp_last_error)

    # the same run on both sides, on scripted draws, before anything is timed
    ok_h = host_side(solver(True))
    want = (R.tobytes(), t.tobytes(), P.tobytes(), tri.tobytes())
    for a in (R, t, P, tri):
        a[...] = 0
    ok_g = gpu_side(solver(True))
    if ok_h != 1 or ok_g != 1 or want != (R.tobytes(), t.tobytes(), P.tobytes(), tri.tobytes()):
        raise SystemExit("N=%d: the GPU run differs from the host run, or nothing was initialised (%d, %d)" % (N, ok_h, ok_g))

    a, b = solver(False), solver(False)
    th, tg, tc, t1s, t2s = [], [], [], [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        host_side(a)
        t1 = time.perf_counter()
        gpu_side(b)
        t2 = time.perf_counter()
        if i >= warmup:
            th.append((t1 - t0) * 1e3); tg.append((t2 - t1) * 1e3); tc.append(calls[0] + calls[1]); t1s.append(calls[0]); t2s.append(calls[1])
    h, g = float(np.median(th)), float(np.median(tg))
    return {"matches": N, "keys_per_frame": n1, "iterations": ITS, "hypotheses": H, "reps": reps, "warmup": warmup, "host_ms": h, "gpu_ms": g,
            "gpu_calls_ms": float(np.median(tc)), "hypotheses_ms": float(np.median(t1s)), "check_rt_ms": float(np.median(t2s)),
            "host_ms_min_max": [float(min(th)), float(max(th))], "gpu_ms_min_max": [float(min(tg)), float(max(tg))], "host_over_gpu": h / g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,300,1000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_batch.json"))
    args = ap.parse_args()
    pkg = _pkg()
    m = pkg.ORBmatcher(0.9, True)
    results = []
    for N in [int(v) for v in args.sizes.split(",")]:
        r = run(pkg, m, N, args.reps, args.warmup)
        print("N=%-5d host %8.3f ms   draws + two GPU calls + replay %8.3f ms (the calls %7.3f ms = %.3f + %.3f)   host/gpu %.2f" %
              (N, r["host_ms"], r["gpu_ms"], r["gpu_calls_ms"], r["hypotheses_ms"], r["check_rt_ms"], r["host_over_gpu"]), flush=True)
        results.append(r)
    m.close()
    doc = {"tool": "tools/bench_init.py",
           "workload": "tests/initializer_cases.py make_case('general', N): planted motion, a fifth of the matches wrong; one Initialize of "
                       "200 iterations = 400 hypotheses + 4 CheckRT passes, the same bytes on both sides",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
