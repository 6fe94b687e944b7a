#!/usr/bin/env python3
"""Cost of the PnPsolver RANSAC of Tracking::Relocalization for K candidate key frames: every hypothesis on the host
(orbp_pnp_iterate, include/orbp.h) against all candidates' hypotheses in one GPU call (orbm_pnp_hypotheses, include/orbm.h)
followed by the replay, on one GPU.

Workload: tests/pnp_cases.py make_case(N, ...): a planted pose, points at 4 to 40 m, 0.5 px noise, 40 % wrong matches (30-80 px off).
Relocalization's SetRansacParameters(0.99, minInliers, 300, 4, 0.5, 5.991) with minInliers = 70 % of N, which no hypothesis reaches
(60 % of the matches are right), so no pose comes back, Refine never runs and every solver runs all its iterations on both sides.
The iteration count is that of a lost frame, 35: with epsilon = 0.5 (any candidate whose 50 % is above minInliers = 10) mRansacMaxIts
is 35 and the reference's `||` loop runs them all in the first iterate(5); here minInliers lowers mRansacMaxIts, and iterate(35) runs
35 iterations by the other side of the same `||`.  Both sides do the same work: K * 35 four-point EPnP solves, each checked against N
correspondences.
Per (K, N), medians over --reps rounds after --warmup rounds on a warm handle, the two sides alternating inside a round, the C calls
alone on a host clock (the GPU call ends in its own synchronisation):
  host_ms      per solver: set_ransac_parameters, then iterate(35) (draws and evaluation inside)
  gpu_ms       per solver: set_ransac_parameters and orbp_pnp_draw(35); the sets copied into the batch's array of stride 8; ONE
               orbm_pnp_hypotheses (one staged upload, one launch, one download, one synchronisation); per solver attach_results and
               iterate(35) (the replay)
  gpu_call_ms  the orbm_pnp_hypotheses call of that round alone
Before anything is timed the replayed run is compared with the host run on scripted draws: same return values, flags, counts.
The numbers are what one run measured.

usage: tools/bench_pnp.py [--candidates 1,5,20] [--sizes 50,150,400] [--reps 30] [--warmup 5] [--out profiles/pnp_batch.json]
"""
import argparse
import ctypes as C
import importlib.util
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_cases as pc  # noqa: E402

ITS, SET = 35, 4


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(pkg, m, K, N, reps, warmup):
    L = pkg.lib()
    cases = [pc.make_case("bench", N, SET, 7000 + 31 * k + N, noise=0.5, wrong=(2 * N) // 5, zmin=4.0, zmax=40.0) for k in range(K)]
    min_inliers = int(math.ceil(0.7 * N))
    prm = (C.c_double(0.99), min_inliers, 300, SET, C.c_float(0.5), C.c_float(5.991))

    def solvers(scripted):
        out = []
        for c in cases:
            fx, fy, cx, cy = (float(v) for v in c["K"])
            out.append(pkg.PnPsolver(c["p2d"], c["sigma2"], c["p3d"], fx, fy, cx, cy, rand=pc.Lcg(c["seed"]) if scripted else None,
                                     rand_max=pc.RAND_MAX))
        return out

    def chk(rc, err):
        if rc < 0:
            raise SystemExit("status %d: %s" % (rc, err().decode()))
        return rc

    # the static part of the batch; the samples are drawn at every round
    probe = solvers(False)
    for s in probe:
        s.SetRansacParameters(0.99, min_inliers, 300, SET, 0.5, 5.991)
        assert s.ransac_state()["max_its"] <= ITS
    off, p2d, p3d, e, cams, hyp_off, sm8, mask_off = pkg.ORBmatcher.pack_pnp_problems(
        [s.problem()[:5] + (np.zeros((ITS, SET), np.int32),) for s in probe])
    H, MW = int(hyp_off[-1]), int(mask_off[-1])
    sm4 = np.zeros((H, SET), np.int32)
    cnt, Rt, masks = np.zeros(H, np.int32), np.zeros((H, 12), np.float64), np.zeros(MW, np.uint32)
    inl, T = np.zeros(N + 1, np.uint8), np.zeros(16, np.float32)
    no_more, ninl = C.c_int(), C.c_int()
    sm_ptr = [C.c_void_p(sm4.ctypes.data + 4 * SET * int(hyp_off[k])) for k in range(K)]
    cnt_ptr = [C.c_void_p(cnt.ctypes.data + 4 * int(hyp_off[k])) for k in range(K)]
    Rt_ptr = [C.c_void_p(Rt.ctypes.data + 96 * int(hyp_off[k])) for k in range(K)]
    mask_ptr = [C.c_void_p(masks.ctypes.data + 4 * int(mask_off[k])) for k in range(K)]
    pi, pT = p(inl), p(T)

    def iterate_all(s, trace):
        got = chk(L.orbp_pnp_iterate(s.h, ITS, C.byref(no_more), pi, C.byref(ninl), pT), L.orbp_last_error)
        if trace is not None:
            trace.append((got, no_more.value, ninl.value, s.ransac_state()["iterations"]))
        return got

    def host_side(ss, trace=None):
        n = 0
        for s in ss:
            L.orbp_pnp_set_ransac_parameters(s.h, *prm)
            n += iterate_all(s, trace)
        return n

    call_ms = [0.0]

    def gpu_side(ss, trace=None):
        for k, s in enumerate(ss):
            L.orbp_pnp_set_ransac_parameters(s.h, *prm)
            if L.orbp_pnp_draw(s.h, ITS, sm_ptr[k]) != ITS:
                raise SystemExit("draw")
        sm8[:, :SET] = sm4
        t0 = time.perf_counter()
        chk(L.orbm_pnp_hypotheses(m.h, K, p(off), p(p2d), p(p3d), p(e), p(cams), p(hyp_off), p(sm8), p(mask_off), p(cnt), p(Rt), p(masks)),
            L.orbm_last_error)
        call_ms[0] = (time.perf_counter() - t0) * 1e3
        n = 0
        for k, s in enumerate(ss):
            chk(L.orbp_pnp_attach_results(s.h, ITS, cnt_ptr[k], Rt_ptr[k], mask_ptr[k]), L.orbp_last_error)
            n += iterate_all(s, trace)
        return n

    # the same run on both sides, on scripted draws, before anything is timed; the counts of the hypotheses as well
    ta, tb = [], []
    poses = host_side(solvers(True), ta)
    if gpu_side(solvers(True), tb) != poses or ta != tb or poses != 0:
        raise SystemExit("K=%d N=%d: the replayed run differs from the host run, or a pose came back" % (K, N))
    ref = solvers(True)
    for k, s in enumerate(ref):
        s.SetRansacParameters(0.99, min_inliers, 300, SET, 0.5, 5.991)
        want = s.hypotheses(sm4[int(hyp_off[k]):int(hyp_off[k + 1])])
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        if want[0].tobytes() != cnt[h0:h1].tobytes() or want[1].tobytes() != Rt[h0:h1].tobytes() or \
                want[2].tobytes() != masks[int(mask_off[k]):int(mask_off[k + 1])].tobytes():
            raise SystemExit("K=%d N=%d: the GPU results differ from orbp_pnp_hypothesis" % (K, N))

    a, b = solvers(False), solvers(False)
    th, tg, tc = [], [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        host_side(a)
        t1 = time.perf_counter()
        gpu_side(b)
        t2 = time.perf_counter()
        if i >= warmup:
            th.append((t1 - t0) * 1e3); tg.append((t2 - t1) * 1e3); tc.append(call_ms[0])
    h, g = float(np.median(th)), float(np.median(tg))
    return {"candidates": K, "correspondences_each": N, "hypotheses": H, "reps": reps, "warmup": warmup, "min_inliers": min_inliers,
            "host_ms": h, "gpu_ms": g, "gpu_call_ms": float(np.median(tc)), "host_ms_min_max": [float(min(th)), float(max(th))],
            "gpu_ms_min_max": [float(min(tg)), float(max(tg))], "host_over_gpu": h / g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="1,5,20")
    ap.add_argument("--sizes", default="50,150,400")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_batch.json"))
    args = ap.parse_args()
    pkg = _pkg()
    m = pkg.ORBmatcher(0.75, True)
    results = []
    for K in [int(v) for v in args.candidates.split(",")]:
        for N in [int(v) for v in args.sizes.split(",")]:
            r = run(pkg, m, K, N, args.reps, args.warmup)
            print("K=%-3d N=%-4d host %8.3f ms   one GPU call + replay %8.3f ms (the call %7.3f ms)   host/gpu %.2f" %
                  (K, N, r["host_ms"], r["gpu_ms"], r["gpu_call_ms"], r["host_over_gpu"]), flush=True)
            results.append(r)
    m.close()
    doc = {"tool": "tools/bench_pnp.py",
           "workload": "tests/pnp_cases.py make_case: planted pose, 40 % wrong matches; SetRansacParameters(0.99, 0.7 N, 300, 4, 0.5, 5.991), "
                       "iterate(35): all 35 iterations of every solver on both sides, no pose returned",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
