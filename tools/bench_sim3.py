#!/usr/bin/env python3
"""Cost of the Sim3Solver RANSAC of LoopClosing::ComputeSim3 for K candidate key frames: every hypothesis on the host
(orbp_sim3_iterate, include/orbp.h) against all candidates' hypotheses in one GPU call (orbm_sim3_hypotheses, include/orbm.h)
followed by the replay, on one GPU.

Workload: tests/sim3_cases.py make_case(N, seed): a planted similarity, two cameras, a quarter of the N correspondences outliers (none below N = 63).
SetRansacParameters(1 - 1e-12, 20, 300): the probability is raised so that mRansacMaxIts is 300 at every N (with 0.99 it is 70 at
N = 50), and both sides run all 300 iterations of every solver: iterate() is called again after a returned pose until bNoMore, as
ComputeSim3 does when OptimizeSim3 rejects the pose.  Both sides do the same work: K * 300 hypotheses over N correspondences.
Per (K, N), medians over --reps rounds after --warmup rounds on a warm handle, the two sides alternating inside a round, the C calls
alone on a host clock (the GPU call ends in its own synchronisation):
  host_ms    per solver: set_ransac_parameters, then iterate(300) until bNoMore (draws and evaluation inside)
  gpu_ms     per solver: set_ransac_parameters and orbp_sim3_draw(300) straight into the batch's triple array; ONE
             orbm_sim3_hypotheses (one staged upload, one launch, one download, one synchronisation); per solver attach_results
             and iterate(300) until bNoMore (the replay)
  gpu_call_ms  the orbm_sim3_hypotheses call of that round alone
Before anything is timed the replayed run is compared with the host run on scripted draws: same calls, poses, flags, counts.
The numbers are what one run measured.

usage: tools/bench_sim3.py [--candidates 1,5,20] [--sizes 50,150,400] [--reps 30] [--warmup 5] [--out profiles/sim3_batch.json]
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
import sim3_cases as sc  # noqa: E402

PROB, MIN_INLIERS, MAX_ITS = 1 - 1e-12, 20, 300


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
    cases = [sc.make_case(N, 9000 + 31 * k + N, False) for k in range(K)]

    def solvers(scripted):
        out = []
        for c in cases:
            s = pkg.Sim3Solver(c["x1"], c["x2"], c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"], False,
                               rand=sc.Lcg(c["seed"]) if scripted else None, rand_max=sc.RAND_MAX)
            out.append(s)
        return out

    def chk(rc, err):
        if rc < 0:
            raise SystemExit("status %d: %s" % (rc, err().decode()))
        return rc

    # the static part of the batch; the triples are drawn into `tri` at every round
    probe = solvers(False)
    for s in probe:
        s.SetRansacParameters(PROB, MIN_INLIERS, MAX_ITS)
        assert s.ransac_state()["max_its"] == MAX_ITS
    off, x1, x2, e1, e2, cams, hyp_off, tri, mask_off = pkg.ORBmatcher.pack_sim3_problems(
        [s.problem()[:7] + (np.zeros((MAX_ITS, 3), np.int32),) for s in probe])
    H, MW, W = int(hyp_off[-1]), int(mask_off[-1]), (N + 31) // 32
    cnt, sRt, masks = np.zeros(H, np.int32), np.zeros((H, 13), np.float32), np.zeros(MW, np.uint32)
    inl, T = np.zeros(N + 1, np.uint8), np.zeros(16, np.float32)
    no_more, ninl = C.c_int(), C.c_int()
    tri_ptr = [C.c_void_p(tri.ctypes.data + 12 * int(hyp_off[k])) for k in range(K)]
    cnt_ptr = [C.c_void_p(cnt.ctypes.data + 4 * int(hyp_off[k])) for k in range(K)]
    sRt_ptr = [C.c_void_p(sRt.ctypes.data + 52 * int(hyp_off[k])) for k in range(K)]
    mask_ptr = [C.c_void_p(masks.ctypes.data + 4 * int(mask_off[k])) for k in range(K)]
    pi, pT = p(inl), p(T)

    def iterate_all(s, trace=None):
        poses = 0
        while True:
            got = chk(L.orbp_sim3_iterate(s.h, MAX_ITS, C.byref(no_more), pi, C.byref(ninl), pT), L.orbp_last_error)
            poses += got
            if trace is not None:
                trace.append((got, no_more.value, ninl.value, T.tobytes() if got else b"", inl[:N].tobytes()))
            if no_more.value:
                return poses

    def host_side(ss, trace=None):
        n = 0
        for s in ss:
            L.orbp_sim3_set_ransac_parameters(s.h, PROB, MIN_INLIERS, MAX_ITS)
            n += iterate_all(s, trace)
        return n

    call_ms = [0.0]

    def gpu_side(ss, trace=None):
        for k, s in enumerate(ss):
            L.orbp_sim3_set_ransac_parameters(s.h, PROB, MIN_INLIERS, MAX_ITS)
            if L.orbp_sim3_draw(s.h, MAX_ITS, tri_ptr[k]) != MAX_ITS:
                raise SystemExit("draw")
        t0 = time.perf_counter()
        chk(L.orbm_sim3_hypotheses(m.h, K, p(off), p(x1), p(x2), p(e1), p(e2), p(cams), p(hyp_off), p(tri), p(mask_off), p(cnt), p(sRt), p(masks)),
            L.orbm_last_error)
        call_ms[0] = (time.perf_counter() - t0) * 1e3
        n = 0
        for k, s in enumerate(ss):
            chk(L.orbp_sim3_attach_results(s.h, MAX_ITS, cnt_ptr[k], sRt_ptr[k], mask_ptr[k]), L.orbp_last_error)
            n += iterate_all(s, trace)
        return n

    # the same run on both sides, on scripted draws, before anything is timed
    ta, tb = [], []
    poses = host_side(solvers(True), ta)
    if gpu_side(solvers(True), tb) != poses or ta != tb:
        raise SystemExit("K=%d N=%d: the replayed run differs from the host run" % (K, N))

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
    return {"candidates": K, "correspondences_each": N, "hypotheses": H, "reps": reps, "warmup": warmup, "poses_returned": poses,
            "host_ms": h, "gpu_ms": g, "gpu_call_ms": float(np.median(tc)), "host_ms_min_max": [float(min(th)), float(max(th))],
            "gpu_ms_min_max": [float(min(tg)), float(max(tg))], "host_over_gpu": h / g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="1,5,20")
    ap.add_argument("--sizes", default="50,150,400")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_batch.json"))
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
    doc = {"tool": "tools/bench_sim3.py",
           "workload": "tests/sim3_cases.py make_case: planted similarity, a quarter outliers; SetRansacParameters(1 - 1e-12, 20, 300), all 300 "
                       "iterations of every solver on both sides",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
