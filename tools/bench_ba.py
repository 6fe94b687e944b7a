#!/usr/bin/env python3
"""Cost of Optimizer::BundleAdjustment on the GPU (orbm_bundle_adjustment, include/orbm.h) against the host path
(orbp_bundle_adjustment, include/orbp.h), and of the many-workgroup solve of csrc/orbm_spd.hip against the one-workgroup
k_lba_solve it stands in for, on one GPU.  No assertion on time.

Shapes (key frames : points : n_iterations : robust), tests/ba_cases.py scene(): the key frame with mnId == 0 fixed, a point seen by
two key frames at least, a tenth gross outliers:
  2:150:20:1      the initial map of Tracking::CreateInitialMapMonocular (monocular)
  40:8000:10:0, 150:30000:10:0, 400:60000:10:0      LoopClosing::RunGlobalBundleAdjustment (stereo and monocular mixed)
Per shape, the C calls alone from the same host arrays, host clock: gpu_ms the median over --reps calls after --warmup on a warm
handle; host_ms likewise up to --host-median-kfs key frames, ONE call (host_calls = 1) up to --host-max-kfs, and not measured
beyond (host_ms = null): the host path's dense Cholesky grows with (6 K)^3.  These shapes are not held away from their decision
boundaries as the test cases are: whether the counts came out the same is recorded, not demanded.

Then one GPU call split by events (orbm_bundle_adjustment_split; the groups are bench_lba.py's, "solve" holding every launch of the
many-workgroup solve), the median of --split-reps calls by call time.

The solver alone (orbm_spd_solve_timed, an internal entry): A = G G^T + n I at n = 240, 768, 1800, 3072, the device routine timed
by events from a fresh device copy, the factorisation and the two substitutions apart, medians over --solve-reps.  Beside it, in
the same run, k_lba_solve's time per launch from orbm_local_bundle_adjustment_split at 40:40:8000 (n = 240) and 128:40:8000
(n = 768): the solver orbm_local_bundle_adjustment keeps.

usage: tools/bench_ba.py [--shapes ...] [--reps 10] [--warmup 2] [--split-reps 3] [--solve-sizes 240,768,1800,3072]
                         [--lba-shapes 40:40:8000,128:40:8000] [--out profiles/ba_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ba_cases as bc  # noqa: E402
import bench_lba  # noqa: E402
from bench_lba import SPLIT, p, timed  # noqa: E402


def run(pkg, m, n_kfs, n_points, n_it, robust, args):
    L = pkg.lib()
    t0 = time.perf_counter()
    pr = bc.scene(np.random.default_rng(n_points), n_free=n_kfs - 1, n_points=n_points, kinds="mono" if n_kfs == 2 else "mixed",
                  outliers=0.1, fixed_at=0)
    s, a = pkg.pack_lba_problem(pr)
    E = len(a["edge_kf"])
    print("scene %d:%d built in %.1f s, %d edges" % (n_kfs, n_points, time.perf_counter() - t0, E), flush=True)
    xw0 = a["xw"].copy()
    out = {side: dict(T=np.zeros((n_kfs, 16), np.float32), x=xw0.copy(), st=pkg.BaStats()) for side in ("host", "gpu")}

    def call(side):
        o = out[side]
        np.copyto(o["x"], xw0)
        if side == "host":
            rc = L.orbp_bundle_adjustment(C.byref(s), n_it, robust, p(o["T"]), p(o["x"]), None, C.byref(o["st"]))
        else:
            rc = L.orbm_bundle_adjustment(m.h, C.byref(s), n_it, robust, p(o["T"]), p(o["x"]), None, C.byref(o["st"]))
        if rc != 0:
            raise SystemExit("%s: status %d: %s" % (side, rc, (L.orbp_last_error() if side == "host" else L.orbm_last_error()).decode()))

    def split_call():
        o = out["gpu"]
        np.copyto(o["x"], xw0)
        ms, cnt = np.zeros(len(SPLIT), np.float64), np.zeros(len(SPLIT), np.int32)
        t0 = time.perf_counter()
        rc = L.orbm_bundle_adjustment_split(m.h, C.byref(s), n_it, robust, p(o["T"]), p(o["x"]), None, C.byref(o["st"]), p(ms), p(cnt))
        t1 = time.perf_counter()
        if rc != 0:
            raise SystemExit("split: status %d: %s" % (rc, L.orbm_last_error().decode()))
        return (t1 - t0) * 1e3, ms, cnt

    call("gpu")
    sg = out["gpu"]["st"].as_dict()
    res = dict(key_frames=n_kfs, points=n_points, edges=E, n_iterations=n_it, robust=bool(robust), unknowns_reduced=6 * n_kfs,
               reps=args.reps, warmup=args.warmup, iterations=sg["iterations"], trials=sg["trials"], chi2_gpu=sg["chi2"])
    res["gpu_ms"] = timed(lambda: call("gpu"), args.reps, args.warmup)
    res["gpu_ms_per_trial"] = res["gpu_ms"] / max(1, sg["trials"])
    if n_kfs <= args.host_max_kfs:
        t0 = time.perf_counter()
        call("host")
        first = (time.perf_counter() - t0) * 1e3
        if n_kfs <= args.host_median_kfs:
            res["host_ms"], res["host_calls"] = timed(lambda: call("host"), args.reps, args.warmup), args.reps
        else:
            res["host_ms"], res["host_calls"] = first, 1
        sh = out["host"]["st"].as_dict()
        res.update(host_over_gpu=res["host_ms"] / res["gpu_ms"], chi2_host=sh["chi2"],
                   same_counts=all(sh[k] == sg[k] for k in ("iterations", "trials")),
                   max_pose_difference=float(np.abs(out["host"]["T"] - out["gpu"]["T"]).max()),
                   max_point_difference=float(np.abs(out["host"]["x"] - out["gpu"]["x"]).max()))
    else:
        res["host_ms"], res["host_calls"] = None, 0
    whole = out["gpu"]["T"].tobytes() + out["gpu"]["x"].tobytes()
    runs = sorted((split_call() for _ in range(args.split_reps)), key=lambda r: r[0])
    res["split_same_bytes"] = whole == out["gpu"]["T"].tobytes() + out["gpu"]["x"].tobytes()
    t, ms, cnt = runs[len(runs) // 2]
    res["split_call_ms"] = t
    res["split_ms"] = {k: float(v) for k, v in zip(SPLIT, ms)}
    res["split_launches"] = {k: int(v) for k, v in zip(SPLIT, cnt)}
    res["split_device_ms"] = float(ms.sum())
    res["split_host_gap_ms"] = t - float(ms.sum())
    res["solve_ms_per_trial"] = float(ms[SPLIT.index("solve")]) / max(1, int(cnt[SPLIT.index("solve")]))
    return res


def solver(pkg, m, n, reps):
    L = pkg.lib()
    L.orbm_spd_solve_timed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.orbm_spd_solve_timed.restype = C.c_int
    rng = np.random.default_rng(n)
    G = rng.normal(size=(n, n))
    A, b = G @ G.T + n * np.eye(n), rng.normal(size=n)
    ms = np.zeros(2)
    if L.orbm_spd_solve_timed(m.h, p(A), p(b), n, reps, p(ms)) != 0:
        raise SystemExit("spd_solve_timed: %s" % L.orbm_last_error().decode())
    x, ok = m.spd_solve(A, b)
    err = float(np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))
    return dict(n=n, reps=reps, factor_ms=float(ms[0]), substitute_ms=float(ms[1]), spd_solve_ms=float(ms.sum()), ok=ok,
                backward_error=err, launches=5 * ((n + bc.NB - 1) // bc.NB) - 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:150:20:1,40:8000:10:0,150:30000:10:0,400:60000:10:0")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--split-reps", type=int, default=3)
    ap.add_argument("--host-median-kfs", type=int, default=40)
    ap.add_argument("--host-max-kfs", type=int, default=400)
    ap.add_argument("--solve-sizes", default="240,768,1800,3072")
    ap.add_argument("--solve-reps", type=int, default=10)
    ap.add_argument("--lba-shapes", default="40:40:8000,128:40:8000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_bench.json"))
    args = ap.parse_args()
    pkg = bench_lba._pkg()
    m = pkg.ORBmatcher(0.8, True)
    doc = {"tool": "tools/bench_ba.py", "what": "C calls from host arrays, host clock, ms; split_*: one GPU call by events; solver: device "
           "routine by events", "solver": [], "k_lba_solve": [], "rows": []}

    def save():
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=2)
            fh.write("\n")

    for n in (int(v) for v in args.solve_sizes.split(",") if v):
        doc["solver"].append(solver(pkg, m, n, args.solve_reps))
        print(json.dumps(doc["solver"][-1]), flush=True)
        save()
    for shape in (v for v in args.lba_shapes.split(",") if v):
        k, f, n = (int(v) for v in shape.split(":"))
        r = bench_lba.run(pkg, m, k, f, n, 0, 0, args.split_reps, medians=False)
        doc["k_lba_solve"].append(dict(shape=shape, n=6 * k, launches=r["split_launches"]["solve"], total_ms=r["split_ms"]["solve"],
                                       k_lba_solve_ms=r["split_ms"]["solve"] / max(1, r["split_launches"]["solve"])))
        print(json.dumps(doc["k_lba_solve"][-1]), flush=True)
        save()
    for shape in (v for v in args.shapes.split(",") if v):
        k, n, it, rb = (int(v) for v in shape.split(":"))
        doc["rows"].append(run(pkg, m, k, n, it, rb, args))
        print(json.dumps(doc["rows"][-1]), flush=True)
        save()
    m.close()


if __name__ == "__main__":
    main()
