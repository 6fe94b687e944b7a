#!/usr/bin/env python3
"""Cost of Optimizer::OptimizeEssentialGraph on the GPU (orbm_optimize_essential_graph, include/orbm.h) against the host path
(orbp_optimize_essential_graph, include/orbp.h, an envelope Cholesky) on one GPU.  No assertion on time.

Shapes: 20, 50, 200 and 438 (ORBM_EG_MAX_KFS) key frames, tests/eg_cases.py graph(): a chain (the spanning tree) plus a covisibility band
of 10 plus one loop of 10 LoopConnections edges from the last ten key frames to the first ten, the first key frame fixed, the last
ten corrected by a Sim3 of 0.3 rad, scale 1.1 and 2 units; n_iterations = 20, as the reference asks.  Per shape, the C calls alone
from the same host arrays, host clock: gpu_ms and host_ms the medians over --reps calls after --warmup on a warm handle.  These
shapes are not held away from their decision boundaries as the test cases are: whether the counts came out the same is recorded,
not demanded.

Then one GPU call split by events (orbm_optimize_essential_graph_split; the groups are ORBM_EG_SPLIT_* of include/orbm.h), the
median of --split-reps calls by call time.

usage: tools/bench_eg.py [--sizes 20,50,200,438] [--reps 5] [--warmup 1] [--split-reps 3] [--out profiles/eg_bench.json]
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
import eg_cases as ec  # noqa: E402
import bench_lba  # noqa: E402
from bench_lba import p, timed  # noqa: E402

SPLIT = ("upload", "linearize", "assemble", "stage", "solve", "update_errors", "read_back", "output")    # ORBM_EG_SPLIT_*


def run(pkg, m, n, n_it, args):
    L = pkg.lib()
    pr = ec.graph(seed=n, n=n, fixed=0, corrected_from=n - 10, band=10, loop_connections=tuple((n - 1 - k, k) for k in range(10)))
    s, a = pkg.pack_eg_problem(pr)
    E = len(a["edge_i"])
    out = {side: dict(T=np.zeros((n, 16), np.float32), S=np.zeros((n, 8)), st=pkg.EgStats()) for side in ("host", "gpu")}

    def call(side):
        o = out[side]
        if side == "host":
            rc = L.orbp_optimize_essential_graph(C.byref(s), n_it, p(o["T"]), None, p(o["S"]), C.byref(o["st"]))
        else:
            rc = L.orbm_optimize_essential_graph(m.h, C.byref(s), n_it, p(o["T"]), None, p(o["S"]), C.byref(o["st"]))
        if rc != 0:
            raise SystemExit("%s: status %d: %s" % (side, rc, (L.orbp_last_error() if side == "host" else L.orbm_last_error()).decode()))

    def split_call():
        o = out["gpu"]
        ms, cnt = np.zeros(len(SPLIT), np.float64), np.zeros(len(SPLIT), np.int32)
        t0 = time.perf_counter()
        rc = L.orbm_optimize_essential_graph_split(m.h, C.byref(s), n_it, p(o["T"]), None, p(o["S"]), C.byref(o["st"]), p(ms), p(cnt))
        t1 = time.perf_counter()
        if rc != 0:
            raise SystemExit("split: status %d: %s" % (rc, L.orbm_last_error().decode()))
        return (t1 - t0) * 1e3, ms, cnt

    call("gpu")
    call("host")
    sg, sh = out["gpu"]["st"].as_dict(), out["host"]["st"].as_dict()
    res = dict(key_frames=n, edges=E, unknowns=7 * (n - 1), n_iterations=n_it, reps=args.reps, warmup=args.warmup,
               iterations=sg["iterations"], trials=sg["trials"], chi2_initial=sg["chi2_initial"], chi2_gpu=sg["chi2_final"],
               chi2_host=sh["chi2_final"], same_counts=all(sh[k] == sg[k] for k in ("iterations", "trials")),
               host_iterations=sh["iterations"], host_trials=sh["trials"],
               max_sim3_difference=float(np.abs(out["host"]["S"] - out["gpu"]["S"]).max()))
    res["gpu_ms"] = timed(lambda: call("gpu"), args.reps, args.warmup)
    res["host_ms"] = timed(lambda: call("host"), args.reps, args.warmup)
    res["gpu_ms_per_trial"] = res["gpu_ms"] / max(1, sg["trials"])
    res["host_ms_per_trial"] = res["host_ms"] / max(1, sh["trials"])
    res["host_over_gpu"] = res["host_ms"] / res["gpu_ms"]
    whole = out["gpu"]["T"].tobytes() + out["gpu"]["S"].tobytes()
    runs = sorted((split_call() for _ in range(args.split_reps)), key=lambda r: r[0])
    res["split_same_bytes"] = whole == out["gpu"]["T"].tobytes() + out["gpu"]["S"].tobytes()
    t, ms, cnt = runs[len(runs) // 2]
    res["split_call_ms"] = t
    res["split_ms"] = {k: float(v) for k, v in zip(SPLIT, ms)}
    res["split_launches"] = {k: int(v) for k, v in zip(SPLIT, cnt)}
    res["split_device_ms"] = float(ms.sum())
    res["split_host_gap_ms"] = t - float(ms.sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,50,200,438")
    ap.add_argument("--n-iterations", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--split-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eg_bench.json"))
    args = ap.parse_args()
    pkg = bench_lba._pkg()
    m = pkg.ORBmatcher(0.8, True)
    doc = {"tool": "tools/bench_eg.py", "what": "C calls from host arrays, host clock, ms; split_*: one GPU call by events", "rows": []}
    for n in (int(v) for v in args.sizes.split(",") if v):
        doc["rows"].append(run(pkg, m, n, args.n_iterations, args))
        print(json.dumps(doc["rows"][-1]), flush=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=2)
            fh.write("\n")
    m.close()


if __name__ == "__main__":
    main()
