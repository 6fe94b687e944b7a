#!/usr/bin/env python3
"""Cost of Optimizer::LocalBundleAdjustment on the GPU (orbm_local_bundle_adjustment, include/orbm.h) against the host path
(orbp_local_bundle_adjustment, include/orbp.h), on one GPU.  No assertion on time: both sides are new code.

Workload: tests/lba_cases.py scene() at three shapes of the kind the reference meets (local key frames : fixed key frames : points):
5:5:500, 15:20:2500 and 40:40:8000, every point seen by three key frames at least (about 5.5 to 6 observations a point: about
2 750, 15 000 and 48 000 edges), stereo and monocular observations mixed, a tenth gross outliers, so both rounds run.  Per shape,
medians over --reps calls after --warmup calls on a warm handle, the C calls alone from the same host arrays, host clock:
  host_ms     orbp_local_bundle_adjustment
  gpu_ms      orbm_local_bundle_adjustment (one staged upload, the host-driven Levenberg loop with one 64-byte read-back a trial,
              one download)
with the iteration and trial counts.  These shapes are not held away from their decision boundaries as the test cases are: whether
flags and counts came out the same on both sides is recorded, not demanded.

Then the split of one GPU call by events (orbm_local_bundle_adjustment_split, include/orbm.h): per group of launches its device time
summed over the call and the number of times it ran, the k_lba_reduce_out + 64-byte copy step the host waits for among them; the
call's host-clock time; and split_host_gap_ms = that time minus the sum of the groups, which is what the host spends outside the
device's work: building the key-frame CSR, enqueueing, and per synchronisation the wake-up after the copy and the decision.  Divided
by the number of synchronisations (split_syncs) it is the cost of one synchronisation as the launch structure pays it.  The median of
--split-reps such calls (by call time) is recorded.

--cap-shape runs one more shape at ORBM_LBA_MAX_LOCAL local key frames for the split alone (no medians): what the single-workgroup
solve costs at the largest system the GPU call accepts.

usage: tools/bench_lba.py [--shapes 5:5:500,15:20:2500,40:40:8000] [--reps 30] [--warmup 5] [--split-reps 5]
                          [--cap-shape 128:40:8000] [--out profiles/lba_bench.json]
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
import lba_cases as lc  # noqa: E402


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def timed(fn, reps, warmup):
    t = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t))


SPLIT = ("upload", "setup", "errors", "linearize", "reduce_points", "reduce_kfs", "dinv", "schur", "solve", "update", "read_back",
         "flag_output", "download")         # ORBM_LBA_SPLIT_* of include/orbm.h


def run(pkg, m, n_local, n_fixed, n_points, reps, warmup, split_reps, medians=True):
    L = pkg.lib()
    pr = lc.scene(np.random.default_rng(n_points), n_free=n_local, n_fixed=n_fixed, n_points=n_points, kinds="mixed", outliers=0.1,
                  min_degree=3)
    s, a = pkg.pack_lba_problem(pr)
    E = len(a["edge_kf"])
    xw0 = a["xw"].copy()
    out = {side: dict(T=np.zeros((n_local, 16), np.float32), x=xw0.copy(), e=np.zeros(E, np.uint8), st=pkg.LbaStats()) for side in ("host", "gpu")}

    def call(side):
        o = out[side]
        np.copyto(o["x"], xw0)
        if side == "host":
            rc = L.orbp_local_bundle_adjustment(C.byref(s), p(o["T"]), p(o["x"]), p(o["e"]), None, C.byref(o["st"]))
        else:
            rc = L.orbm_local_bundle_adjustment(m.h, C.byref(s), p(o["T"]), p(o["x"]), p(o["e"]), None, C.byref(o["st"]))
        if rc != 0:
            raise SystemExit("%s: status %d: %s" % (side, rc, (L.orbp_last_error() if side == "host" else L.orbm_last_error()).decode()))

    def split_call():
        o = out["gpu"]
        np.copyto(o["x"], xw0)
        ms, cnt = np.zeros(len(SPLIT), np.float64), np.zeros(len(SPLIT), np.int32)
        t0 = time.perf_counter()
        rc = L.orbm_local_bundle_adjustment_split(m.h, C.byref(s), p(o["T"]), p(o["x"]), p(o["e"]), None, C.byref(o["st"]), p(ms), p(cnt))
        t1 = time.perf_counter()
        if rc != 0:
            raise SystemExit("split: status %d: %s" % (rc, L.orbm_last_error().decode()))
        return (t1 - t0) * 1e3, ms, cnt

    if medians:
        call("host")
    call("gpu")
    if not medians:
        out["host"] = out["gpu"]
    sh, sg = out["host"]["st"].as_dict(), out["gpu"]["st"].as_dict()
    res = dict(local_kfs=n_local, fixed_kfs=n_fixed, points=n_points, edges=E, reps=reps, warmup=warmup,
               iterations=list(sg["iterations"]), trials=list(sg["trials"]), level1=sg["n_level1"], erased=int(out["gpu"]["e"].sum()),
               same_flags=bool(np.array_equal(out["host"]["e"], out["gpu"]["e"])),
               same_counts=all(sh[k] == sg[k] for k in ("iterations", "trials", "n_level1")),
               max_pose_difference=float(np.abs(out["host"]["T"] - out["gpu"]["T"]).max()),
               max_point_difference=float(np.abs(out["host"]["x"] - out["gpu"]["x"]).max()),
               chi2_host=sh["chi2"], chi2_gpu=sg["chi2"])
    if medians:
        res["host_ms"] = timed(lambda: call("host"), reps, warmup)
        res["gpu_ms"] = timed(lambda: call("gpu"), reps, warmup)
        res["host_over_gpu"] = res["host_ms"] / res["gpu_ms"]
        res["gpu_ms_per_trial"] = res["gpu_ms"] / max(1, sum(sg["trials"]))
    else:
        for k in ("same_flags", "same_counts", "max_pose_difference", "max_point_difference", "chi2_host"):
            del res[k]
    whole = out["gpu"]["T"].tobytes() + out["gpu"]["x"].tobytes() + out["gpu"]["e"].tobytes()
    runs = sorted((split_call() for _ in range(split_reps)), key=lambda r: r[0])
    res["split_same_bytes"] = whole == out["gpu"]["T"].tobytes() + out["gpu"]["x"].tobytes() + out["gpu"]["e"].tobytes()
    t, ms, cnt = runs[len(runs) // 2]
    res["split_call_ms"] = t
    res["split_ms"] = {k: float(v) for k, v in zip(SPLIT, ms)}
    res["split_launches"] = {k: int(v) for k, v in zip(SPLIT, cnt)}
    res["split_device_ms"] = float(ms.sum())
    res["split_host_gap_ms"] = t - float(ms.sum())
    res["split_syncs"] = int(cnt[SPLIT.index("read_back")]) + 1
    res["split_host_gap_us_per_sync"] = 1e3 * res["split_host_gap_ms"] / res["split_syncs"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5:5:500,15:20:2500,40:40:8000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--split-reps", type=int, default=5)
    ap.add_argument("--cap-shape", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_bench.json"))
    args = ap.parse_args()
    pkg = _pkg()
    m = pkg.ORBmatcher(0.8, True)
    rows = []
    for shape in args.shapes.split(","):
        k, f, n = (int(v) for v in shape.split(":"))
        rows.append(run(pkg, m, k, f, n, args.reps, args.warmup, args.split_reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.cap_shape:
        k, f, n = (int(v) for v in args.cap_shape.split(":"))
        rows.append(run(pkg, m, k, f, n, 0, 0, args.split_reps, medians=False))
        rows[-1]["what"] = "split alone, at the largest number of local key frames the GPU call accepts"
        print(json.dumps(rows[-1]), flush=True)
    m.close()
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/bench_lba.py", "what": "medians of the C calls from host arrays, host clock, ms; split_*: one GPU call by events", "rows": rows}, fh, indent=2)
        fh.write("\n")


if __name__ == "__main__":
    main()
