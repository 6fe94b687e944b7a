#!/usr/bin/env python3
"""Cost of Optimizer::PoseOptimization for a batch of problems in one launch (orbm_pose_optimization_batch, include/orbm.h)
against the host path called once per problem (orbp_pose_optimization, include/orbp.h), on one GPU.

Workload: tests/pose_cases.py bench_problems(B, n): B problems of n observations (KITTI calibration, noise 0.7 px, a fifth of the
observations gross outliers in every third problem, stereo edges in every third), the same arrays on every path.  Per (B, n),
medians over --reps calls after --warmup calls on a warm handle:
  host_loop_ms      B calls of orbp_pose_optimization, the C calls alone, host clock
  batch_host_ms     orbm_pose_optimization_batch from host arrays, the C call alone (one staged upload, one launch, one download,
                    one synchronisation), host clock
  batch_device_ms   orbm_pose_optimization_batch_device on resident inputs, timed by events on its stream: the kernel and its launch
                    (the in/out poses are copied afresh on the same stream before the first event)
The batch results are checked against the host loop's (pose to 2e-6, flags, counts) before anything is timed.
The numbers are what one run measured.

usage: tools/bench_pose.py [--batches 1,8,64] [--sizes 300,1500] [--reps 30] [--warmup 5] [--out profiles/pose_batch.json]
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
import pose_cases as pc  # noqa: E402


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


def run(pkg, m, B, n, reps, warmup):
    import torch
    L = pkg.lib()
    problems = pc.bench_problems(B, n)
    off, obs, ur, s2, xw, cams, T0 = pkg.ORBmatcher.pack_pose_problems(problems)
    N = int(off[-1])

    def chk(rc, err=L.orbm_last_error):
        if rc < 0:
            raise SystemExit("status %d: %s" % (rc, err().decode()))
        return rc

    Th, oh, gh = T0.copy(), np.zeros(N, np.uint8), np.zeros(B, np.int32)

    def host_loop():
        np.copyto(Th, T0)
        for k in range(B):
            a, b = int(off[k]), int(off[k + 1])
            c = cams[k]
            gh[k] = chk(L.orbp_pose_optimization(b - a, p(obs[a:b]), None if ur is None else p(ur[a:b]), p(s2[a:b]), p(xw[a:b]), float(c["fx"]),
                                                 float(c["fy"]), float(c["cx"]), float(c["cy"]), float(c["bf"]), p(Th[k]), p(oh[a:b])), L.orbp_last_error)

    Tb, ob, gb = T0.copy(), np.zeros(N, np.uint8), np.zeros(B, np.int32)

    def batch_host():
        np.copyto(Tb, T0)
        chk(L.orbm_pose_optimization_batch(m.h, B, p(off), p(obs), p(ur), p(s2), p(xw), p(cams), p(Tb), p(ob), p(gb)))

    host_loop()
    batch_host()
    if not (np.abs(Tb - Th).max() <= 2e-6 and np.array_equal(ob, oh) and np.array_equal(gb, gh)):
        raise SystemExit("the batch differs from the host loop at B = %d, n = %d" % (B, n))
    res = dict(problems=B, observations_each=n, reps=reps, warmup=warmup, inliers=int(gh.sum()))
    res["host_loop_ms"] = timed(host_loop, reps, warmup)
    res["batch_host_ms"] = timed(batch_host, reps, warmup)

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_in = [dev(off), dev(obs), dev(ur), dev(s2), dev(xw), dev(cams.view(np.float32).reshape(B, 5))]
    d_T0, d_T = dev(T0), dev(T0)
    d_o, d_g = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = []
    for i in range(warmup + reps):
        with torch.cuda.stream(s):
            d_T.copy_(d_T0)
            e0.record(s)
            m.pose_optimization_batch_device(B, *d_in, d_T, d_o, d_g, stream=s)
            e1.record(s)
        s.synchronize()
        if i >= warmup:
            t.append(e0.elapsed_time(e1))
    res["batch_device_ms"] = float(np.median(t))
    if not (d_T.cpu().numpy().tobytes() == Tb.tobytes() and np.array_equal(d_o.cpu().numpy(), ob) and np.array_equal(d_g.cpu().numpy(), gb)):
        raise SystemExit("the device entry point differs from the host entry point at B = %d, n = %d" % (B, n))
    res["host_loop_over_batch_host"] = res["host_loop_ms"] / res["batch_host_ms"]
    res["host_loop_over_batch_device"] = res["host_loop_ms"] / res["batch_device_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--sizes", default="300,1500")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = _pkg()
    m = pkg.ORBmatcher(0.8, max_queries=65536, max_train=1024, max_pairs=1024)
    results = []
    for n in (int(v) for v in a.sizes.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            print("B = %d, n = %d" % (B, n), file=sys.stderr, flush=True)
            results.append(run(pkg, m, B, n, a.reps, a.warmup))
    m.close()
    out = dict(tool="tools/bench_pose.py",
               workload="tests/pose_cases.py bench_problems: KITTI calibration, noise 0.7 px, n/5 gross outliers in every third problem, stereo edges in every third",
               results=results,
               note="single run; medians of --reps after --warmup on a warm handle; host_loop and batch_host by the host clock around the C calls "
                    "(batch_host ends in a synchronisation), batch_device by events on the call's stream")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
