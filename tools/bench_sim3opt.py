#!/usr/bin/env python3
"""Cost of Optimizer::OptimizeSim3 for a batch of problems in one launch (orbm_optimize_sim3_batch, include/orbm.h) against the host
path called once per problem (orbp_optimize_sim3, include/orbp.h), on one GPU.

Workload: tests/optimize_sim3_cases.py bench_problems(B, n): B problems of n pairs (KITTI calibration, noise 0.7 px, a fifth of
the pairs gross outliers in every other problem, free scale in every third), the same arrays on every path.  Per (B, n), medians
over --reps calls after --warmup calls on a warm handle:
  host_loop_ms      B calls of orbp_optimize_sim3, the C calls alone, host clock
  batch_host_ms     orbm_optimize_sim3_batch from host arrays, the C call alone (one staged upload, one launch, one download, one
                    synchronisation), host clock
  batch_device_ms   orbm_optimize_sim3_batch_device on resident inputs, timed by events on its stream: the kernel and its launch
                    (the in/out S12 are copied afresh on the same stream before the first event)
The batch results are checked against the host loop's (flags, counts, S12 within the bar of tests/golden/sim3opt/tolerance.json)
before anything is timed.  The numbers are what one run measured.

usage: tools/bench_sim3opt.py [--batches 1,3,8,20] [--sizes 50,150,400] [--reps 30] [--warmup 5] [--out profiles/sim3opt_batch.json]
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
import optimize_sim3_cases as sc  # noqa: E402

BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "sim3opt", "tolerance.json")))["bar"]


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
    problems = sc.bench_problems(B, n)
    off, x1, x2, o1, o2, s1, s2, cams, th2, fix, S0 = pkg.ORBmatcher.pack_sim3opt_problems(problems)
    N = int(off[-1])

    def chk(rc, err=L.orbm_last_error):
        if rc < 0:
            raise SystemExit("status %d: %s" % (rc, err().decode()))
        return rc

    Sh, fh, gh = S0.copy(), np.zeros(N, np.uint8), np.zeros(B, np.int32)

    def host_loop():
        np.copyto(Sh, S0)
        for k in range(B):
            a, b = int(off[k]), int(off[k + 1])
            gh[k] = chk(L.orbp_optimize_sim3(b - a, p(x1[a:b]), p(x2[a:b]), p(o1[a:b]), p(o2[a:b]), p(s1[a:b]), p(s2[a:b]), p(cams[k, :4]),
                                             p(cams[k, 4:]), float(th2[k]), int(fix[k]), p(Sh[k]), p(fh[a:b])), L.orbp_last_error)

    Sb, fb, gb = S0.copy(), np.zeros(N, np.uint8), np.zeros(B, np.int32)

    def batch_host():
        np.copyto(Sb, S0)
        chk(L.orbm_optimize_sim3_batch(m.h, B, p(off), p(x1), p(x2), p(o1), p(o2), p(s1), p(s2), p(cams), p(th2), p(fix), p(Sb), p(fb), p(gb)))

    host_loop()
    batch_host()
    d = np.abs(Sb - Sh)
    if not (np.array_equal(fb, fh) and np.array_equal(gb, gh) and d[:, :4].max() <= BARS["quaternion"] and d[:, 4:7].max() <= BARS["translation"]
            and d[:, 7].max() <= BARS["scale"]):
        raise SystemExit("the batch differs from the host loop at B = %d, n = %d" % (B, n))
    res = dict(problems=B, pairs_each=n, reps=reps, warmup=warmup, inliers=int(gh.sum()))
    res["host_loop_ms"] = timed(host_loop, reps, warmup)
    res["batch_host_ms"] = timed(batch_host, reps, warmup)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_in = [dev(a) for a in (off, x1, x2, o1, o2, s1, s2, cams, th2, fix)]
    d_S0, d_S = dev(S0), dev(S0)
    d_f, d_g = torch.zeros(max(N, 1), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = []
    for i in range(warmup + reps):
        with torch.cuda.stream(s):
            d_S.copy_(d_S0)
            e0.record(s)
            m.optimize_sim3_batch_device(B, *d_in, d_S, d_f, d_g, stream=s)
            e1.record(s)
        s.synchronize()
        if i >= warmup:
            t.append(e0.elapsed_time(e1))
    res["batch_device_ms"] = float(np.median(t))
    if not (d_S.cpu().numpy().tobytes() == Sb.tobytes() and np.array_equal(d_f.cpu().numpy()[:N], fb) and np.array_equal(d_g.cpu().numpy(), gb)):
        raise SystemExit("the device entry point differs from the host entry point at B = %d, n = %d" % (B, n))
    res["host_loop_over_batch_host"] = res["host_loop_ms"] / res["batch_host_ms"]
    res["host_loop_over_batch_device"] = res["host_loop_ms"] / res["batch_device_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,3,8,20")
    ap.add_argument("--sizes", default="50,150,400")
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
    out = dict(tool="tools/bench_sim3opt.py",
               workload="tests/optimize_sim3_cases.py bench_problems: KITTI calibration, noise 0.7 px, n/5 gross outliers in every other problem, "
                        "free scale in every third, th2 = 10",
               results=results,
               note="single run; medians of --reps after --warmup on a warm handle; host_loop and batch_host by the host clock around the C calls "
                    "(batch_host ends in a synchronisation), batch_device by events on the call's stream")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
