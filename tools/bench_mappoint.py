#!/usr/bin/env python3
"""Cost of MapPoint::ComputeDistinctiveDescriptors for all MapPoints of a key frame (include/orbm.h,
orbm_distinctive_descriptors) on one GPU, against the two things an integrator could do instead.

Workload: the key-frame-shaped batch of tests/mappoint_oracle.py (run lengths mostly 2..15 with a tail to a few hundred; a
run = one random descriptor with up to 6 bit flips per observation) at M = 500, 2000 and 8000 MapPoints.  Per size, median
host-clock ms over --reps calls after --warmup calls, every timed region ending in a device synchronisation or running on the
host only:
  (a) batched_ms           orbm_distinctive_descriptors from host arrays, the C call alone (batched_python_ms: through the
                           numpy wrapper ORBmatcher.distinctive_descriptors)
  (b) device_call_ms       orbm_distinctive_descriptors_device on resident inputs + a stream synchronise: launches and kernels
                           without the staging copy, the two transfers and the result copy; transfers_ms = (a) - device_call_ms.
                           With --kernel-stats (the stats CSV of a `rocprofv3 --kernel-trace --stats` run of this tool with
                           --sizes M --only-batched, a run of its own) kernel_us is the k_dd_* kernel time per call at that M
  (c) per_point_distances_ms   what INTEGRATION.md recommended before: one dense orbm_distances call per MapPoint with N >= 3
                           (its N x N matrix comes back; the medians and the minimum are NOT counted: a lower bound)
  (d) host_port_ms         tools/mappoint_host_port.cc, a single-thread PORT of the reference's algorithm compiled with g++ -O2
                           (not the reference binary), on the same batch; its answers are checked against (a)
The numbers are what one run measured; there is no speed gate.

usage: tools/bench_mappoint.py [--sizes 500,2000,8000] [--reps 30] [--warmup 5] [--out profiles/mappoint_bench.json]
                               [--kernel-stats CSV] [--only-batched]
"""
import argparse
import csv
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mappoint_oracle as MO  # noqa: E402


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def host_port():
    so = os.path.join(tempfile.mkdtemp(prefix="mappoint_port_"), "mappoint_host_port.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "mappoint_host_port.cc"), "-o", so])
    L = C.CDLL(so)
    L.mappoint_host_port.argtypes = [C.c_int] + [C.c_void_p] * 4
    L.mappoint_host_port.restype = None
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def timed(fn, reps, warmup):
    t = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def kernel_stats(path):
    rows = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_dd_" in row["Name"]:
                rows[row["Name"].split("(")[0].split()[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    if "k_dd_small" not in rows:
        raise SystemExit("%s: no k_dd_small row" % path)
    return rows


def run(pkg, port, npts, reps, warmup, only_batched):
    import torch
    rng = np.random.default_rng(1000 + npts)
    lengths = MO.run_lengths_keyframe(rng, npts)
    off, desc = MO.batch_from_lengths(rng, lengths)
    m = pkg.ORBmatcher()
    L = pkg.lib()
    best, med = np.zeros(npts, np.int32), np.zeros(npts, np.int32)

    def batched():
        rc = L.orbm_distinctive_descriptors(m.h, npts, p(off), p(desc), p(best), p(med))
        if rc != 0:
            raise SystemExit("orbm status %d: %s" % (rc, L.orbm_last_error().decode()))
    a_med, a_min = timed(batched, reps, warmup)
    res = dict(points=npts, rows=int(off[-1]), max_run=int(lengths.max()), pairs=int((lengths * (lengths - 1) // 2).sum()),
               batched_ms=a_med, batched_ms_min=a_min, reps=reps, warmup=warmup)
    if only_batched:
        return res
    res["batched_python_ms"] = timed(lambda: m.distinctive_descriptors(off, desc), reps, warmup)[0]

    d_off, d_desc = torch.from_numpy(off).cuda(), torch.from_numpy(desc).cuda()
    d_best = torch.zeros(npts, dtype=torch.int32, device="cuda"); d_med = torch.zeros(npts, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def device():
        m.distinctive_descriptors_device(npts, d_off.data_ptr(), d_desc.data_ptr(), int(off[-1]), int(lengths.max()),
                                         d_best.data_ptr(), d_med.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
    res["device_call_ms"] = timed(device, reps, warmup)[0]
    res["transfers_ms"] = a_med - res["device_call_ms"]
    if not (np.array_equal(d_best.cpu().numpy(), best) and np.array_equal(d_med.cpu().numpy(), med)):
        raise SystemExit("device entry point differs from the host entry point")

    big = np.nonzero(lengths >= 3)[0]
    dist = np.zeros(int(lengths.max()) ** 2, np.int32)
    rows = [np.ascontiguousarray(desc[off[i]:off[i + 1]]) for i in big]

    def per_point():
        for r in rows:
            rc = L.orbm_distances(m.h, p(r), len(r), p(r), len(r), None, None, p(dist))
            if rc != 0:
                raise SystemExit("orbm status %d: %s" % (rc, L.orbm_last_error().decode()))
    res["per_point_distances_ms"] = timed(per_point, max(3, reps // 6), 1)[0]
    res["per_point_calls"] = int(len(big))

    pb, pm = np.zeros(npts, np.int32), np.zeros(npts, np.int32)
    res["host_port_ms"] = timed(lambda: port.mappoint_host_port(npts, p(off), p(desc), p(pb), p(pm)), reps, warmup)[0]
    if not (np.array_equal(pb, best) and np.array_equal(pm, med)):
        raise SystemExit("host port differs from the library")
    res["batched_over_host_port"] = res["host_port_ms"] / a_med
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,2000,8000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-stats-points", type=int, default=2000)
    ap.add_argument("--only-batched", action="store_true")
    a = ap.parse_args()
    pkg = _pkg()
    port = None if a.only_batched else host_port()
    results = [run(pkg, port, int(s), a.reps, a.warmup, a.only_batched) for s in a.sizes.split(",")]
    out = dict(tool="tools/bench_mappoint.py", workload="key-frame-shaped runs (mostly 2..15, tail to 400), <= 6 bit flips per row",
               results=results,
               note="single run; host clock around synchronised calls, medians; batched_ms = the C call from host arrays; "
                    "device_call_ms = launches + kernels on resident inputs; per_point_distances_ms = one orbm_distances call per MapPoint "
                    "with N >= 3, selection not counted; host_port_ms = single-thread g++ -O2 port of the reference's algorithm "
                    "(tools/mappoint_host_port.cc), not the reference binary")
    if a.kernel_stats:
        rows = kernel_stats(a.kernel_stats)
        calls = rows["k_dd_small"][0]
        out["kernel"] = dict(points=a.kernel_stats_points, calls=calls, kernel_us=sum(t for _, t in rows.values()) / calls / 1e3,
                             per_kernel_us={k: t / calls / 1e3 for k, (_, t) in sorted(rows.items())},
                             source=os.path.basename(a.kernel_stats))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
