#!/usr/bin/env python3
"""Cost of the CreateNewMapPoints per-match loop (include/orbm.h, orbm_triangulate_matches) on one GPU.

Workload: the mixed stereo / mono key-frame pair of tests/triangulation_oracle.py (KITTI calibration, 0.5 m baseline, depths
2-40 m, 0.7 px noise, 10 % outliers), n matches over two key frames of max(n, 2000) features each.  Per n, median host-clock ms
over --reps calls after --warmup calls, every timed region ending in a device synchronisation:
  host_call_ms     orbm_triangulate_matches from host arrays, the C call alone: one staged upload, one launch, one download
  device_call_ms   orbm_triangulate_matches_device on resident inputs + a stream synchronise: the launch and the kernel
  transfers_ms     the difference
With --kernel-stats (the stats CSV of a `rocprofv3 --kernel-trace --stats` run of this tool with --sizes N --only-host, a run
of its own) kernel_us is k_triangulate's own duration per call at that n.
Nothing on the host is timed against it: the loop it replaces costs one 4x4 cv::SVD per match, and no OpenCV is here to
measure.  The numbers are what one run measured; there is no speed gate.

usage: tools/bench_triangulate.py [--sizes 100,300,1000,5000,20000] [--reps 30] [--warmup 5] [--out profiles/triangulate_bench.json]
                                  [--kernel-stats CSV --kernel-stats-n N] [--only-host]
"""
import argparse
import csv
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triangulation_oracle as T  # noqa: E402


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


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


def run(pkg, n, reps, warmup, only_host):
    import torch
    rng = np.random.default_rng(2000 + n)
    nfeat = max(n, 2000)
    cam1, kf1, cam2, kf2, matches = T.make_pair(rng, nfeat)
    matches = np.ascontiguousarray(matches[:n])
    cam1, cams2, off2 = np.array([cam1]), np.array([cam2]), np.array([0, nfeat], np.int32)
    m = pkg.ORBmatcher()
    L = pkg.lib()
    st, x = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)

    def host():
        rc = L.orbm_triangulate_matches(m.h, p(cam1), p(kf1.kps_un), p(kf1.keys_xy), p(kf1.u_right), p(kf1.depth), nfeat, p(cams2), 1, p(off2),
                                        p(kf2.kps_un), p(kf2.keys_xy), p(kf2.u_right), p(kf2.depth), p(matches), n, p(st), p(x))
        if rc != 0:
            raise SystemExit("orbm status %d: %s" % (rc, L.orbm_last_error().decode()))
    h_med, h_min = timed(host, reps, warmup)
    est, ex = T.triangulate(cam1[0], kf1, cams2, off2, kf2, matches)
    if not (np.array_equal(st, est) and np.array_equal(x.view(np.uint32), ex.view(np.uint32))):
        raise SystemExit("the library differs from the restatement at n = %d" % n)
    res = dict(matches=n, features_per_key_frame=nfeat, accepted=int((est <= T.STEREO2).sum()), svd_solves=int(np.isin(est, [0, 4]).sum() + 0),
               host_call_ms=h_med, host_call_ms_min=h_min, reps=reps, warmup=warmup)
    if only_host:
        return res

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = [dev(cam1), dev(kf1.kps_un), dev(kf1.keys_xy), dev(kf1.u_right), dev(kf1.depth), dev(cams2), dev(off2), dev(kf2.kps_un),
         dev(kf2.keys_xy), dev(kf2.u_right), dev(kf2.depth), dev(matches)]
    d_st = torch.zeros(n, dtype=torch.uint8, device="cuda"); d_x = torch.zeros((n, 3), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def device():
        m.triangulate_matches_device(*[t.data_ptr() for t in d[:5]], nfeat, d[5].data_ptr(), 1, *[t.data_ptr() for t in d[6:]], n,
                                     d_st.data_ptr(), d_x.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
    res["device_call_ms"], res["device_call_ms_min"] = timed(device, reps, warmup)
    res["transfers_ms"] = h_med - res["device_call_ms"]
    if not (np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_x.cpu().numpy().view(np.uint32), x.view(np.uint32))):
        raise SystemExit("device entry point differs from the host entry point")
    m.close()
    return res


def kernel_stats(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_triangulate" in row["Name"]:
                return int(row["Calls"]), float(row["TotalDurationNs"])
    raise SystemExit("%s: no k_triangulate row" % path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,300,1000,5000,20000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-stats-n", type=int, default=1000)
    ap.add_argument("--only-host", action="store_true")
    a = ap.parse_args()
    pkg = _pkg()
    results = [run(pkg, int(s), a.reps, a.warmup, a.only_host) for s in a.sizes.split(",")]
    out = dict(tool="tools/bench_triangulate.py",
               workload="mixed stereo / mono pair, KITTI calibration, 0.5 m baseline, depths 2-40 m, 0.7 px noise, 10 % outliers",
               results=results,
               note="single run; host clock around synchronised calls, medians; host_call_ms = the C call from host arrays; "
                    "device_call_ms = launch + kernel on resident inputs; no host cv::SVD loop was measured")
    if a.kernel_stats:
        calls, total = kernel_stats(a.kernel_stats)
        out["kernel"] = dict(matches=a.kernel_stats_n, calls=calls, kernel_us=total / calls / 1e3, source=os.path.basename(a.kernel_stats))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
