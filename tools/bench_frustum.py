#!/usr/bin/env python3
"""Cost of Frame::isInFrustum over a local map and of Tracking::SearchLocalPoints in one call (include/orbm.h) on one GPU.

Workload: the stereo scene of tests/frustum_oracle.py (KITTI calibration, local points 1-80 m over one and a half fields of
view, 10 % skipped) with n local MapPoints, and its synthetic current frame (the visible points' key points plus 600 of clutter).
Per n, median host-clock ms over --reps calls after --warmup calls, every timed region ending in a device synchronisation:
  a_frustum_host_ms     orbm_frustum from host arrays, the C call alone: one staged upload, one launch, one download
  b_frustum_device_ms   orbm_frustum_device on resident inputs + a stream synchronise: the launch and the kernel
  c_fused_ms            orbm_search_local_points (the frame's grid is in the handle)
  d_two_calls_ms        what the library offered before for the same work: orbm_frustum, its outputs on the host, in_view =
                        (status == 0), orbm_search_by_projection_map; measured three times (d_runs_ms), d_spread_ms = max - min
Both (c) and (d) copy the frame's cur_obs afresh inside the timed region and must return the same matches.
Nothing on the host is timed against (a): no plain C++ isInFrustum loop is here, so that comparison is unmeasured.
The numbers are what one run measured.

usage: tools/bench_frustum.py [--sizes 500,1000,2000,5000,20000] [--reps 30] [--warmup 5] [--out profiles/frustum_bench.json]
                              [--only fused|two]    (one path only, for a rocprofv3 kernel trace of its own)
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
import frustum_oracle as F  # noqa: E402


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
    return float(np.median(t))


def run(pkg, n, reps, warmup, only):
    import torch
    sc = F.make_scene(np.random.default_rng(3000 + n), n)
    fr = F.make_frame(np.random.default_rng(4000 + n), sc)
    view = np.array([sc.view])
    nc = len(fr.kps)
    sf = np.ascontiguousarray(sc.view["scale_factors"][:8])
    m = pkg.ORBmatcher(0.8, max_queries=max(8192, 3 * n), max_train=8192)
    L = pkg.lib()
    m.grid_build(fr.kps, *[float(b) for b in sc.view["bounds"]])
    st = np.zeros(n, np.uint8)
    px, py, pxr, vc = (np.zeros(n, np.float32) for _ in range(4))
    lv = np.zeros(n, np.int32)
    nt, nm = C.c_int(0), C.c_int(0)
    cm = np.zeros(nc, np.int32)
    cur = fr.cur_obs.copy()
    lim, th, ratio = C.c_float(0.5), C.c_float(3.0), C.c_float(0.8)

    def chk(rc):
        if rc != 0:
            raise SystemExit("orbm status %d: %s" % (rc, L.orbm_last_error().decode()))

    def frustum():
        chk(L.orbm_frustum(m.h, p(view), n, p(sc.skip), p(sc.xw), p(sc.normal), p(sc.mf_max), p(sc.mf_min), lim, p(st), p(px), p(py), p(pxr),
                           p(lv), p(vc), C.byref(nt)))

    def fused():
        np.copyto(cur, fr.cur_obs)
        chk(L.orbm_search_local_points(m.h, p(view), n, p(sc.skip), p(sc.xw), p(sc.normal), p(sc.mf_max), p(sc.mf_min), lim, p(fr.mp_desc),
                                       p(fr.mp_obs), p(fr.kps), p(fr.desc), p(fr.u_right), nc, th, ratio, p(st), p(px), p(py), p(pxr), p(lv),
                                       p(vc), C.byref(nt), p(cur), p(cm), C.byref(nm)))

    def two_calls():
        np.copyto(cur, fr.cur_obs)
        frustum()
        if nt.value > 0:
            in_view = (st == 0).astype(np.uint8)
            chk(L.orbm_search_by_projection_map(m.h, n, p(in_view), p(px), p(py), p(pxr), p(lv), p(vc), p(fr.mp_desc), p(fr.mp_obs), p(sf), 8,
                                                p(fr.kps), p(fr.desc), p(fr.u_right), nc, th, ratio, p(cur), p(cm), C.byref(nm)))

    res = dict(map_points=n, key_points=nc, reps=reps, warmup=warmup)
    if only:
        res[only] = timed(fused if only == "fused" else two_calls, reps, warmup)
        return res
    res["a_frustum_host_ms"] = timed(frustum, reps, warmup)
    want = F.frustum(*sc.args(), 0.5)
    if not (np.array_equal(st, want[0]) and np.array_equal(px.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(lv, want[4])):
        raise SystemExit("the library differs from the restatement at n = %d" % n)
    res["in_view"] = int(nt.value)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = [dev(view), dev(sc.skip), dev(sc.xw), dev(sc.normal), dev(sc.mf_max), dev(sc.mf_min)]
    o = [torch.zeros(n, dtype=torch.uint8, device="cuda")] + [torch.zeros(n, device="cuda") for _ in range(3)] + \
        [torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda")]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def device():
        m.frustum_device(d[0].data_ptr(), n, *[t.data_ptr() for t in d[1:]], 0.5, *[t.data_ptr() for t in o], stream=s.cuda_stream)
        s.synchronize()
    res["b_frustum_device_ms"] = timed(device, reps, warmup)
    if not np.array_equal(o[0].cpu().numpy(), st):
        raise SystemExit("device entry point differs from the host entry point")
    d_runs = [timed(two_calls, reps, warmup)]
    cm_two, nm_two = cm.copy(), nm.value
    res["c_fused_ms"] = timed(fused, reps, warmup)
    if nm.value != nm_two or not np.array_equal(cm, cm_two):
        raise SystemExit("the fused call differs from the two calls at n = %d" % n)
    d_runs += [timed(two_calls, reps, warmup), timed(two_calls, reps, warmup)]
    res["matches"] = int(nm.value)
    res["d_runs_ms"] = d_runs
    res["d_two_calls_ms"] = float(np.median(d_runs))
    res["d_spread_ms"] = float(max(d_runs) - min(d_runs))
    res["c_within_d_plus_spread"] = bool(res["c_fused_ms"] <= res["d_two_calls_ms"] + res["d_spread_ms"])
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,1000,2000,5000,20000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["fused", "two"], default=None)
    a = ap.parse_args()
    pkg = _pkg()
    results = [run(pkg, int(s), a.reps, a.warmup, a.only) for s in a.sizes.split(",")]
    out = dict(tool="tools/bench_frustum.py",
               workload="stereo scene, KITTI calibration, local points 1-80 m, 10 % skipped; frame = visible points' key points + 600 clutter; th 3",
               results=results,
               note="single run; host clock around synchronised calls, medians of --reps after --warmup; d measured three times; "
                    "no host isInFrustum loop was measured")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
