#!/usr/bin/env python3
"""Cost of the forward half of LocalMapping::SearchInNeighbors' GPU work on one GPU: the one batch call (include/orbm.h,
orbm_fuse_views) against the loop it replaces, nviews x (orbm_project_points_kf + orbm_grid_build_kf + orbm_fuse), on the same
snapshot.

Workload: tests/fuse_views_oracle.make_scene at working size -- nviews target key frames of --features features, --points MapPoints
in the list.  Per nviews, median host-clock ms over --reps calls after --warmup calls, the C calls alone (arguments marshalled
once); every timed region ends in the device synchronisation the calls make themselves.
  batch_ms   one orbm_fuse_views
  loop_ms    nviews x (one orbm_project_points_kf (host) + one orbm_grid_build_kf + one orbm_fuse)
The loop's figure leaves out what its caller also does per point on the host between the projection and the search (the two
distance getters, MapPoint::PredictScale, ur = u - bf*invz): levels and flags are computed once, outside the timed region.  So it
is a lower bound of the loop.  The best_idx of the two sides are compared before anything is timed.  The numbers are what one run
measured; there is no speed gate.  Without a GPU the tool fails and writes nothing.

usage: tools/bench_fuse_views.py [--views 1,5,20,90] [--features 2000] [--points 1500] [--reps 30] [--warmup 5]
                                 [--out profiles/fuse_views_bench.json]
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
import fuse_views_oracle as FV  # noqa: E402


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


def run(pkg, nviews, nfeat, npoints, reps, warmup):
    sc = FV.make_scene(seed=4000 + nviews, nviews=nviews, n_mp=npoints, nfeat=[nfeat] * nviews)
    L = pkg.lib()
    m = pkg.ORBmatcher(0.6, True)
    ok = pkg.ORBX_OK
    views, off, kps, ur, dk, skip, xw, normal, mf_max, mf_min, mp_desc = [np.ascontiguousarray(a) for a in sc.inputs()]
    nv, n = sc.nviews, sc.n_mp
    outs = [np.zeros((nv, n), t) for t in (np.uint8, np.int32, np.int32, np.float32, np.float32, np.float32, np.int32)] + [np.zeros(nv, np.int32)]
    batch_args = [m.h, p(views), nv, p(off), p(kps), p(ur), p(dk), n, p(skip), p(xw), p(normal), p(mf_max), p(mf_min), p(mp_desc), C.c_float(sc.th)] + \
                 [p(o) for o in outs]

    def batch():
        assert L.orbm_fuse_views(*batch_args) == ok, L.orbm_last_error()

    batch()
    status, best_idx = outs[0].copy(), outs[1].copy()

    # the loop, marshalled once per view; use / level / ur are the caller's host work between the two C calls: computed once
    per = []
    for k in range(nv):
        V, feat = sc.views[k], sc.feats[k]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = V["Rcw"].reshape(3, 3)
        T[:3, 3] = V["tcw"]
        T = np.ascontiguousarray(T.reshape(16))
        Ow, b = np.ascontiguousarray(V["Ow"]), np.ascontiguousarray(V["bounds"])
        u, v, iz, d3 = (np.zeros(n, np.float32) for _ in range(4))
        inside = np.zeros(n, np.uint8)
        proj = [p(T), p(Ow), C.c_float(V["fx"]), C.c_float(V["fy"]), C.c_float(V["cx"]), C.c_float(V["cy"]), p(b), p(xw), p(normal), n, p(u), p(v), p(iz),
                p(d3), p(inside)]
        reached = np.isin(status[k], (FV.MATCH, FV.NO_MATCH)).astype(np.uint8)
        lvl = np.ascontiguousarray(outs[6][k].copy())
        pur = np.ascontiguousarray(outs[5][k].copy())
        nl = int(V["nlevels"])
        sf, inv = np.ascontiguousarray(V["scale_factors"][:nl]), np.ascontiguousarray(V["inv_level_sigma2"][:nl])
        g = FV.grid_tuple(V)
        bi, nf = np.full(n, -1, np.int32), C.c_int(0)
        grid = [m.h, p(feat.kps), len(feat)] + [C.c_float(x) for x in g]
        fuse = [m.h, n, p(reached), p(u), p(v), p(pur), p(lvl), p(mp_desc), p(sf), p(inv), nl, p(feat.kps), p(feat.u_right), p(feat.desc), len(feat),
                C.c_float(sc.th), p(bi), C.byref(nf)]
        per.append(dict(keep=(T, Ow, b, u, v, iz, d3, inside, reached, lvl, pur, sf, inv), proj=proj, grid=grid, fuse=fuse, bi=bi))

    def loop():
        for w in per:
            assert L.orbm_project_points_kf(*w["proj"]) == ok, L.orbm_last_error()
            assert L.orbm_grid_build_kf(*w["grid"]) == ok, L.orbm_last_error()
            assert L.orbm_fuse(*w["fuse"]) == ok, L.orbm_last_error()

    loop()                                   # faster and different is not faster
    for k, w in enumerate(per):
        assert np.array_equal(w["bi"], best_idx[k]), "view %d: best_idx differs" % k
    row = dict(nviews=nv, features=nfeat, points=n, searched=int(np.isin(status, (FV.MATCH, FV.NO_MATCH)).sum()), fused=int((status == FV.MATCH).sum()))
    # each side twice, alternating: the second pass shows the spread of the same measurement
    row["batch_ms"], row["batch_min_ms"] = timed(batch, reps, warmup)
    row["loop_ms"], row["loop_min_ms"] = timed(loop, reps, warmup)
    row["batch_ms_again"], _ = timed(batch, reps, warmup)
    row["loop_ms_again"], _ = timed(loop, reps, warmup)
    row["loop_over_batch"] = row["loop_ms"] / row["batch_ms"]
    m.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="1,5,20,90")
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--points", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_views_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fuse_views: no GPU; nothing measured, nothing written")
    pkg = _pkg()
    rows = [run(pkg, int(v), a.features, a.points, a.reps, a.warmup) for v in a.views.split(",")]
    for r in rows:
        print(json.dumps(r))
    out = dict(tool="tools/bench_fuse_views.py", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               method="median host-clock ms of the C calls over reps calls after warmup calls; *_again = the same measurement repeated after the other side's; "
                      "the loop leaves out the caller's per-point getters and PredictScale", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
