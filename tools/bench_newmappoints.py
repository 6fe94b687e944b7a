#!/usr/bin/env python3
"""Cost of LocalMapping::CreateNewMapPoints' GPU work per key frame on one GPU: the one batch call (include/orbm.h,
orbm_create_new_map_points) against the loop it replaces, nviews x (orbm_search_for_triangulation + orbm_triangulate_matches),
on the same inputs.

Workload: the scenes of tests/newmappoints_batch_oracle.py at working size -- key frames of 2000 features (KITTI calibration, mixed
stereo / mono, baselines from 0.05 m to 3 m over the views, 20 features per vocabulary node, 30 % of the features with a MapPoint
already, 10 % outlier descriptors), nviews second views.  Both sides run on the snapshot taken before the loop; the loop's
triangulation calls get the pair lists its searches return (built once, outside the timed region: composing the list is host
work of the caller on both sides).  Per nviews, median host-clock ms over --reps calls after --warmup calls, the C calls alone
(arguments marshalled once); every timed region ends in the device synchronisation the calls make themselves.
  batch_ms   one orbm_create_new_map_points
  loop_ms    nviews x (one orbm_search_for_triangulation + one orbm_triangulate_matches)
The outputs of the two sides are compared before anything is timed.  The numbers are what one run measured; there is no speed
gate.  Without a GPU the tool fails and writes nothing.

usage: tools/bench_newmappoints.py [--views 1,5,10,20] [--features 2000] [--reps 30] [--warmup 5]
                                   [--out profiles/newmappoints_batch_bench.json]
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
import newmappoints_batch_oracle as B  # noqa: E402
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


def c_arrays(*arrays):
    return [np.ascontiguousarray(a) for a in arrays]


def run(pkg, nviews, nfeat, reps, warmup):
    sc = B.make_scene(seed=3000 + nviews, nviews=nviews, npts=nfeat, seen=1.0, node_size=20, has_mp=0.3, baselines=(0.05, 3.0))
    L = pkg.lib()
    m = pkg.ORBmatcher(0.6, False)
    ok = pkg.ORBX_OK
    n1 = len(sc.kf1)

    # the batch call, marshalled once
    (cam1, k1, x1, u1, z1, d1, h1, fv1, cams2, F12, off2, k2, x2, u2, z2, d2, h2, fvo, fv2, only_stereo) = sc.batch_args()
    cam1a = np.ascontiguousarray(cam1, T.CAM_DTYPE).reshape(1)
    f1 = c_arrays(*[np.asarray(a, np.int32) for a in fv1])
    f2 = c_arrays(*[np.asarray(a, np.int32) for a in fv2])
    F12 = np.ascontiguousarray(F12, np.float32)
    bm = np.full((nviews, n1), -1, np.int32)
    bs, bx, bn = np.full((nviews, n1), 255, np.uint8), np.zeros((nviews, n1, 3), np.float32), np.zeros(nviews, np.int32)
    batch_args = [m.h, p(cam1a), p(k1), p(x1), p(u1), p(z1), p(d1), n1, p(h1), p(f1[0]), p(f1[1]), p(f1[2]), len(f1[0]), p(cams2), p(F12), nviews,
                  p(off2), p(k2), p(x2), p(u2), p(z2), p(d2), p(h2), p(fvo), p(f2[0]), p(f2[1]), p(f2[2]), 0, p(bm), p(bs), p(bx), p(bn)]

    def batch():
        assert L.orbm_create_new_map_points(*batch_args) == ok, L.orbm_last_error()

    # the loop, marshalled once per view
    views = []
    for v in range(nviews):
        kf2 = sc.kfs2[v]
        Cw, T2w, K2, F, sf2, sg2 = sc.search_args(v)
        keep = c_arrays(np.asarray(Cw, np.float32), np.asarray(T2w, np.float32).reshape(16), np.asarray(F, np.float32).reshape(9),
                        np.asarray(sf2, np.float32), np.asarray(sg2, np.float32), *[np.asarray(a, np.int32) for a in sc.fvs2[v]],
                        np.ascontiguousarray(sc.cams2[v], T.CAM_DTYPE).reshape(1), np.array([0, len(kf2)], np.int32))
        m12, nm = np.full(n1, -1, np.int32), C.c_int(0)
        search = [m.h, p(k1), p(d1), n1, p(h1), p(u1), p(f1[0]), p(f1[1]), p(f1[2]), len(f1[0]), p(kf2.kps_un), p(sc.descs2[v]), len(kf2),
                  p(sc.has2[v]), p(kf2.u_right), p(keep[5]), p(keep[6]), p(keep[7]), len(keep[5]), p(keep[0]), p(keep[1]), *K2, p(keep[2]),
                  p(keep[3]), p(keep[4]), len(keep[3]), 0, 0, p(m12), C.byref(nm)]
        views.append(dict(keep=keep, kf2=kf2, m12=m12, nm=nm, search=search))

    def loop_search(v):
        assert L.orbm_search_for_triangulation(*views[v]["search"]) == ok, L.orbm_last_error()

    for v in range(nviews):                      # the pair lists the searches return, once
        loop_search(v)
        w = views[v]
        i1 = np.nonzero(w["m12"] >= 0)[0]
        w["pairs"] = np.stack([i1, w["m12"][i1], np.zeros(len(i1), np.int64)], 1).astype(np.int32)
        w["st"], w["x"] = np.full(len(i1), 255, np.uint8), np.zeros((len(i1), 3), np.float32)
        kf2 = w["kf2"]
        w["tri"] = [m.h, p(cam1a), p(k1), p(x1), p(u1), p(z1), n1, p(w["keep"][8]), 1, p(w["keep"][9]), p(kf2.kps_un), p(kf2.keys_xy), p(kf2.u_right),
                    p(kf2.depth), p(w["pairs"]), len(i1), p(w["st"]), p(w["x"])]

    def loop():
        for v in range(nviews):
            loop_search(v)
            assert L.orbm_triangulate_matches(*views[v]["tri"]) == ok, L.orbm_last_error()

    # faster and different is not faster: the two sides agree before anything is timed
    batch()
    loop()
    pairs = 0
    for v in range(nviews):
        w = views[v]
        i1 = w["pairs"][:, 0]
        assert np.array_equal(bm[v], w["m12"]) and bn[v] == w["nm"].value, "view %d: matches differ" % v
        assert np.array_equal(bs[v, i1], w["st"]) and np.array_equal(bx[v, i1].view(np.uint32), w["x"].view(np.uint32)), "view %d: points differ" % v
        pairs += len(i1)
    row = dict(nviews=nviews, features=n1, pairs=int(pairs), accepted=int((bs <= T.STEREO2).sum()))
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
    ap.add_argument("--views", default="1,5,10,20")
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newmappoints_batch_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_newmappoints: no GPU; nothing measured, nothing written")
    pkg = _pkg()
    rows = [run(pkg, int(v), a.features, a.reps, a.warmup) for v in a.views.split(",")]
    for r in rows:
        print(json.dumps(r))
    out = dict(tool="tools/bench_newmappoints.py", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               method="median host-clock ms of the C calls over reps calls after warmup calls; *_again = the same measurement repeated after the other side's", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
