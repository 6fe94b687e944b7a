#!/usr/bin/env python3
"""Cost of SearchByBoW over the candidate key frames of a relocalisation (Tracking::Relocalization) or of a loop detection
(LoopClosing::ComputeSim3) on one GPU: the one batch call (include/orbm.h, orbm_search_by_bow_batch / orbm_search_by_bow_kf_batch)
against the loop it replaces, K calls of orbm_search_by_bow / orbm_search_by_bow_kf on the same handle and the same inputs.

Workload: the generator of tests/bow_batch_cases.py at working size -- a shared side of N features spread at random over 1000
vocabulary node ids (636 of them occupied at N = 1000, 865 at N = 2000: the order of what levelsup = 4 gives on a real vocabulary),
K candidates of N features each, 70 % of them copies of shared features with 0 to 30 flipped bits in the node of their source.
Host arrays in and out, the C calls alone (arguments marshalled once): the
adapters' gather from the object graph is on neither side.  Every timed region ends in the device synchronisation the calls make
themselves.  The two sides alternate inside one process, repetition by repetition, after --warmup repetitions of both; per shape
the median, the 10th / 90th percentile and the minimum of --reps host-clock times:
  batch_ms   one batch call over K candidates
  loop_ms    K one-candidate calls
The outputs of the two sides are compared before anything is timed.  The numbers are what one run measured; there is no speed
gate.  Without a GPU the tool fails and writes nothing.

usage: tools/bench_bow_batch.py [--k 1,5,20] [--features 1000,2000] [--reps 200] [--warmup 20] [--out profiles/bow_batch.json]
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
import bow_batch_cases as B  # noqa: E402


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def stats(t):
    t = np.asarray(t) * 1e3
    return dict(median=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), min=float(t.min()))


def working_case(variant, nfeat, kmax):
    rng = np.random.default_rng(nfeat + (0 if variant == "frame" else 1))
    sizes = [int(s) for s in rng.multinomial(nfeat, np.full(1000, 1e-3)) if s > 0]
    return B.make_case("bench-%s-%d" % (variant, nfeat), variant, 9000 + nfeat + (0 if variant == "frame" else 1), nfeat, sizes,
                       [{"n": nfeat} for _ in range(kmax)], nnratio=0.75, check_ori=True)


def run(pkg, case, reps, warmup):
    L = pkg.lib()
    ok = pkg.ORBX_OK
    m = pkg.ORBmatcher(case.nnratio, case.check_ori)
    K, n = len(case.cands), len(case.shared)
    nn, ori = C.c_float(case.nnratio), 1 if case.check_ori else 0
    sh, keep_s = pkg.bow_sides([case.shared.tup()])
    cs, keep_c = pkg.bow_sides([c.tup() for c in case.cands])
    bt, bn = np.full((K, n), -1, np.int32), np.zeros(K, np.int32)
    lt, ln = np.full((K, n), -1, np.int32), [C.c_int(0) for _ in range(K)]
    s = case.shared
    sfv = [np.ascontiguousarray(a, np.int32) for a in s.fv]
    loops = []
    for c, cand in enumerate(case.cands):
        cfv = [np.ascontiguousarray(a, np.int32) for a in cand.fv]
        keep_c.append(cfv)
        if case.variant == "frame":
            loops.append([m.h, p(cand.desc), p(cand.kps), len(cand), p(cand.valid), p(cfv[0]), p(cfv[1]), p(cfv[2]), len(cfv[0]),
                          p(s.desc), p(s.kps), n, p(sfv[0]), p(sfv[1]), p(sfv[2]), len(sfv[0]), nn, ori, p(lt[c]), C.byref(ln[c])])
        else:
            loops.append([m.h, p(s.desc), p(s.kps), n, p(s.valid), p(sfv[0]), p(sfv[1]), p(sfv[2]), len(sfv[0]),
                          p(cand.desc), p(cand.kps), len(cand), p(cand.valid), p(cfv[0]), p(cfv[1]), p(cfv[2]), len(cfv[0]), nn, ori, p(lt[c]),
                          C.byref(ln[c])])
    shp, csp = C.cast(sh, C.c_void_p), C.cast(cs, C.c_void_p)

    if case.variant == "frame":
        def batch():
            assert L.orbm_search_by_bow_batch(m.h, csp, K, shp, nn, ori, p(bt), p(bn)) == ok, L.orbm_last_error()

        def loop():
            for a in loops:
                assert L.orbm_search_by_bow(*a) == ok, L.orbm_last_error()
    else:
        def batch():
            assert L.orbm_search_by_bow_kf_batch(m.h, shp, csp, K, nn, ori, p(bt), p(bn)) == ok, L.orbm_last_error()

        def loop():
            for a in loops:
                assert L.orbm_search_by_bow_kf(*a) == ok, L.orbm_last_error()

    # faster and different is not faster: the two sides agree before anything is timed
    batch()
    loop()
    assert np.array_equal(bt, lt) and list(bn) == [v.value for v in ln], "%s: the batch call and the loop differ" % case.name
    tb, tl = [], []
    for i in range(warmup + reps):                  # alternating, the loop first
        t0 = time.perf_counter()
        loop()
        t1 = time.perf_counter()
        batch()
        t2 = time.perf_counter()
        if i >= warmup:
            tl.append(t1 - t0); tb.append(t2 - t1)
    m.close()
    row = dict(variant=case.variant, k=K, features=n, nodes=int(len(s.fv[0])), matches=int(bn.sum()), batch_ms=stats(tb), loop_ms=stats(tl))
    row["loop_over_batch"] = row["loop_ms"]["median"] / row["batch_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,5,20")
    ap.add_argument("--features", default="1000,2000")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_batch.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bow_batch: no GPU; nothing measured, nothing written")
    pkg = _pkg()
    ks = [int(k) for k in a.k.split(",")]
    rows = []
    for variant in ("frame", "kf"):
        for nfeat in [int(f) for f in a.features.split(",")]:
            full = working_case(variant, nfeat, max(ks))
            for k in ks:
                rows.append(run(pkg, full.first(k), a.reps, a.warmup))
                print(json.dumps(rows[-1]), flush=True)
    out = dict(tool="tools/bench_bow_batch.py", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               method="host-clock ms of the C calls, host arrays in and out; loop and batch alternate per repetition in one process after "
                      "warmup repetitions of both; median, 10th / 90th percentile and minimum over reps", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
