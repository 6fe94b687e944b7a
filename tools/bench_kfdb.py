#!/usr/bin/env python3
"""Cost of the keyframe-database queries (include/orbk.h) on one GPU.

Workload: maps of 1 000, 5 000 and 20 000 keyframes, each a BowVector of about 1 000 entries over a 1 000 000-word vocabulary
with Zipf-distributed word ids (a few words appear in most keyframes, as in a real DBoW2 vocabulary, so most keyframes share
some word with any query), and 2 000-entry queries.  Every keyframe has 10 random covisibility neighbours.

Reports the median host-clock ms of DetectRelocalizationCandidates and DetectLoopCandidates through the Python wrapper
(*_ms_median: end to end, including the wrapper's building of the neighbour lists) and of the library alone
(*_lib_ms_median: orbk_query_begin + orbk_query_end timed around the C calls; each ends in a device synchronisation or
runs on the host only; warm-up calls first) and, per query, the bytes the scoring kernel must move: 4 B per keyframe entry (every
word id is read) plus 8 B per matched keyframe value.  With --kernel-stats (a rocprofv3 --kernel-trace --stats CSV of a run
of this tool with --sizes N) it adds the kernel's mean time and its bytes against the 8 TB/s HBM peak for that size.
There is no CPU baseline and no speed target: the numbers are what one run measured.

usage: tools/bench_kfdb.py [--sizes 1000,5000,20000] [--reps 30] [--out profiles/kfdb_bench.json] [--kernel-stats CSV]
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
HBM_PEAK = 8.0e12
NWORDS = 1_000_000
KF_ENTRIES = 1000
QUERY_ENTRIES = 2000


def _pkg():
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(ROOT, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def zipf_bow(rng, perm, n, a=1.1):
    ids = np.zeros(0, np.int64)
    while len(ids) < n:
        r = rng.zipf(a, 4 * n) - 1
        ids = np.unique(np.concatenate([ids, perm[r[r < len(perm)]]]))
    ids = np.sort(rng.choice(ids, n, replace=False)).astype(np.int32)
    v = rng.random(n) + 1e-3
    return ids, v / v.sum()


def kernel_stats(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_kfdb_score" in row["Name"]:
                return int(row["Calls"]), float(row["AverageNs"])
    raise SystemExit("%s: no k_kfdb_score row" % path)


def run(pkg, nkf, reps, warmup, seed=0):
    rng = np.random.default_rng(seed + nkf)
    perm = rng.permutation(NWORDS)
    db = pkg.KeyFrameDatabase(NWORDS, max_keyframes=nkf, max_entries=nkf * KF_ENTRIES)
    entries = 0
    for k in range(1, nkf + 1):
        b = zipf_bow(rng, perm, int(rng.integers(KF_ENTRIES - 100, KF_ENTRIES + 101)))
        db.add(k, b)
        entries += len(b[0])
    covis = {k: [int(x) for x in rng.integers(1, nkf + 1, 10)] for k in range(1, nkf + 1)}
    queries = [zipf_bow(rng, perm, QUERY_ENTRIES) for _ in range(8)]
    rec = [db.score(q) for q in queries]
    matched = float(np.mean([r["words"].sum() for r in rec]))
    t_reloc, t_loop, ncand = [], [], []
    for i in range(warmup + reps):
        q = queries[i % len(queries)]
        t0 = time.perf_counter()
        c = db.DetectRelocalizationCandidates(1_000_000 + i, q, covis)
        t1 = time.perf_counter()
        db.DetectLoopCandidates(2_000_000 + i, q, covis[1 + i % nkf][:5], 0.0, covis)
        t2 = time.perf_counter()
        if i >= warmup:
            t_reloc.append((t1 - t0) * 1e3); t_loop.append((t2 - t1) * 1e3); ncand.append(len(c))
    # the library alone: the two C calls timed around themselves, the neighbour arrays built between them untimed
    L = db.L
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    sc = np.zeros(nkf, np.uint64); si = np.zeros(nkf, np.float32); cand = np.zeros(nkf, np.uint64)
    n = C.c_int(); nc = C.c_int()
    lib_ms = {pkg.ORBK_RELOC: [], pkg.ORBK_LOOP: []}
    for i in range(warmup + reps):
        q = queries[i % len(queries)]
        for kind in (pkg.ORBK_RELOC, pkg.ORBK_LOOP):
            conn = np.array(covis[1 + i % nkf][:5] if kind == pkg.ORBK_LOOP else [], np.uint64)
            t0 = time.perf_counter()
            rc = L.orbk_query_begin(db.h, kind, 3_000_000 + 2 * i + kind, p(q[0]), p(q[1]), len(q[0]), p(conn), len(conn), 0.0,
                                    p(sc), p(si), nkf, C.byref(n))
            t1 = time.perf_counter()
            nb = [covis[int(k)] for k in sc[:n.value]]
            off = np.zeros(len(nb) + 1, np.int32)
            off[1:] = np.cumsum([len(x) for x in nb])
            nb_ids = np.array([x for l in nb for x in l], np.uint64)
            t2 = time.perf_counter()
            rc2 = L.orbk_query_end(db.h, kind, p(off), p(nb_ids), p(cand), nkf, C.byref(nc))
            t3 = time.perf_counter()
            if rc != 0 or rc2 != 0:
                raise SystemExit("orbk status %d / %d: %s" % (rc, rc2, L.orbk_last_error().decode()))
            if i >= warmup:
                lib_ms[kind].append((t1 - t0 + t3 - t2) * 1e3)
    return dict(keyframes=nkf, entries=entries, query_entries=QUERY_ENTRIES,
                records_per_query=float(np.mean([len(r) for r in rec])), matched_entries_per_query=matched,
                kernel_bytes_per_query=int(4 * entries + 8 * matched),
                reloc_ms_median=float(np.median(t_reloc)), loop_ms_median=float(np.median(t_loop)),
                reloc_lib_ms_median=float(np.median(lib_ms[pkg.ORBK_RELOC])), loop_lib_ms_median=float(np.median(lib_ms[pkg.ORBK_LOOP])),
                reloc_ms_min=float(np.min(t_reloc)), loop_ms_min=float(np.min(t_loop)),
                reloc_candidates_median=float(np.median(ncand)), reps=reps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000,20000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    pkg = _pkg()
    sizes = [int(s) for s in a.sizes.split(",")]
    results = [run(pkg, n, a.reps, a.warmup) for n in sizes]
    out = dict(tool="tools/bench_kfdb.py", nwords=NWORDS, keyframe_entries=KF_ENTRIES, zipf_a=1.1, results=results,
               note="single run; host clock around synchronised calls; *_ms_median = Python end to end, *_lib_ms_median = the two C calls alone; no CPU baseline of the reference's database")
    if a.kernel_stats:
        calls, avg_ns = kernel_stats(a.kernel_stats)
        r = results[-1]
        out["kernel"] = dict(keyframes=r["keyframes"], name="k_kfdb_score", calls=calls, avg_us=avg_ns / 1e3,
                             bytes=r["kernel_bytes_per_query"], achieved_TBps=r["kernel_bytes_per_query"] / (avg_ns * 1e-9) / 1e12,
                             hbm_peak_fraction=r["kernel_bytes_per_query"] / (avg_ns * 1e-9) / HBM_PEAK,
                             source=os.path.basename(a.kernel_stats))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
