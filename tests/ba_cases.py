"""The BundleAdjustment cases the tests share (tests/test_ba_cpu.py, tests/test_ba_gpu.py, tests/tools/measure_ba_spread.py), in
the manner of tests/lba_cases.py, whose scene() builds them.  A problem is the dict of my_slam_amd.pack_lba_problem, gathered as
src/Optimizer.cc:71-184 walks: every key frame is "local", the one with mnId == 0 is fixed, n_fixed is normally 0.  A case is
(problem, n_iterations, robust).

The shapes follow the solver of csrc/orbm_spd.hip, whose panel is NB = 48 unknowns = B = 8 key frames: 1, B - 1, B, B + 1 and
3 B + 1 free key frames (with the fixed one 2, 8, 9, 10 and 26 blocks of the reduced system: one panel exactly filled, one row
over, and four panels with a ragged last one); a point's observers are a random subset of all key frames, so the off-diagonal panels
of the largest case are not empty.  Points: 0, 1, 63 / 64 / 65, 400.  SCALE_SPECS, further down, holds three dense cases of 49,
89 and 512 blocks: a group of its own with bars of its own.

Condition on every case, asserted when it is built: in the oracle (tests/ba_oracle.py), in both summation orders, every decision
stays at least 1e-3 (relative) from its boundary, both orders give the same transcript and counts, and the case's own predicate
holds.  A seed that violates it is replaced by the next, at most 50 times; then the build fails.  No case is dropped.

Every tolerance case fixes the scale: stereo edges, or two fixed key frames.  GAUGE cases (the monocular two-key-frame initial map,
and a map without any fixed key frame) are compared on counts and final chi2 only.

oracle(name) and host(ms, name) compute each case once and keep the results; nobody may change them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_oracle as bo  # noqa: E402
import lba_cases as lc  # noqa: E402

MARGIN = lc.MARGIN
NB, B = 48, 8                        # SPD_NB of csrc/orbm_spd.hip and the key frames of one panel
KEYS, FLOAT_ULP, diffs = lc.KEYS, lc.FLOAT_ULP, lc.diffs


def scene(rng, n_free, n_points, kinds="mixed", outliers=0.0, fixed_at=None, n_fixed=0, id0=True, all_fixed=False, empty=False,
          observers=None):
    """lba_cases.scene() with the mnId == 0 key frame moved to position fixed_at of the list (None: the end, where scene() puts
    it).  empty: one more free key frame and one more point, both without edges, the point in the middle of the list."""
    pr = lc.scene(rng, n_free=n_free, n_fixed=n_fixed, n_points=n_points, kinds=kinds, outliers=outliers, local_id0=id0,
                  all_local_fixed=all_fixed, observers=observers)
    pr = {k: v for k, v in pr.items() if k not in ("k_bad", "k_behind")}
    K = len(pr["local_fixed"])
    if id0 and fixed_at is not None and fixed_at != K - 1:
        order = list(range(K - 1))
        order.insert(fixed_at, K - 1)                        # new position -> old index
        order += list(range(K, len(pr["Tcw"])))
        new_of = np.empty(len(order), np.int32)
        new_of[order] = np.arange(len(order), dtype=np.int32)
        pr["local_fixed"] = pr["local_fixed"][order[:K]]
        pr["Tcw"], pr["cam"] = pr["Tcw"][order], pr["cam"][order]
        pr["edge_kf"] = new_of[pr["edge_kf"]]
    if empty:
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = lc.rot(np.array([0.02, -0.03, 0.01])).astype(np.float32)
        T[:3, 3] = (0.3, -0.1, 0.2)
        pr["edge_kf"] = np.where(pr["edge_kf"] >= K, pr["edge_kf"] + 1, pr["edge_kf"]).astype(np.int32)
        pr["local_fixed"] = np.concatenate([pr["local_fixed"], np.zeros(1, np.uint8)])
        pr["Tcw"] = np.concatenate([pr["Tcw"][:K], T[None], pr["Tcw"][K:]])
        pr["cam"] = np.concatenate([pr["cam"][:K], pr["cam"][:1], pr["cam"][K:]])
        at = len(pr["xw"]) // 2
        pr["xw"] = np.concatenate([pr["xw"][:at], np.array([[0.123, -0.456, 7.89]], np.float32), pr["xw"][at:]])
        pr["edge_off"] = np.concatenate([pr["edge_off"][:at + 1], pr["edge_off"][at:]]).astype(np.int32)
        pr["empty_kf"], pr["empty_point"] = K, at
    return pr


_ORACLE_OF = {}


def checked(seed, make, variants):
    """variants: [(n_iterations, robust, predicate)]: one problem that meets the condition under each of them"""
    for attempt in range(50):
        pr = make(np.random.default_rng(seed + 100000 * attempt))
        found = {}
        for n_iterations, robust, predicate in variants:
            f = bo.bundle_adjustment(pr, n_iterations, robust, "forward")
            r = bo.bundle_adjustment(pr, n_iterations, robust, "reverse")
            same = f["transcript"] == r["transcript"] and all(f["stats"][k] == r["stats"][k] for k in ("iterations", "trials"))
            if not (min(f["margin"], r["margin"]) > MARGIN and same and (predicate is None or predicate(pr, f))):
                break
            for a in (f["Tcw"], f["xw"]):
                a.setflags(write=False)
            found[(id(pr), n_iterations, bool(robust))] = (f, r)
        else:
            _ORACLE_OF.update(found)
            return pr
    raise AssertionError("no seed from %d on gives a problem that meets the condition" % seed)


def ran_all(pr, f):
    return f["stats"]["iterations"] >= 1


def by_nbad(pr, f):
    return f["ended_by_nbad"]


def rejects(pr, f):
    return f["stats"]["trials"] > f["stats"]["iterations"]


_OUTLIER_SCENE = dict(n_free=B, n_points=64, kinds="mixed", outliers=0.1, fixed_at=3)
SPECS = {
    # name: (seed, scene arguments, n_iterations, robust, predicate)
    "init_map_mono": (100, dict(n_free=1, n_points=150, kinds="mono"), 20, True, ran_all),           # src/Tracking.cc:695
    # one point: three more key frames that only constrain it (n_fixed) keep the problem over-determined (15 residuals, 9 unknowns),
    # so that the final chi2 is not a zero to rounding, of which no relative comparison can be made
    "k1_p1_stereo": (200, dict(n_free=1, n_fixed=3, n_points=1, kinds="stereo"), 10, True, ran_all),
    "k1_p0": (300, dict(n_free=1, n_points=0), 10, True, None),
    "k7_p63_stereo": (400, dict(n_free=B - 1, n_points=63, kinds="stereo", fixed_at=0), 10, False, ran_all),
    "k8_p64_robust": (500, _OUTLIER_SCENE, 10, True, ran_all),
    "k8_p64_plain": (500, _OUTLIER_SCENE, 10, False, ran_all),                                       # the same problem, no kernel
    "k9_p65_mixed": (600, dict(n_free=B + 1, n_points=65, kinds="mixed", fixed_at=5), 1, False, ran_all),
    "k25_p400_mixed": (700, dict(n_free=3 * B + 1, n_points=400, kinds="mixed", fixed_at=13), 10, False, ran_all),   # LoopClosing.cc:651
    "iterations_0": (800, dict(n_free=2, n_points=40, kinds="stereo"), 0, True, None),
    "nbad_stops": (900, dict(n_free=2, n_points=40, kinds="stereo"), 20, True, by_nbad),
    "rejecting": (1000, dict(n_free=1, n_fixed=2, n_points=30, kinds="stereo", id0=False, all_fixed=True, outliers=1.0), 5, True, rejects),
    "empty_vertices": (1100, dict(n_free=3, n_points=64, kinds="mixed", empty=True), 10, True, ran_all),
    "n_fixed_2": (1200, dict(n_free=B, n_fixed=2, n_points=65, kinds="mixed", id0=False), 10, True, ran_all),
    "no_fixed_gauge": (1300, dict(n_free=3, n_points=80, kinds="stereo", id0=False), 10, False, ran_all),
}
NAMES = tuple(SPECS)
GAUGE = ("init_map_mono", "no_fixed_gauge")
TOLERANCE_NAMES = tuple(n for n in NAMES if n not in GAUGE)
LARGEST = "k25_p400_mixed"


# The scale cases: reduced systems that csrc/orbm_spd.hip solves with a second and a third workgroup of k_spd_backward (49 and 89
# blocks: 294 and 534 unknowns) and at ORBM_BA_MAX_KFS (512 blocks, 3072 unknowns = ORBM_SPD_MAX_N), this time with edges.  A group
# of its own: the stop sweeps, the spread over NAMES and the case count of tolerance.json stay as they are, and each has bars of
# its own there under "scale" (4 x the spread of the oracle's two orders on that case alone: the spread grows with the condition
# of the system, and a pooled bar would let the small cases hide behind the large ones).
# Density is a condition of these cases (dense_enough): lba_cases.scene() gives a point about six observers, which at 512 key
# frames leaves S almost block-diagonal; here 300 points are each seen by a third of all key frames.
# One iteration at the larger two; two at the smallest, so that an accepted step feeds a second linearisation.
density = lc.density


def dense_enough(pr, f):
    """no key frame without edges, every key frame with more than 64 (the lane stride of k_lba_reduce_kfs and k_lba_schur wraps),
    at least a quarter of S's tiles below the diagonal occupied, and an iteration that ran"""
    fewest, tiles = density(pr)
    return fewest > 64 and tiles >= 0.25 and ran_all(pr, f)


SCALE_POINTS = 300
SCALE_SPECS = {
    "scale_k49": (2000, dict(n_free=48, n_points=SCALE_POINTS, kinds="mixed", fixed_at=20, observers=49 // 3), 2, False, dense_enough),
    "scale_k89": (2100, dict(n_free=88, n_points=SCALE_POINTS, kinds="mixed", fixed_at=50, observers=89 // 3), 1, True, dense_enough),
    "scale_k512": (2200, dict(n_free=511, n_points=SCALE_POINTS, kinds="mixed", fixed_at=300, observers=512 // 3), 1, False, dense_enough),
}
SCALE_NAMES = tuple(SCALE_SPECS)
AT_THE_CAP = "scale_k512"

_CASES = {}
_HOST = {}


SAME_PROBLEM = ("k8_p64_robust", "k8_p64_plain")     # one scene under both settings of `robust`


def case(name):
    """(problem, n_iterations, robust)"""
    if name not in _CASES:
        group = SAME_PROBLEM if name in SAME_PROBLEM else (name,)
        specs = SCALE_SPECS if name in SCALE_SPECS else SPECS
        seed, args = specs[group[0]][:2]
        assert all(specs[n][:2] == (seed, args) for n in group)
        pr = checked(seed, lambda rng: scene(rng, **args), [specs[n][2:] for n in group])
        for n in group:
            _CASES[n] = (pr, specs[n][2], specs[n][3])
    return _CASES[name]


def oracle(name):
    """(forward, reverse) results of tests/ba_oracle.py for case `name`"""
    pr, n_it, robust = case(name)
    return _ORACLE_OF[(id(pr), n_it, bool(robust))]


def host(ms, name):
    """(code, Tcw, xw, stats) of the host path orbp_bundle_adjustment for case `name`, computed once"""
    if name not in _HOST:
        pr, n_it, robust = case(name)
        res = ms.BundleAdjustment(pr, n_it, robust)
        for a in res[1:3]:
            a.setflags(write=False)
        _HOST[name] = res
    return _HOST[name]


def assert_same(got, want_Tcw, want_xw, want_stats, bars, what, coordinates=True, float_roundings=1):
    """identical counts; poses, points and final chi2 within the bars of tests/golden/ba/tolerance.json plus half a float ulp of the
    largest magnitude compared for each side that was rounded to float (lba_cases.assert_same has the rule)"""
    code, Tcw, xw, stats = got
    assert code == 0, what
    for k in ("iterations", "trials"):
        assert stats[k] == want_stats[k], "%s: %s %s != %s" % (what, k, stats[k], want_stats[k])
    d = diffs(Tcw, xw, stats["chi2"], want_Tcw, want_xw, want_stats["chi2"])
    scale = (1.0, float(np.abs(np.asarray(want_Tcw, np.float64).reshape(-1, 4, 4)[:, :3, 3]).max()) if len(want_Tcw) else 0.0,
             float(np.abs(want_xw).max()) if len(want_xw) else 0.0, 0.0)
    for name, x, bar, s in zip(KEYS, d, bars, scale):
        if not coordinates and name != "chi2_relative":
            continue
        allowed = bar + float_roundings * 0.5 * FLOAT_ULP * s
        print("%s: |d %s| = %.3g (bar %.3g + float rounding %.3g)" % (what, name, x, bar, allowed - bar))
        assert x <= allowed, "%s: |d %s| = %.3g > %.3g" % (what, name, x, allowed)
