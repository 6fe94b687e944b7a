"""The LocalBundleAdjustment cases the tests share (tests/test_lba_cpu.py, tests/test_lba_gpu.py, tests/test_lba_cxx.py,
tests/tools/measure_lba_spread.py), in the manner of tests/optimize_sim3_cases.py.  A problem is the dict of
my_slam_amd.pack_lba_problem.

scene(): key frames on a short sideways track looking at a point cloud 6 .. 20 m ahead, KITTI or TUM1 calibration per key frame
(tests/pose_cases.py), pixel noise 0.7, free poses perturbed by a few centimetres and tenths of a degree, points by a few
centimetres; a tenth of the observations can be gross outliers (30 .. 80 px).  A point's observers are a random subset of the key
frames in random order (the order of the reference's observations map is a pointer order).  Options plant the special structures:
a point whose every edge becomes level 1, a free key frame whose every edge becomes level 1, an edge that ends behind its camera,
and mild outliers, some of which end with a stale chi2 above and a fresh chi2 below the threshold.

Condition on every problem, asserted when the cases are built: in the oracle, in both summation orders, every decision (chi2 against
its threshold at both flagging passes, depth against 0, rho against 0 in every trial, (iniChi - currentChi) * 1e3 against iniChi)
stays at least 1e-3 (relative) from its boundary, both orders give the same flags, trial transcript and counts, and the case's own
predicate holds (the planted structure is there).  A seed that violates it is replaced by the next, at most 50 times; then the
build fails.  No case is dropped.

Every tolerance case fixes the scale: at least two fixed key frames, or stereo edges.  "gauge_mono" is monocular with the mnId == 0
key frame as its only fixed one: the scale is gauge, and it is compared on flags, counts and final chi2 only.

oracle(name) and host(ms, name) compute each case once and keep the results; nobody may change them."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_oracle as lo  # noqa: E402
from pose_cases import KITTI, TUM1, SIGMA2, BF_KITTI, BF_OTHER  # noqa: E402

MARGIN = 1e-3
CAM_KITTI = KITTI + (BF_KITTI,)
CAM_TUM1 = TUM1 + (BF_OTHER,)


def rot(w):
    th = math.sqrt(float(w @ w))
    K = lo.skew(w / th) if th > 0 else np.zeros((3, 3))
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def project(R, t, cam, X):
    pc = R @ X + t
    u = cam[0] * pc[0] / pc[2] + cam[2]
    return np.array([u, cam[1] * pc[1] / pc[2] + cam[3]]), u - cam[4] / pc[2], pc[2]


def scene(rng, n_free, n_fixed, n_points, kinds="mixed", outliers=0.0, local_id0=False, all_local_fixed=False, min_degree=2,
          bad_point=False, bad_kf=False, behind=False, mild=0.0, observers=None):
    """observers: every point is seen by that many key frames (None: about six, drawn per point, and the first point by all).
    kinds: "mono", "stereo" or "mixed" (each observation is stereo with probability 1/2).  local_id0: one more local key frame,
    fixed (mnId == 0).  bad_kf: one more free local key frame that sees 8 points at random pixels.  behind: one more free local
    key frame 13 m ahead of the others; a point 8 m ahead is behind it and is "observed" where the projection formula puts it."""
    n_local = n_free + (1 if local_id0 else 0) + (1 if bad_kf else 0) + (1 if behind else 0)
    NK = n_local + n_fixed
    local_fixed = np.zeros(n_local, np.uint8)
    if local_id0:
        local_fixed[n_free] = 1
    if all_local_fixed:
        local_fixed[:] = 1
    R, t, cam = [], [], []
    for k in range(NK):
        Rk = rot(rng.normal(size=3) * 0.04)
        c = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-0.3, 0.3), rng.uniform(-1, 1)])
        R.append(Rk); t.append(-Rk @ c)
        cam.append(CAM_TUM1 if k % 4 == 3 else CAM_KITTI)
    k_bad = n_free + (1 if local_id0 else 0) if bad_kf else -1
    k_behind = n_local - 1 if behind else -1
    if behind:
        c = np.array([0.2, 0.0, 13.0])
        t[k_behind] = -R[k_behind] @ c
    # inside a cone of 0.15 either side, so that every right-image coordinate of a stereo observation is positive
    X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(6, 20, n_points)], 1) if n_points else np.zeros((0, 3))
    X[:, 0] *= X[:, 2] / 20
    ordinary = [k for k in range(NK) if k not in (k_bad, k_behind)]
    edge_off, edge_kf, obs, ur, inv = [0], [], [], [], []
    top = len(ordinary)

    def add(k, p, uv, u_r, stereo, level=None):
        edge_kf.append(k); obs.append(uv); ur.append(abs(u_r) if stereo else -1.0)         # a gross outlier may cross 0: reflected
        inv.append(1.0 / SIGMA2[rng.integers(0, 8) if level is None else level])

    for p in range(n_points):
        if observers is not None:
            deg = min(observers, top)
        elif p == 0:
            deg = top                                          # one point seen by every key frame
        elif p == 1:
            deg = min(min_degree, top)
        else:
            deg = int(min(top, min_degree + rng.geometric(0.25) - 1))
        seen = list(rng.permutation(ordinary)[:deg])
        if behind and p >= 2 and X[p, 2] > 16.5:
            seen.insert(int(rng.integers(0, len(seen) + 1)), k_behind)
        for k in seen:
            uv, u_r, _ = project(R[k], t[k], cam[k], X[p])
            uv = uv + rng.normal(size=2) * 0.7
            u_r = u_r + rng.normal() * 0.7
            stereo = kinds == "stereo" or (kinds == "mixed" and rng.random() < 0.5)
            level = int(rng.integers(0, 8))
            if rng.random() < outliers:
                uv = uv + rng.uniform(30, 80, 2) * rng.choice([-1, 1], 2)
                u_r = u_r + rng.uniform(30, 80) * rng.choice([-1, 1])
            elif rng.random() < mild:
                a = rng.uniform(0, 2 * math.pi)           # a chi2 of 6.2 .. 12 before the noise
                uv = uv + math.sqrt(rng.uniform(6.2, 12.0) * SIGMA2[level]) * np.array([math.cos(a), math.sin(a)])
            add(k, p, uv, u_r, stereo, level)
        edge_off.append(len(edge_kf))
    extra = []
    if bad_point:                                              # three observers, each 60 .. 100 px off in its own direction
        Xb = np.array([0.5, 0.3, 10.0])
        rows = []
        for k in rng.permutation(ordinary)[:3]:
            uv, u_r, _ = project(R[k], t[k], cam[k], Xb)
            a = rng.uniform(0, 2 * math.pi)
            rows.append((k, uv + rng.uniform(60, 100) * np.array([math.cos(a), math.sin(a)]), u_r + rng.uniform(40, 80), kinds != "mono"))
        extra.append((Xb, rows))
    if behind:
        Xb = np.array([0.4, -0.2, 8.0])
        rows = []
        for k in list(rng.permutation(ordinary)[:3]) + [k_behind]:
            uv, u_r, _ = project(R[k], t[k], cam[k], Xb)
            rows.append((k, uv + rng.normal(size=2) * 0.7, u_r, False))
        extra.append((Xb, rows))
    for Xb, rows in extra:
        X = np.vstack([X, Xb[None]])
        for k, uv, u_r, stereo in rows:
            add(k, len(X) - 1, uv, u_r, stereo)
        edge_off.append(len(edge_kf))
    if bad_kf:                                                 # 8 of the points, seen at random pixels: appended to their observers
        pts = rng.choice(np.arange(2, n_points), 8, replace=False)
        per = [[(edge_kf[e], obs[e], ur[e], inv[e]) for e in range(edge_off[p], edge_off[p + 1])] for p in range(len(X))]
        for p in pts:
            per[p].append((k_bad, np.array([rng.uniform(0, 1200), rng.uniform(0, 370)]), -1.0, 1.0 / SIGMA2[rng.integers(0, 3)]))
        edge_off, edge_kf, obs, ur, inv = [0], [], [], [], []
        for rows in per:
            for k, uv, u_r, s in rows:
                edge_kf.append(k); obs.append(uv); ur.append(u_r); inv.append(s)
            edge_off.append(len(edge_kf))
    Tcw = np.zeros((NK, 4, 4), np.float32)
    for k in range(NK):
        Rk, tk = R[k], t[k]
        if k < n_local and not local_fixed[k]:
            dR = rot(rng.normal(size=3) * 0.003)              # tenths of a degree
            Rk, tk = dR @ Rk, dR @ tk + rng.normal(size=3) * 0.03
        Tcw[k, :3, :3], Tcw[k, :3, 3], Tcw[k, 3, 3] = Rk, tk, 1.0
    xw = (X + rng.normal(size=X.shape) * 0.03).astype(np.float32)
    return {"local_fixed": local_fixed, "Tcw": Tcw, "cam": np.asarray(cam, np.float32).reshape(NK, 5), "xw": xw.reshape(-1, 3),
            "edge_off": np.asarray(edge_off, np.int32), "edge_kf": np.asarray(edge_kf, np.int32),
            "obs": np.asarray(obs, np.float32).reshape(-1, 2), "u_right": np.asarray(ur, np.float32),
            "inv_sigma2": np.asarray(inv, np.float32), "k_bad": k_bad, "k_behind": k_behind}


_ORACLE_OF = {}       # id(problem) -> (forward result, reverse result)


def checked(seed, make, predicate=None):
    """make(rng) with the first seed of seed, seed + 100000, ... whose problem meets the condition of the module comment"""
    for attempt in range(50):
        pr = make(np.random.default_rng(seed + 100000 * attempt))
        f = lo.local_bundle_adjustment(pr, "forward")
        r = lo.local_bundle_adjustment(pr, "reverse")
        same = (np.array_equal(f["erase"], r["erase"]) and np.array_equal(f["level1"], r["level1"]) and f["transcript"] == r["transcript"]
                and all(f["stats"][k] == r["stats"][k] for k in ("iterations", "trials", "n_level1")))
        if min(f["margin"], r["margin"]) > MARGIN and same and (predicate is None or predicate(pr, f)):
            assert min(f["margin"], r["margin"]) > MARGIN and same
            for a in (f["erase"], f["level1"], f["Tcw"], f["xw"]):
                a.setflags(write=False)
            _ORACLE_OF[id(pr)] = (f, r)
            return pr
    raise AssertionError("no seed from %d on gives a problem that meets the condition" % seed)


def edges_of_kf(pr, k):
    return np.flatnonzero(pr["edge_kf"] == k)


def has_bad_point(pr, f):
    e0, e1 = pr["edge_off"][-2], pr["edge_off"][-1]
    return bool(f["level1"][e0:e1].all())


def has_bad_kf(pr, f):
    e = edges_of_kf(pr, pr["k_bad"])
    return len(e) == 8 and bool(f["level1"][e].all())


def has_behind(pr, f):
    e = int(pr["edge_off"][-1]) - 1                            # the last edge: the planted point in the key frame ahead of it
    return bool(f["erase"][e] and f["level1"][e] and f["stale_chi2"][e] < 0.5 * lo.TH_MONO)


def stale_flips(pr, f):
    """level-1 edges whose stale chi2 is above and whose chi2 at the final estimates is below the threshold, by a margin"""
    th = np.where(pr["u_right"] < 0, lo.TH_MONO, lo.TH_STEREO)
    return np.flatnonzero(f["level1"] & (f["stale_chi2"] > th) & (f["fresh_chi2"] < th * (1 - MARGIN)))


def has_stale_flip(pr, f):
    return len(stale_flips(pr, f)) > 0


def all_level1(pr, f):
    return bool(f["level1"].all()) and f["stats"]["iterations"] == (5, 0)


def ran_ten(pr, f):
    return f["stats"]["n_level1"] > 0 and f["stats"]["iterations"][1] >= 1


SPECS = {
    # name: (seed, scene arguments, predicate)
    "k1_p1_stereo": (100, dict(n_free=1, n_fixed=2, n_points=1, kinds="stereo"), None),
    "k1_p63_mono": (200, dict(n_free=1, n_fixed=3, n_points=63, kinds="mono"), None),
    "k2_p64_stereo": (300, dict(n_free=2, n_fixed=1, n_points=64, kinds="stereo"), None),
    "k2_p65_mixed": (400, dict(n_free=2, n_fixed=2, n_points=65, kinds="mixed", outliers=0.1), ran_ten),
    "k11_p257_mixed": (500, dict(n_free=11, n_fixed=6, n_points=257, kinds="mixed", outliers=0.1), ran_ten),
    "k43_p1500_mixed": (600, dict(n_free=43, n_fixed=10, n_points=1500, kinds="mixed", outliers=0.1), ran_ten),
    "bad_point": (700, dict(n_free=3, n_fixed=2, n_points=80, kinds="mixed", bad_point=True), has_bad_point),
    "bad_kf": (800, dict(n_free=3, n_fixed=2, n_points=80, kinds="mixed", bad_kf=True), has_bad_kf),
    "behind": (900, dict(n_free=3, n_fixed=2, n_points=80, kinds="mono", behind=True), has_behind),
    # four observers at least: a point that loses mild outliers still keeps a well-conditioned block
    "stale_flip": (1000, dict(n_free=3, n_fixed=3, n_points=120, kinds="mixed", mild=0.15, min_degree=4), has_stale_flip),
    "local_id0": (1100, dict(n_free=2, n_fixed=0, n_points=64, kinds="mixed", local_id0=True), None),
    "no_points": (1200, dict(n_free=2, n_fixed=1, n_points=0), None),
    # every key frame fixed: the points alone are optimised.  A problem of independent points converges to rounding within a few
    # iterations, where rho is noise; so every observation here is a gross outlier: the Huber round keeps moving for its five
    # iterations, every edge becomes level 1 and the second round has no active edge
    "no_free": (1300, dict(n_free=1, n_fixed=2, n_points=30, kinds="stereo", all_local_fixed=True, outliers=1.0), all_level1),
    "gauge_mono": (1400, dict(n_free=3, n_fixed=0, n_points=100, kinds="mono", local_id0=True), None),
}
NAMES = tuple(SPECS)


def density(pr, B=8):
    """(fewest edges of a key frame, share of the 6 B x 6 B tiles strictly below the diagonal of S that hold a non-zero 6 x 6 block):
    block (a, b) of S is non-zero where key frames a and b see a common point"""
    K = len(pr["local_fixed"])
    sees = np.zeros((K, len(pr["xw"])), bool)
    point_of = np.repeat(np.arange(len(pr["xw"])), np.diff(pr["edge_off"]))
    local = pr["edge_kf"] < K
    sees[pr["edge_kf"][local], point_of[local]] = True
    share = (sees.astype(np.int32) @ sees.T.astype(np.int32)) > 0
    T = (K + B - 1) // B
    tiles = [share[B * i:B * i + B, B * j:B * j + B].any() for i in range(T) for j in range(i)]
    return int(np.bincount(pr["edge_kf"], minlength=K)[:K].min()), float(np.mean(tiles))


def dense_and_ran_ten(pr, f):
    """no key frame without edges, every key frame with more than 64 (the lane stride of k_lba_reduce_kfs and k_lba_schur wraps),
    at least a quarter of S's tiles below the diagonal occupied, and a second round that ran after outliers were flagged"""
    fewest, tiles = density(pr)
    return fewest > 64 and tiles >= 0.25 and ran_ten(pr, f)


# The scale case: ORBM_LBA_MAX_LOCAL = 128 local key frames, all free (768 unknowns: three strides of the 256 threads of the
# one-workgroup k_lba_solve, a trailing triangle of 290 thousand entries), 8 fixed ones, 300 points each seen by a third of all key
# frames, a tenth of the observations gross outliers as in the `mixed` cases above.  A group of its own: it takes no part in the
# common spread or the case count of tolerance.json and has bars of its own there under "scale", made the same way.
SCALE_SPECS = {
    "scale_k128": (1500, dict(n_free=128, n_fixed=8, n_points=300, kinds="mixed", outliers=0.1, observers=136 // 3), dense_and_ran_ten),
}
SCALE_NAMES = tuple(SCALE_SPECS)
GAUGE = ("gauge_mono",)             # compared on flags, counts and final chi2 only
TOLERANCE_NAMES = tuple(n for n in NAMES if n not in GAUGE)

_CASES = {}
_HOST = {}


def case(name):
    if name not in _CASES:
        seed, args, pred = SPECS[name] if name in SPECS else SCALE_SPECS[name]
        _CASES[name] = checked(seed, lambda rng: scene(rng, **args), pred)
    return _CASES[name]


def cases():
    return {name: case(name) for name in NAMES}


def oracle(name):
    """(forward, reverse) results of tests/lba_oracle.py for case `name`"""
    return _ORACLE_OF[id(case(name))]


def host(ms, name):
    """(code, Tcw, xw, erase, stats) of the host path orbp_local_bundle_adjustment for case `name`, computed once"""
    if name not in _HOST:
        res = ms.LocalBundleAdjustment(case(name))
        for a in res[1:4]:
            a.setflags(write=False)
        _HOST[name] = res
    return _HOST[name]


def raw_call(fn, ms, pr, stop=None, guard=16, fill=0x5A):
    """a raw C call with guard bytes around every output -> (code, (Tcw, xw, erase, stats bytes), guards intact, packed arrays).
    fn(problem, Tcw, xw, erase, stop, stats) makes the call from ctypes arguments: the host path or a handle's GPU call"""
    s, a = ms.pack_lba_problem(pr)
    K, P, E = s.n_local, s.n_points, len(a["edge_kf"])
    T = np.full(16 * K + 2 * guard, np.float32(7.25), np.float32)
    x = np.full(3 * P + 2 * guard, np.float32(7.25), np.float32)
    x[guard:guard + 3 * P] = a["xw"].reshape(-1)
    er = np.full(E + 2 * guard, fill, np.uint8)
    st = np.full(40 + 2 * guard, fill, np.uint8)
    code = fn(C.byref(s), C.c_void_p(T.ctypes.data + 4 * guard), C.c_void_p(x.ctypes.data + 4 * guard), C.c_void_p(er.ctypes.data + guard),
              None if stop is None else stop.ctypes.data_as(C.c_void_p), C.c_void_p(st.ctypes.data + guard))
    ok = ((T[:guard] == 7.25).all() and (T[guard + 16 * K:] == 7.25).all() and (x[:guard] == 7.25).all() and (x[guard + 3 * P:] == 7.25).all()
          and (er[:guard] == fill).all() and (er[guard + E:] == fill).all() and (st[:guard] == fill).all() and (st[guard + 40:] == fill).all())
    return code, (T[guard:guard + 16 * K], x[guard:guard + 3 * P], er[guard:guard + E], st[guard:guard + 40]), ok, a


def diffs(Tcw, xw, chi2, ref_Tcw, ref_xw, ref_chi2):
    """(rotation entries, translation, point coordinates, final chi2 relative): the largest differences"""
    Tcw, ref_Tcw = np.asarray(Tcw, np.float64).reshape(-1, 4, 4), np.asarray(ref_Tcw, np.float64).reshape(-1, 4, 4)
    xw, ref_xw = np.asarray(xw, np.float64).reshape(-1, 3), np.asarray(ref_xw, np.float64).reshape(-1, 3)
    dr = float(np.abs(Tcw[:, :3, :3] - ref_Tcw[:, :3, :3]).max()) if len(Tcw) else 0.0
    dt = float(np.abs(Tcw[:, :3, 3] - ref_Tcw[:, :3, 3]).max()) if len(Tcw) else 0.0
    dx = float(np.abs(xw - ref_xw).max()) if len(xw) else 0.0
    dc = abs(chi2 - ref_chi2) / abs(ref_chi2) if ref_chi2 != 0 else abs(chi2)
    return dr, dt, dx, dc


KEYS = ("rotation", "translation", "point", "chi2_relative")
FLOAT_ULP = 2.0 ** -23


def assert_same(got, want_Tcw, want_xw, want_erase, want_stats, bars, what, coordinates=True, float_roundings=1):
    """identical erase flags and counts; poses, points and final chi2 within the bars of tests/golden/lba/tolerance.json.  The
    product's poses and points are floats: each side that was rounded to float adds half a float ulp of the largest magnitude
    compared (float_roundings = 1 against the oracle's doubles, 2 between two float results)."""
    code, Tcw, xw, erase, stats = got
    assert code == 0, what
    flips = np.flatnonzero(np.asarray(erase, bool) != np.asarray(want_erase, bool))
    assert len(flips) == 0, "%s: %d erase flags differ, first at edge %d" % (what, len(flips), flips[0])
    for k in ("iterations", "trials", "n_level1", "second_round"):
        assert tuple(np.atleast_1d(stats[k])) == tuple(np.atleast_1d(want_stats[k])), "%s: %s %s != %s" % (what, k, stats[k], want_stats[k])
    d = diffs(Tcw, xw, stats["chi2"], want_Tcw, want_xw, want_stats["chi2"])
    scale = (1.0, float(np.abs(np.asarray(want_Tcw, np.float64).reshape(-1, 4, 4)[:, :3, 3]).max()) if len(want_Tcw) else 0.0,
             float(np.abs(want_xw).max()) if len(want_xw) else 0.0, 0.0)
    for name, x, bar, s in zip(KEYS, d, bars, scale):
        if not coordinates and name != "chi2_relative":
            continue
        allowed = bar + float_roundings * 0.5 * FLOAT_ULP * s
        print("%s: |d %s| = %.3g (bar %.3g + float rounding %.3g)" % (what, name, x, bar, allowed - bar))
        assert x <= allowed, "%s: |d %s| = %.3g > %.3g" % (what, name, x, allowed)
