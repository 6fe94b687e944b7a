"""The OptimizeSim3 cases the tests share (tests/test_optimize_sim3_cpu.py, tests/test_optimize_sim3_gpu.py,
tests/tools/measure_sim3opt_spread.py), in the manner of tests/pose_cases.py.  A problem is the argument tuple of
my_slam_amd.OptimizeSim3: (x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale, S12).

scene(): one synthetic point cloud seen by two key frames.  x1c are the points in key frame 1, a known S12 (a rotation below 0.3
rad, a translation below 1 m, scale 1 or 1.3) takes x2c to x1c, both are projected with their own calibration and get pixel noise
0.7; a fifth of the pairs can be gross outliers (30..80 px off in image 1).  The starting value is the truth perturbed by a few
degrees, a few centimetres and, where the scale is free, a few percent.  Its quaternion is a unit one in double: the oracle keeps
matrices, and a quaternion off the unit sphere by a float's rounding would put the two on different parametrisations.

Condition on every problem: in the oracle, in both summation orders, no pair's chi2 at either flagging pass lies within 1e-3 * th2
of th2, and both orders flag the same pairs.  A seed that violates it is replaced by the next one; build() asserts the condition,
so identical flags are a fair demand on the product.

oracle(name) and host(ms, name) compute each case once and keep the results; nobody may change them."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimize_sim3_oracle as so  # noqa: E402
from pose_cases import KITTI, TUM1, SIGMA2  # noqa: E402

TH2 = 10.0                       # LoopClosing::ComputeSim3 calls with th2 = 10 (src/LoopClosing.cc:327)
MARGIN = 1e-3
SINGLE_SIZES = (0, 9, 10, 11, 63, 64, 65, 255, 256, 257, 600)
MIXED_SIZES = (0, 300, 9, 600, 11, 64, 10, 257, 40, 30, 0, 200, 65)
# (fix_scale, true scale) of the four variants of a size; each without and with outliers
VARIANTS = ((True, 1.0), (False, 1.0), (True, 1.3), (False, 1.3))


def rot(w):
    th = math.sqrt(float(w @ w))
    K = so.skew(w / th) if th > 0 else np.zeros((3, 3))
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def unit_quat(R):
    q = so.quat_from_R(R)
    return q / math.sqrt(float(q @ q))


def scene(rng, n, noise=0.7, n_wrong=0, K1=KITTI, K2=KITTI, scale=1.0, fix_scale=True, th2=TH2, perturb=True):
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    R = rot(rng.normal(size=3) * 0.1)
    t = rng.uniform(-0.6, 0.6, 3)
    x1 = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2, 2, n), rng.uniform(5, 20, n)], 1)
    x2 = ((x1 - t) @ R) / scale                               # x1 = s R x2 + t
    o1 = x1[:, :2] / x1[:, 2:3] * K1[:2] + K1[2:] + rng.normal(size=(n, 2)) * noise
    o2 = x2[:, :2] / x2[:, 2:3] * K2[:2] + K2[2:] + rng.normal(size=(n, 2)) * noise
    if n_wrong:
        o1[:n_wrong] += rng.uniform(30, 80, (n_wrong, 2)) * rng.choice([-1, 1], (n_wrong, 2))
    s1 = (1.0 / SIGMA2[rng.integers(0, 8, n)]).astype(np.float32)
    s2 = (1.0 / SIGMA2[rng.integers(0, 8, n)]).astype(np.float32)
    if perturb:
        dR = rot(rng.normal(size=3) * 0.03)                   # a few degrees
        dt = rng.normal(size=3) * 0.03                        # a few centimetres
        ds = 1.0 if fix_scale else math.exp(rng.normal() * 0.03)
    else:
        dR, dt, ds = np.eye(3), np.zeros(3), 1.0
    S12 = np.concatenate([unit_quat(dR @ R), dR @ t + dt, [scale * ds]])
    return (x1.astype(np.float32), x2.astype(np.float32), o1.astype(np.float32), o2.astype(np.float32), s1, s2,
            np.asarray(K1, np.float32), np.asarray(K2, np.float32), float(th2), bool(fix_scale), S12)


_ORACLE_OF = {}       # id(problem tuple) -> (S forward or None, flags, nIn, S reverse or None)


def checked(seed, make):
    """make(rng) with the first seed of seed, seed + 100000, ... whose problem meets the condition of the module comment"""
    for attempt in range(50):
        pr = make(np.random.default_rng(seed + 100000 * attempt))
        Sf, ff, nf, mf = so.optimize_sim3(*pr, order="forward")
        Sr, fr, nr, mr = so.optimize_sim3(*pr, order="reverse")
        if min(mf, mr) > MARGIN and np.array_equal(ff, fr) and nf == nr:
            assert min(mf, mr) > MARGIN and np.array_equal(ff, fr)
            ff.setflags(write=False)
            _ORACLE_OF[id(pr)] = (Sf, ff, nf, Sr)
            return pr
    raise AssertionError("no seed from %d on gives a problem away from its thresholds" % seed)


def single(n):
    """the eight problems of size n: the four VARIANTS, each without and with a fifth of gross outliers"""
    out = []
    for v, (fix, scale) in enumerate(VARIANTS):
        for wrong in (0, 1):
            out.append(checked(7000 + 16 * n + 2 * v + wrong,
                               lambda rng: scene(rng, n, n_wrong=(n // 5 if wrong else 0), scale=scale, fix_scale=fix,
                                                 K2=(TUM1 if v == 1 else KITTI))))
    return out


def mixed():
    """13 problems: two cameras, both fix_scale values, th2 10 and 5.991, outliers in every other one"""
    out = []
    for k, n in enumerate(MIXED_SIZES):
        fix, scale = VARIANTS[k % 4]
        out.append(checked(9100 + k, lambda rng: scene(rng, n, n_wrong=(n // 5 if k % 2 else 0), scale=scale, fix_scale=fix,
                                                       K1=(TUM1 if k in (3, 7) else KITTI), K2=(TUM1 if k in (5, 7) else KITTI),
                                                       th2=(5.991 if k % 3 == 1 else TH2))))
    return out


def too_few_left():
    """14 pairs, 6 of them gross outliers: the first pass leaves 8 < 10, so S12 comes back untouched (:1211-1212)"""
    return checked(4300, lambda rng: scene(rng, 14, n_wrong=6, fix_scale=False))


def fixed_point():
    """starts at the truth without noise: every pair is kept"""
    return checked(4400, lambda rng: scene(rng, 100, noise=0.0, fix_scale=False, perturb=False))


def bench_problems(B, n, seed=1):
    """B problems of n pairs in the loop-closing regime (not checked against the oracle): outliers in every other problem"""
    rng = np.random.default_rng(seed)
    return [scene(rng, n, n_wrong=(n // 5 if p % 2 else 0), fix_scale=(p % 3 != 2)) for p in range(B)]


def all_cases():
    cases = {"single_%d" % n: single(n) for n in SINGLE_SIZES}
    cases["mixed"] = mixed()
    cases["too_few_left"] = [too_few_left()]
    cases["fixed_point"] = [fixed_point()]
    return cases


_CASES = None
_HOST = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = all_cases()
    return _CASES


def oracle(name):
    """[(S12 forward or None, flags, nIn, S12 reverse or None)] of the oracle for the problems of case `name`"""
    return [_ORACLE_OF[id(pr)] for pr in cases()[name]]


def host(ms, name):
    """[(S12, flags, nIn)] of the host path orbp_optimize_sim3 for the problems of case `name`, computed once"""
    if name not in _HOST:
        res = []
        for pr in cases()[name]:
            S, f, n = ms.OptimizeSim3(*pr)
            S.setflags(write=False); f.setflags(write=False)
            res.append((S, f, n))
        _HOST[name] = res
    return _HOST[name]


def align(S, ref):
    """S with its quaternion's sign chosen as ref's (q and -q are one rotation)"""
    S = np.array(S, np.float64)
    if float(S[:4] @ np.asarray(ref)[:4]) < 0:
        S[:4] = -S[:4]
    return S


def diff3(a, b):
    """(quaternion, translation, scale): the largest per-entry differences of two S12"""
    a = align(a, b)
    d = np.abs(a - np.asarray(b, np.float64))
    return float(d[:4].max()), float(d[4:7].max()), float(d[7])


def assert_same(got, want, bars, what=""):
    """identical flags, identical nIn, S12 within the bars (quaternion, translation, scale) of tests/golden/sim3opt/tolerance.json"""
    S1, f1, n1 = got
    S2, f2, n2 = want
    flips = np.flatnonzero(np.asarray(f1, bool) != np.asarray(f2, bool))
    assert len(flips) == 0, "%s: %d flags differ, first at pair %d" % (what, len(flips), flips[0])
    assert n1 == n2, "%s: nIn %d != %d" % (what, n1, n2)
    if S2 is None:
        return
    d = diff3(S1, S2)
    for name, x, bar in zip(("quaternion", "translation", "scale"), d, bars):
        assert x <= bar, "%s: |d %s| = %.3g > %.3g" % (what, name, x, bar)
