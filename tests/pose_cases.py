"""The PoseOptimization cases the batch tests share (tests/test_pose_batch_cpu.py, tests/test_pose_batch_gpu.py,
tests/test_pose_batch_cxx.py).  scene() is the generator of tests/test_pose.py (the calibration is an argument here, the random
draws are the same), and problem() is the body of test_pose_optimization_equals_oracle: noise 0.7, every other trial with n/5
gross outliers, the last two trials with stereo edges mixed in (u_right[::3] = -1).  A problem is the argument tuple of
my_slam_amd.PoseOptimization: (obs, inv_sigma2, xw, fx, fy, cx, cy, Tcw, u_right, bf).

host(ms, key) runs the host path orbp_pose_optimization once per case and keeps the result; nobody may change it."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pose_oracle as po  # noqa: E402

KITTI = (718.856, 718.856, 607.1928, 185.2157)             # KITTI 00-02 (Examples/Monocular/KITTI00-02.yaml)
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)   # another camera (Examples/Monocular/TUM1.yaml)
BF_KITTI, BF_OTHER = 386.1448, 40.0
SIGMA2 = (1.2 ** np.arange(8)) ** 2
TRIALS = 6

SINGLE_SIZES = (0, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 1500)
MIXED_SIZES = (0, 300, 2, 1500, 9, 64, 10, 257, 3, 30, 0, 200, 65)


def scene(rng, n, noise=0.0, n_wrong=0, K=KITTI, rot=None):
    """rot = (axis, angle) sets the true rotation; without it the axis is random and the angle below 0.5 rad"""
    fx, fy, cx, cy = K
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0, 0.5)
    if rot is not None:
        ax, ang = np.asarray(rot[0], np.float64) / np.linalg.norm(rot[0]), rot[1]
    Kx = po._skew(ax)
    R = np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * Kx @ Kx
    t = rng.uniform(-1, 1, 3)
    pc = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2, 2, n), rng.uniform(4, 20, n)], 1)
    pw = (pc - t) @ R
    u = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1) + rng.normal(size=(n, 2)) * noise
    if n_wrong:
        u[:n_wrong] += rng.uniform(30, 80, (n_wrong, 2)) * rng.choice([-1, 1], (n_wrong, 2))
    return R, t, pw, u


def T_of(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def problem(rng, n, trial, K=KITTI, bf=BF_KITTI, n_wrong=None, rot=None):
    """one trial of test_pose_optimization_equals_oracle; n_wrong overrides the n/5 of the odd trials"""
    if n_wrong is None:
        n_wrong = n // 5 if trial % 2 else 0
    R, t, pw, u = scene(rng, n, noise=0.7, n_wrong=n_wrong, K=K, rot=rot)
    inv_s2 = (1.0 / SIGMA2[rng.integers(0, 8, n)]).astype(np.float32)
    dR, dt = po._se3_exp(np.concatenate([rng.normal(size=3) * 0.02, rng.normal(size=3) * 0.1]))
    T0 = T_of(dR @ R, dR @ t + dt)
    ur, use_bf = None, 0.0
    if trial >= 4 and n:                                   # stereo edges mixed in (mvuRight >= 0)
        use_bf = bf
        pc = pw @ R.T + t
        ur = (u[:, 0] - use_bf / pc[:, 2] + rng.normal(size=n) * 0.5).astype(np.float32)
        ur[::3] = -1
    return (u.astype(np.float32), inv_s2, pw.astype(np.float32), K[0], K[1], K[2], K[3], T0, ur, use_bf)


def single(n):
    """the TRIALS problems of size n, seeded as tests/test_pose.py seeds them"""
    rng = np.random.default_rng(500 + n)
    return [problem(rng, n, trial) for trial in range(TRIALS)]


def mixed():
    """13 problems: mono and stereo-mixed, outliers in every other one, two values of bf and one camera with other intrinsics"""
    rng = np.random.default_rng(77)
    out = []
    for k, n in enumerate(MIXED_SIZES):
        trial = (1, 4, 0, 5)[k % 4] if n else 0            # outliers / stereo / clean / stereo with outliers
        K = TUM1 if k == 7 else KITTI
        bf = BF_OTHER if k in (3, 7, 11) else BF_KITTI
        out.append(problem(rng, n, trial, K=K, bf=bf))
    return out


def all_outliers():
    """every observation is a gross outlier and all of them are flagged before the last round: the active set is empty then,
    optimize() is skipped and the pose that comes back is the one that went in (tests/test_pose_batch_cpu.py asserts both)"""
    return problem(np.random.default_rng(43), 40, 0, n_wrong=40)


def fixed_point():
    """starts at the truth without noise (tests/test_pose.py, the fixed-point test)"""
    rng = np.random.default_rng(9)
    R, t, pw, u = scene(rng, 100)
    return (u.astype(np.float32), np.ones(100, np.float32), pw.astype(np.float32), *KITTI, T_of(R, t), None, 0.0)


LARGE_ANGLES = (2.2, 2.9, 3.1)


def large_rotation():
    """18 problems of 64 observations whose true rotation is LARGE_ANGLES about axes 0.05 off x, y and z, clean and with n/5
    outliers: the trace of R is negative, so Quaterniond(Matrix3d) takes its three branches on the largest diagonal entry, which
    no rotation below 0.5 rad reaches"""
    rng = np.random.default_rng(29)
    out = []
    for a in range(3):
        ax = np.zeros(3)
        ax[a], ax[(a + 1) % 3] = 1.0, 0.05
        for ang in LARGE_ANGLES:
            out += [problem(rng, 64, trial, rot=(ax, ang)) for trial in (0, 1)]
    return out


def bench_problems(B, n, seed=1):
    """B problems of n observations in the tracking regime: a fifth of them outliers in every other problem, stereo in every third"""
    rng = np.random.default_rng(seed)
    return [problem(rng, n, (1, 0, 4)[p % 3]) for p in range(B)]


def all_cases():
    """name -> list of problems: every case the GPU tests use"""
    cases = {"single_%d" % n: single(n) for n in SINGLE_SIZES}
    cases["mixed"] = mixed()
    cases["all_outliers"] = [all_outliers()]
    cases["fixed_point"] = [fixed_point()]
    cases["large_rotation"] = large_rotation()
    return cases


_CASES = None
_HOST = {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = all_cases()
    return _CASES


def host(ms, name):
    """[(Tcw, outlier, n_good)] of the host path for the problems of case `name`, computed once"""
    if name not in _HOST:
        res = []
        for pr in cases()[name]:
            T, o, n = ms.PoseOptimization(*pr)
            T.setflags(write=False); o.setflags(write=False)
            res.append((T, o, n))
        _HOST[name] = res
    return _HOST[name]


def edge_chi2(pr, T, i):
    """the fp64 chi2 of observation i of problem pr at pose T (for a failure message: how close to its threshold the edge is)"""
    obs, inv_s2, xw, fx, fy, cx, cy, _, ur, bf = pr
    pc = T[:3, :3].astype(np.float64) @ xw[i].astype(np.float64) + T[:3, 3].astype(np.float64)
    e = [obs[i, 0] - (fx * pc[0] / pc[2] + cx), obs[i, 1] - (fy * pc[1] / pc[2] + cy)]
    if ur is not None and ur[i] >= 0:
        e.append(ur[i] - (fx * pc[0] / pc[2] + cx - bf / pc[2]))
    return float(np.dot(e, e) * inv_s2[i])


def assert_same(got, want, pr, what=""):
    """the bar of tests/test_pose.py for this function: |dTcw| <= 2e-6 per entry, flags identical, n_good identical"""
    T1, o1, n1 = got
    T2, o2, n2 = want
    flips = np.flatnonzero(np.asarray(o1, bool) != np.asarray(o2, bool))
    assert len(flips) == 0, "%s: %d flags differ; first edge %d has chi2 %.9g at the host's pose (thresholds 5.991 / 7.815)" % (
        what, len(flips), flips[0], edge_chi2(pr, T2, flips[0]))
    assert n1 == n2, "%s: n_good %d != %d" % (what, n1, n2)
    d = float(np.abs(np.asarray(T1, np.float64) - np.asarray(T2, np.float64)).max())
    assert d <= 2e-6, "%s: |dTcw| = %.3g" % (what, d)
