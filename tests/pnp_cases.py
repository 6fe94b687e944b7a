"""Deterministic PnPsolver cases shared by test_pnp_batch_cpu.py and test_pnp_batch_gpu.py.

A case: a planted camera pose, N world points at depths of 4 to 200 m in front of the camera, keypoint octaves 0..7 (so the
thresholds differ), `wrong` mismatched correspondences moved 30-80 px, pixel noise or none, its own calibration, and the samples
PnPsolver::iterate would draw (src/PnPsolver.cc:188-204: swap with back, pop) from the scripted source of tests/test_pose.py.
The tests compare the GPU call, the replay and the host solver with each other byte for byte, so nothing here needs to be
well-conditioned; the cases only have to reach the code paths (mask words, sample sizes, the rank-deficient absolute orientation)."""
import math

import numpy as np

RAND_MAX = 2147483647
SIGMA2 = ((np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)
K_KITTI = (718.856, 718.856, 607.1928, 185.2157)
K_TUM = (517.3, 516.5, 318.6, 255.3)
K_EUROC = (458.654, 457.296, 367.215, 248.375)
RELOC = (0.99, 10, 300, 4, 0.5, 5.991)          # Tracking.cc:1393 SetRansacParameters(0.99,10,300,4,0.5,5.991)


class Lcg:
    """deterministic stand-in for libc rand() (31-bit): the generator of tests/test_pose.py and tools/gen_pnp_golden.py"""
    MAX = RAND_MAX

    def __init__(self, seed):
        self.s = seed

    def __call__(self):
        self.s = (self.s * 1103515245 + 12345) & 0x7FFFFFFF
        return self.s


def draw_sample(N, set_size, rand):
    """one iteration's draw: DUtils::Random::RandomInt(0, size - 1) on the shrinking index vector"""
    avail = list(range(N))
    out = []
    for _ in range(set_size):
        r = int((rand() / (RAND_MAX + 1.0)) * len(avail))
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def make_case(name, N, set_size, seed, noise=0.0, wrong=0, K=K_KITTI, planar_first=0, zmin=4.0, zmax=200.0):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.05, 0.5)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(ang) * S + (1 - math.cos(ang)) * S @ S
    t = rng.uniform(-1, 1, 3)
    fx, fy, cx, cy = K
    z = rng.uniform(zmin, zmax, N)
    pc = np.stack([rng.uniform(-0.4, 0.4, N) * z, rng.uniform(-0.2, 0.2, N) * z, z], 1)
    pw = (pc - t) @ R
    if planar_first:                       # the first points lie in the world plane z = 0, exactly, in float32 too
        pw[:planar_first, 2] = 0.0
        t = t + np.array([0.0, 0.0, 30.0])
        pc = pw @ R.T + t
    p3d = pw.astype(np.float32)
    pc = p3d.astype(np.float64) @ R.T + t
    u = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1) + rng.normal(size=(N, 2)) * noise
    if wrong:
        u[:wrong] += rng.uniform(30, 80, (wrong, 2)) * rng.choice([-1, 1], (wrong, 2))
    sigma2 = SIGMA2[rng.integers(0, 8, N)]
    lcg = Lcg(seed)
    samples = np.array([draw_sample(N, set_size, lcg) for _ in range(9)], np.int32).reshape(-1, set_size)
    return dict(name=name, N=N, set_size=set_size, seed=seed, K=tuple(np.float32(v) for v in K), R=R, t=t, p2d=u.astype(np.float32),
                p3d=p3d, sigma2=sigma2, samples=samples, wrong=wrong)


SIZES = (4, 5, 31, 32, 33, 63, 64, 65, 130)
SET_SIZES = (4, 5, 6, 8)
HYP_COUNTS = (1, 3, 4, 5, 9)             # around the 4-waves-per-workgroup edge
CASES = []
for _N in SIZES:
    for _k, _s in enumerate(SET_SIZES):
        if _s <= _N:
            _noisy = (_N + _k) % 2 == 1
            CASES.append(make_case("n%d_s%d" % (_N, _s), _N, _s, 1000 + 10 * _N + _s,
                                   noise=0.6 if _noisy else 0.0, wrong=_N // 3 if _N >= 31 else 0,
                                   K=(K_KITTI, K_TUM, K_EUROC)[(_N + _k) % 3]))
# the sample {0, 1, 2, 3} of this case is coplanar in the world (z = 0 exactly): estimate_R_and_t's rank-deficient branch
COPLANAR = make_case("n33_s4_coplanar", 33, 4, 77, planar_first=8, zmin=20.0, zmax=40.0)
COPLANAR["samples"] = np.concatenate([np.array([[0, 1, 2, 3], [4, 5, 6, 7], [0, 2, 5, 7]], np.int32), COPLANAR["samples"][:2]])
CASES.append(COPLANAR)
BY_NAME = {c["name"]: c for c in CASES}

# the mixed batch: (case name, hypotheses): different N, set_size and calibration, one problem in the middle without hypotheses
MIXED = (("n130_s4", 9), ("n33_s8", 3), ("n64_s5", 0), ("n5_s5", 4), ("n65_s6", 5))

# for the comparison with oracle/pose_oracle.py: the scenes tests/test_pose.py::test_epnp_equals_oracle holds 1e-8 on (generic points
# at 4 to 20 m, no wrong matches, exact or 0.6 px noise), sampled 6 and 8 at a time
ORACLE = {"n%d_s%d" % (N, s): make_case("oracle_n%d_s%d" % (N, s), N, s, 500 + N + s, noise=0.6 if (N + s) % 4 == 0 else 0.0, zmax=20.0)
          for N in (31, 64, 130) for s in (6, 8)}

# RANSAC scenes (N, wrong, set_size, min_inliers, seed) for the draw / attach / iterate comparisons
RANSAC = {
    "early": (60, 20, 4, 10, 31),          # a pose comes back in the middle of the first queue
    "never": (50, 20, 4, 45, 32),          # min_inliers no hypothesis reaches: every iteration runs
    "set6": (90, 36, 6, 10, 33),
    "late": (150, 75, 4, 60, 34),
}


def ransac_case(key):
    N, wrong, set_size, min_inliers, seed = RANSAC[key]
    c = make_case(key, N, set_size, seed, noise=0.5, wrong=wrong, zmin=4.0, zmax=40.0)
    c["params"] = (0.99, min_inliers, 300, set_size, 0.5, 5.991)
    return c
