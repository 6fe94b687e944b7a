"""Deterministic Sim3Solver cases shared by test_sim3_cpu.py and test_sim3_gpu.py.

A case: a planted similarity (scale in 0.5..2; its fix-scale twin has scale 1), two different cameras, points at 2-20 m in front
of camera 2 (camera 1 sees them at scale times that), keypoint octaves 0..7 on both sides so that the thresholds differ.  Planted
inliers carry no noise beyond the float32 rounding of their coordinates; planted outliers are moved 200-500 px in image 1.  The
triples of a case are the first 300 draws of Sim3Solver::iterate (:163-177) from a scripted source.

The expected answers are hand-derivable because (checked at import with the fp64 oracle, no exclusions):
  * a triple of three planted inliers has exactly the planted inliers as its inliers;
  * a triple that contains an outlier gathers at most MIN_INLIERS - 3 inliers;
  * every triple's triangle has its smallest altitude above ALTITUDE_FLOOR metres (both cameras);
  * no correspondence's err1 / err2 lies within relative MARGIN of its threshold for any triple of the case."""
import numpy as np

import sim3_oracle as O

MIN_INLIERS = 20                 # LoopClosing.cc:276 SetRansacParameters(0.99, 20, 300)
MAX_ITERATIONS = 300
PROBABILITY = 0.99
ALTITUDE_FLOOR = 0.3            # metres: below it the float32 Horn solve loses more than SRT_TOL to conditioning
MARGIN = 1e-3
SIZES = (0, 2, 3, 19, 20, 21, 63, 64, 65, 128, 129, 300)
HYP_COUNTS = (0, 1, 5, 300)
RAND_MAX = 2 ** 31 - 1
K1 = np.array([525.0, 530.0, 319.5, 239.5], np.float32)
K2 = np.array([718.856, 716.3, 607.19, 185.2], np.float32)
# the host path's largest deviation from the fp64 oracle over every triple of every case, measured by
# test_sim3_cpu.py::test_hypothesis_values_against_oracle (it prints the figure): max over s, R, t of |a - b| / max(1, |b|)
SRT_MEASURED = 2.0e-4           # 1.997e-4, on n20_fix: a thin triangle (altitude 0.3-0.5 m at 10 m) in float32, as the reference's types are
SRT_TOL = 4 * SRT_MEASURED
assert SRT_TOL < 1e-3


class Lcg:
    """The scripted uniform source: a 31-bit linear congruential generator, values in [0, RAND_MAX]"""

    def __init__(self, seed):
        self.state = (seed * 2654435761 + 12345) % (2 ** 31)

    def __call__(self):
        self.state = (1103515245 * self.state + 12345) % (2 ** 31)
        return self.state


def _rotation(rng, max_deg):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return O.rodrigues(axis * np.deg2rad(rng.uniform(5, max_deg)))


def make_case(N, seed, fix_scale):
    rng = np.random.default_rng(seed)
    s = 1.0 if fix_scale else float(rng.uniform(0.5, 2.0))
    R, t = _rotation(rng, 20), rng.uniform(-0.3, 0.3, 3)
    z = rng.uniform(2 * max(1, 1 / s), 20 * min(1, 1 / s), N)
    u, v = rng.uniform(60, 1180, N), rng.uniform(30, 340, N)
    x2 = np.stack([(u - K2[2]) / K2[0] * z, (v - K2[3]) / K2[1] * z, z], 1)
    x1 = s * (x2 @ R.T) + t
    n_out = N // 4 if N >= 63 else 0
    outlier = np.zeros(N, bool)
    outlier[rng.permutation(N)[:n_out]] = True
    ang, px = rng.uniform(0, 2 * np.pi, N), rng.uniform(200, 500, N)
    shift = np.stack([px * np.cos(ang) / K1[0], px * np.sin(ang) / K1[1], np.zeros(N)], 1) * x1[:, 2:3]
    x1 = np.where(outlier[:, None], x1 + shift, x1)
    oct1, oct2 = rng.integers(0, 8, N), rng.integers(0, 8, N)
    sig = np.float32(1.2) ** (2 * np.arange(8, dtype=np.float32))
    lcg = Lcg(seed)
    triples = np.array([O.draw_triple(N, lcg, RAND_MAX) for _ in range(MAX_ITERATIONS)], np.int32).reshape(-1, 3) if N >= 3 \
        else np.zeros((0, 3), np.int32)
    return dict(name="n%d_%s" % (N, "fix" if fix_scale else "free"), N=N, seed=seed, fix=fix_scale, s=s, R=R, t=t,
                x1=x1.astype(np.float32), x2=x2.astype(np.float32), sigma2_1=sig[oct1].astype(np.float32),
                sigma2_2=sig[oct2].astype(np.float32), K1=K1, K2=K2, outlier=outlier, triples=triples)


def min_altitude(case):
    """the smallest altitude of any triple's triangle, in either camera"""
    best = np.inf
    for x in (case["x1"].astype(np.float64), case["x2"].astype(np.float64)):
        a, b, c = (x[case["triples"][:, k]] for k in range(3))
        sides = np.max([np.linalg.norm(b - c, axis=1), np.linalg.norm(a - c, axis=1), np.linalg.norm(a - b, axis=1)], 0)
        if len(sides):
            best = min(best, float((np.linalg.norm(np.cross(b - a, c - a), axis=1) / sides).min()))
    return best


def oracle_results(case):
    """fp64 (s, R, t, flags) of every triple of the case, computed once"""
    if "oracle" not in case:
        e1 = np.array([O.max_error(v) for v in case["sigma2_1"]])
        e2 = np.array([O.max_error(v) for v in case["sigma2_2"]])
        x1, x2 = case["x1"].astype(np.float64), case["x2"].astype(np.float64)
        res = []
        for tri in case["triples"]:
            s, R, t = O.compute_sim3(x1[tri], x2[tri], case["fix"])
            err1, err2 = O.errors(s, R, t, x1, x2, case["K1"], case["K2"])
            res.append((s, R, t, (err1 < e1) & (err2 < e2), err1, err2))
        case["oracle"], case["e1"], case["e2"] = res, e1, e2
    return case["oracle"]


def check_conditions(case):
    """The conditions of the module docstring; returns the first violated one as a string, or None"""
    if min_altitude(case) <= ALTITUDE_FLOOR:
        return "a triple is near-degenerate"
    res = oracle_results(case)
    inl = ~case["outlier"]
    for k, tri in enumerate(case["triples"]):
        s, R, t, flags, err1, err2 = res[k]
        if case["outlier"][tri].any():
            if flags.sum() > MIN_INLIERS - 3:
                return "contaminated triple %d gathers %d inliers" % (k, flags.sum())
        elif not np.array_equal(flags, inl):
            return "pure triple %d does not give the planted inliers" % k
        for err, e in ((err1, case["e1"]), (err2, case["e2"])):
            if (np.abs(err - e) <= MARGIN * e).any():
                return "triple %d: an error within %g of its threshold" % (k, MARGIN)
    return None


# seeds for which check_conditions() holds with no exclusions (asserted below and in test_sim3_cpu.py)
SEEDS = {(0, False): 100, (0, True): 101, (2, False): 102, (2, True): 103, (3, False): 104, (3, True): 105, (19, False): 121,
         (19, True): 130, (20, False): 135, (20, True): 137, (21, False): 141, (21, True): 150, (63, False): 202, (63, True): 214,
         (64, False): 348, (64, True): 355, (65, False): 434, (65, True): 440, (128, False): 490, (128, True): 507,
         (129, False): 544, (129, True): 595, (300, False): 926, (300, True): 1004}
CASES = [make_case(N, SEEDS[(N, fix)], fix) for N in SIZES for fix in (False, True)]
BY_NAME = {c["name"]: c for c in CASES}
for _c in CASES:
    _bad = check_conditions(_c)
    assert _bad is None, (_c["name"], _c["seed"], _bad)

# the mixed batch: (case name, hypotheses) -- every size class, every hypothesis count, a problem without correspondences and one
# without hypotheses in the middle
MIXED = (("n300_free", 300), ("n0_free", 0), ("n3_fix", 5), ("n65_free", 1), ("n64_fix", 300), ("n21_free", 0), ("n129_fix", 5),
         ("n63_free", 300), ("n20_fix", 1), ("n128_free", 5))
