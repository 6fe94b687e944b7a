"""Deterministic monocular-Initializer cases shared by test_initializer_cpu.py, test_initializer_gpu.py and the C++ call-site test.

A case: two views of N matched points with a planted motion X2 = R X1 + t (camera K), EXTRA unmatched keys in either frame (so
that Normalize, which runs over ALL keys, differs from a normalisation of the matched ones), the keys of both frames shuffled,
0.25 px of Gaussian noise on every key, and for N >= 128 a fifth of the matches wrong (the second key moved at least 60 px).
Scenes: "plane" (points on a tilted plane: the homography route), "general" (points in a volume: the fundamental route),
"rotation" (the general scene with t = 0: must be refused), "few" (general, N = 63 with 20 wrong matches: too few inliers for
minTriangulated = 50).  The sets of a case are the 200 draws of Initialize (:82-97) from a scripted source.

The expected answers are unambiguous because (checked at import with the fp64 oracle, check_conditions()):
  * for every drawn set without a wrong match whose 8-point system is well conditioned (COND_FLOOR; model H on plane / rotation,
    model F on general / few), no match's chi-square lies within relative MARGIN of its threshold;
  * RH is at least RH_MARGIN away from 0.40, and where CheckRT is reached the verdict does not hang on a margin: either every
    comparison of the 0.7 * maxGood / 0.75 * bestGood / 0.9 * N / minTriangulated / minParallax rules accepts with COUNT_MARGIN
    (PARALLAX_MARGIN degrees) to spare, or one of them refuses by as much (decisions());
  * the oracle accepts plane and general from N = 63 on and refuses rotation, few and every N < 63."""
import numpy as np

import initializer_oracle as O

SIGMA = 1.0
ITERATIONS = 200
SIZES = (8, 9, 63, 64, 65, 128, 129, 300)
HYP_COUNTS = (0, 1, 5, 200)                  # iteration counts: a run of k iterations uses the first k sets
RAND_MAX = 2 ** 31 - 1
K = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
NOISE_PX = 0.25
MARGIN = 1e-3                   # relative distance of a chi-square from its threshold
RH_MARGIN = 0.05
COUNT_MARGIN = 1.5
PARALLAX_MARGIN = 0.2
# a set is compared value by value only where the 8-point system is well conditioned: sigma_8 / sigma_1 of its matrix (the
# second-smallest singular value over the largest, fp64 oracle) is above this; below it the float32 solve loses more than the tolerance
COND_FLOOR = 2e-3
# The host path's largest deviations, measured by test_initializer_cpu.py (each test prints its figure).  The first two are against
# the fp64 oracle (1.548e-6, 1.395e-4).  The last three are against the PLANTED scene (1.144e-2, 5.326e-2, 1.655e-1, all on the plane
# scenes): they are the error of a motion taken from one minimal set of 8 matches with NOISE_PX of noise, decomposed without any
# refinement, as the reference does; the float arithmetic is a small part of them.
NORM_MEASURED = 1.6e-6          # Normalize: max |a - b| / max(1, |b|) over points and T
NORM_TOL = 4 * NORM_MEASURED
MATRIX_MEASURED = 1.4e-4        # H21i / F21i of well-conditioned all-inlier sets, unit Frobenius norm, sign aligned: max |a - b|
MATRIX_TOL = 4 * MATRIX_MEASURED
ROT_MEASURED = 1.2e-2           # Initialize against the planted motion: max |R - R_planted|
ROT_TOL = 4 * ROT_MEASURED
DIR_MEASURED = 5.4e-2           # ... max |t - t_planted / |t_planted||
DIR_TOL = 4 * DIR_MEASURED
STRUCT_MEASURED = 1.7e-1        # ... max over triangulated points of |X |t_planted| - X_planted| / depth
STRUCT_TOL = 4 * STRUCT_MEASURED
assert NORM_TOL < 1e-5 and MATRIX_TOL < 1e-3 and ROT_TOL < 0.1 and DIR_TOL < 0.25 and STRUCT_TOL < 0.75


class Lcg:
    """The scripted uniform source: a 31-bit linear congruential generator, values in [0, RAND_MAX]"""

    def __init__(self, seed):
        self.state = (seed * 2654435761 + 12345) % (2 ** 31)

    def __call__(self):
        self.state = (1103515245 * self.state + 12345) % (2 ** 31)
        return self.state


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(a, a) + np.sin(th) * ax


def _project(X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def make_case(scene, N, seed):
    rng = np.random.default_rng(seed)
    extra = N // 4 + 3
    n1 = n2 = N + extra
    x, y = rng.uniform(-3, 3, n1), rng.uniform(-2, 2, n1)
    z = 6 + 0.25 * x - 0.15 * y if scene in ("plane",) else rng.uniform(4, 10, n1)
    X1 = np.stack([x, y, z], 1)
    R = _rot(rng.normal(size=3) + np.array([0, 3.0, 0]), rng.uniform(3, 8))
    t = np.array([-rng.uniform(0.5, 0.8), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
    if scene == "rotation":
        t = np.zeros(3)
    X2 = X1 @ R.T + t
    k1 = _project(X1) + rng.normal(0, NOISE_PX, (n1, 2))
    k2 = _project(X2) + rng.normal(0, NOISE_PX, (n1, 2))
    n_out = 20 if scene == "few" else (N // 5 if N >= 128 else 0)
    wrong = np.zeros(n1, bool)
    wrong[rng.permutation(N)[:n_out]] = True            # among the first N points: the matched ones
    ang, px = rng.uniform(0, 2 * np.pi, n1), rng.uniform(60, 200, n1)
    k2 = np.where(wrong[:, None], k2 + np.stack([px * np.cos(ang), px * np.sin(ang)], 1), k2)
    # points 0..N-1 are matched, the others are keys without a match; both frames are shuffled
    p1, p2 = rng.permutation(n1), rng.permutation(n2)   # point j is key p1[j] of frame 1 and key p2[j] of frame 2
    keys1, keys2 = np.zeros((n1, 2), np.float32), np.zeros((n2, 2), np.float32)
    keys1[p1], keys2[p2] = k1.astype(np.float32), k2.astype(np.float32)
    matches12 = np.full(n1, -1, np.int32)
    matches12[p1[:N]] = p2[:N]
    point_of_key1 = np.zeros(n1, np.int64)
    point_of_key1[p1] = np.arange(n1)
    first, second = O.matches_of(matches12)
    pts = point_of_key1[first]                           # the 3D point of every match, in match order
    sets = O.draw_sets(N, ITERATIONS, Lcg(seed), RAND_MAX)
    return dict(name="%s%d" % (scene, N), scene=scene, N=N, seed=seed, n1=n1, n2=n2, keys1=keys1, keys2=keys2, matches12=matches12,
                first=first, second=second, R=R, t=t, X1=X1[pts], wrong=wrong[pts], sets=sets, point_of_key1=point_of_key1, X1_all=X1,
                model=O.MODEL_H if scene in ("plane", "rotation") else O.MODEL_F)


def problem_arrays(case):
    """(uv [N, 4], pn [N, 4], T1, T2) of the case in float64, from the oracle's Normalize"""
    k1, k2 = case["keys1"].astype(np.float64), case["keys2"].astype(np.float64)
    pn1, T1 = O.normalize(k1)
    pn2, T2 = O.normalize(k2)
    f, s = case["first"], case["second"]
    return np.hstack([k1[f], k2[s]]), np.hstack([pn1[f], pn2[s]]), T1, T2


def pure_sets(case):
    """indices of the drawn sets without a wrong match"""
    return [k for k, st in enumerate(case["sets"]) if not case["wrong"][st].any()]


def conditioning(case, model, set8):
    """sigma_8 / sigma_1 of ComputeH21's / ComputeF21's matrix on the set (fp64)"""
    _, pn, _, _ = problem_arrays(case)
    q = pn[np.asarray(set8)]
    if model == O.MODEL_H:
        A = []
        for u1, v1, u2, v2 in q:
            A.append([0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2])
            A.append([u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2])
    else:
        A = [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1] for u1, v1, u2, v2 in q]
    w = np.linalg.svd(np.array(A), compute_uv=False)
    return float(w[7] / w[0])


def oracle_matrices(case):
    """{set index: fp64 H21i / F21i} of the pure sets of the case's own model, computed once"""
    if "oracle_M" not in case:
        uv, pn, T1, T2 = problem_arrays(case)
        case["oracle_M"] = {k: O.hypothesis_matrix(case["model"], pn, T1, T2, case["sets"][k]) for k in pure_sets(case)}
    return case["oracle_M"]


def oracle_initialize(case):
    if "oracle_init" not in case:
        case["oracle_init"] = O.initialize(case["keys1"], case["keys2"], case["matches12"], K, SIGMA, case["sets"])
    return case["oracle_init"]


def expect_ok(case):
    return case["scene"] in ("plane", "general") and case["N"] >= 63


def decisions(r):
    """The comparisons that decide ReconstructF (:504-525) / ReconstructH (:721) for the oracle's result r, each as (value, bound,
    margin) with `value > bound` the accepting side"""
    counts, N = r["counts"], r["N"]
    if r["model"] == O.MODEL_F:
        mx = max(counts)
        k = counts.index(mx)
        d = [(mx, max(int(0.9 * N), 50) - 0.5, COUNT_MARGIN), (r["parallax"][k], 1.0, PARALLAX_MARGIN)]
        d += [(0.7 * mx, c, COUNT_MARGIN) for i, c in enumerate(counts) if i != k]        # nsimilar stays 1
        return d
    bg = max(counts)
    return [(0.75 * bg, r["second"], COUNT_MARGIN), (r["parallax"][counts.index(bg)], 1.0, PARALLAX_MARGIN), (bg, 50, COUNT_MARGIN),
            (bg, 0.9 * N, COUNT_MARGIN)]


def well_conditioned_pure_sets(case):
    if "wc_sets" not in case:
        case["wc_sets"] = [k for k in pure_sets(case) if conditioning(case, case["model"], case["sets"][k]) >= COND_FLOOR]
    return case["wc_sets"]


def check_conditions(case):
    """The conditions of the module docstring; returns the first violated one as a string, or None"""
    uv, pn, T1, T2 = problem_arrays(case)
    model = case["model"]
    th = O.TH_H if model == O.MODEL_H else O.TH_F
    M = oracle_matrices(case)
    for k in well_conditioned_pure_sets(case):
        for c in O.chi_squares(model, M[k], uv, SIGMA):
            if (np.abs(c - th) <= MARGIN * th).any():
                return "set %d: a chi-square within %g of its threshold" % (k, MARGIN)
    r = oracle_initialize(case)
    if r["ok"] != expect_ok(case):
        return "the oracle %s the case" % ("accepts" if r["ok"] else "refuses")
    if abs(r["RH"] - 0.40) < RH_MARGIN:
        return "RH = %.3f" % r["RH"]
    if (r["RH"] > 0.40) != (model == O.MODEL_H):
        return "RH = %.3f takes the other route" % r["RH"]
    if r["counts"]:
        d = decisions(r)
        accepted = all(v - b > m for v, b, m in d)
        refused = any(b - v > m for v, b, m in d)
        if not (accepted or refused):
            return "a CheckRT count or the parallax near a rule: %s of %d, parallax %s" % (r["counts"], r["N"], np.round(r["parallax"], 2))
    return None


def find_seed(scene, N, start):
    """the first seed from `start` on for which check_conditions() holds (how SEEDS was filled)"""
    for seed in range(start, start + 200):
        if check_conditions(make_case(scene, N, seed)) is None:
            return seed
    raise RuntimeError("no seed for %s %d" % (scene, N))


# seeds for which check_conditions() holds (found with find_seed, asserted below)
SEEDS = {("plane", 8): 1000, ("plane", 9): 1001, ("plane", 63): 1017, ("plane", 64): 1021, ("plane", 65): 1023, ("plane", 128): 1027,
         ("plane", 129): 1029, ("plane", 300): 1045, ("general", 8): 1046, ("general", 9): 1047, ("general", 63): 1075,
         ("general", 64): 1083, ("general", 65): 1122, ("general", 128): 1128, ("general", 129): 1131, ("general", 300): 1136,
         ("rotation", 129): 1137, ("few", 63): 1138}
SCENES = [(scene, N) for scene in ("plane", "general") for N in SIZES] + [("rotation", 129), ("few", 63)]
CASES = [make_case(scene, N, SEEDS[(scene, N)]) for scene, N in SCENES]
BY_NAME = {c["name"]: c for c in CASES}
for _c in CASES:
    _bad = check_conditions(_c)
    assert _bad is None, (_c["name"], _c["seed"], _bad)

# the mixed batch: (case name, iterations) -- every size class, every iteration count, both routes, and problems without
# hypotheses in the middle.  A problem of k iterations has 2 k hypotheses: the H of the first k sets, then their F
MIXED = (("general300", 200), ("plane8", 5), ("plane64", 0), ("general65", 1), ("plane129", 200), ("general9", 5), ("rotation129", 1),
         ("general128", 0), ("plane63", 5), ("few63", 200))
