"""The OptimizeEssentialGraph cases the tests share (tests/test_eg_cpu.py, tests/test_eg_gpu.py, tests/tools/measure_eg_spread.py).
A problem is the dict of my_slam_amd.pack_eg_problem; a case is (problem, n_iterations).

graph() builds what LoopClosing::CorrectLoop hands over: key frames along a drifted trajectory (Snc, scale 1), of which those from
`corrected_from` on were moved by one Sim3 D (Scw = Snc * D: the correction of the current key frame's neighbourhood), the edges in
the reference's insertion order (src/Optimizer.cc:852-983): the LoopConnections edges (measured from Scw on both ends), then per key
frame its spanning-tree edge to the key frame before it, its old loop edges and its covisibility edges inside a band (measured
from Snc).  The errors a call starts from sit on the edges that cross the correction boundary, where C * Si * Sj^-1 is D
conjugated: D's angle and scale choose the branch of Sim3::log there.

The shapes are the smallest at which each piece can go wrong: 2 key frames; 6 and 7 free ones (42 and 49 unknowns, either side of
the solve's 48-column panel); 14 with a loop; 30 as a chain plus a band plus long loop rows (the envelope); the fixed key frame
first, in the middle, last and absent; two and three edges on a pair; a key frame without edges; the fixed key frame in both roles;
fix_scale; the four branches of Sim3::log and a consistent graph; budgets 0, 1, 2, 3 and 20; a rejected trial; 0, 1, 63, 64 and 65
points with ref = -1 and ref = the fixed key frame among them.  SCALE_SPECS, further down, holds the four graphs at which the GPU
path's launches take more than one workgroup: a group of its own with bars of its own.

Counts: after convergence accept / reject is decided by noise.  Iteration and trial counts are compared exactly on the cases whose
every oracle decision (tests/eg_oracle.py: rho against 0, the _nBad quantity against 0) stays at least MARGIN_FACTOR x its own
spread over the oracle's six variants away from 0; the others are named in CONVERGED and compare estimates and chi2 only.
tests/tools/measure_eg_spread.py computes that list and tests/test_eg_cpu.py holds CONVERGED to it; at most a third of the cases
may be in it.  GAUGE cases (no fixed key frame) compare counts (unless CONVERGED) and chi2 only, and of chi2 what is comparable: H
is singular up to lambda = 1e-16, the step along the seven gauge directions is rounding noise divided by 1e-16, and the oracle's own
six variants end between 4e-5 and 6e-3 after two iterations.  So the initial chi2 is held to its bar and the final one to what
Levenberg guarantees: finite and not above the initial one.

oracle(name, order, nudge) and host(ms, name) compute each result once and keep it; nobody may change them."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eg_oracle as eo  # noqa: E402

MARGIN_FACTOR = 1000
FLOAT_ULP = 2.0 ** -23
KEYS = ("rotation", "translation", "scale", "point", "chi2_final_relative", "chi2_initial_relative")
VARIANTS = tuple((order, nudge) for order in ("forward", "reverse") for nudge in (0, 1, -1))
TOLERANCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eg", "tolerance.json")


def rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def sim3(R, t, s):
    """g2o::Sim3(R, t, s) in operator[] order"""
    return np.concatenate([eo.quat_from_R(np.asarray(R, np.float64)), np.asarray(t, np.float64), [float(s)]])


def graph(seed, n, fixed, corrected_from, D=(0.3, 1.1, 2.0), band=0, loop_connections=(), old_loops=(), extra=(), fix_scale=False,
          n_points=0, isolated=False, snc_differs=True):
    """D = (angle, scale, |translation|) of the correction.  loop_connections / old_loops / extra: (i, j) pairs, vertex 0 first;
    extra edges follow a key frame's own like covisibility edges do.  isolated: one more key frame without edges in the middle."""
    rng = np.random.default_rng(seed)
    Snc = np.zeros((n, 8))
    for k in range(n):                          # a camera moving along x, looking around a little: Tcw
        R = rot(rng.normal(0, 0.15, 3) + np.array([0, 0.05 * k, 0]))
        Snc[k] = sim3(R, -R @ (np.array([0.4 * k, 0.0, 0.0]) + rng.normal(0, 0.05, 3)), 1.0)
    axis = rng.normal(0, 1, 3)
    Dm = sim3(rot(D[0] * axis / np.linalg.norm(axis)), D[2] * np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74]), D[1])
    Scw = Snc.copy()
    for k in range(corrected_from, n):
        Scw[k] = eo.mul(Snc[k], Dm)
    if fix_scale:                               # CorrectLoop under mbFixScale carries scale 1
        assert D[1] == 1.0
    edges = [(i, j, 1) for i, j in loop_connections]
    for i in range(n):
        if i > 0:
            edges.append((i, i - 1, 0))
        edges += [(a, b, 0) for a, b in old_loops if a == i]
        edges += [(i, j, 0) for j in range(max(i - band, 0), i - 1)]
        edges += [(a, b, 0) for a, b in extra if a == i]
    ei, ej, ec = (np.array([e[k] for e in edges], dt) for k, dt in ((0, np.int32), (1, np.int32), (2, np.uint8)))
    if isolated:                                # insert a key frame without edges at n // 2
        at = n // 2
        lone = sim3(rot(np.array([0.02, -0.03, 0.01])), (0.3, -0.1, 0.2), 1.0)
        Snc, Scw = np.insert(Snc, at, lone, 0), np.insert(Scw, at, lone, 0)
        ei, ej = np.where(ei >= at, ei + 1, ei).astype(np.int32), np.where(ej >= at, ej + 1, ej).astype(np.int32)
        fixed = fixed + 1 if fixed >= at else fixed
        n += 1
    pr = {"Scw": Scw, "Snc": Snc if snc_differs else None, "fixed": fixed, "fix_scale": fix_scale, "edge_i": ei, "edge_j": ej,
          "edge_corrected": ec, "xw": np.zeros((0, 3), np.float32), "ref": np.zeros(0, np.int32)}
    if isolated:
        pr["isolated"] = n // 2
    if n_points:
        pr["xw"] = rng.normal(0, 3, (n_points, 3)).astype(np.float32)
        ref = rng.integers(0, n, n_points).astype(np.int32)
        ref[0] = -1                             # keeps its bits
        if n_points > 1 and fixed >= 0:
            ref[-1] = fixed                     # Srw and correctedSwr are inverses of each other up to rounding
        pr["ref"] = ref
    return pr


_BUDGET = dict(seed=70, n=10, fixed=2, corrected_from=6, band=3, loop_connections=((9, 2),))
SPECS = {
    # name: (graph arguments, n_iterations)
    "kf2_one_edge": (dict(seed=10, n=2, fixed=0, corrected_from=1), 1),
    "free6": (dict(seed=20, n=7, fixed=0, corrected_from=4, band=2, loop_connections=((6, 0),), n_points=63), 3),
    "free7": (dict(seed=30, n=8, fixed=0, corrected_from=5, band=2, loop_connections=((7, 0),), n_points=64), 3),
    "free14_loop": (dict(seed=40, n=15, fixed=1, corrected_from=10, band=3, loop_connections=((14, 1), (13, 1), (14, 2)), n_points=65), 3),
    "chain30": (dict(seed=50, n=30, fixed=3, corrected_from=24, band=3, loop_connections=((29, 3), (28, 4)), old_loops=((17, 5),), n_points=1), 20),
    "chain30_budget3": (dict(seed=50, n=30, fixed=3, corrected_from=24, band=3, loop_connections=((29, 3), (28, 4)), old_loops=((17, 5),)), 3),
    "fixed_first": (dict(seed=60, n=10, fixed=0, corrected_from=6, band=2, loop_connections=((9, 0),)), 3),
    "fixed_middle": (dict(seed=61, n=10, fixed=5, corrected_from=7, band=2, loop_connections=((9, 5),)), 2),
    "fixed_last": (dict(seed=62, n=10, fixed=9, corrected_from=4, band=2, loop_connections=((9, 1),)), 3),
    "no_fixed": (dict(seed=63, n=6, fixed=-1, corrected_from=3, band=2), 2),
    "pair_two_edges": (dict(seed=64, n=8, fixed=0, corrected_from=5, old_loops=((5, 4),), loop_connections=((7, 0),)), 3),
    "pair_three_edges": (dict(seed=65, n=8, fixed=0, corrected_from=5, old_loops=((5, 4),), extra=((5, 4),), loop_connections=((7, 0),)), 3),
    "isolated_kf": (dict(seed=66, n=8, fixed=0, corrected_from=5, band=2, loop_connections=((7, 0),), isolated=True), 3),
    "fixed_both_roles": (dict(seed=67, n=8, fixed=3, corrected_from=5, band=2, loop_connections=((7, 3), (3, 6))), 3),
    "fix_scale": (dict(seed=68, n=9, fixed=0, corrected_from=5, D=(0.3, 1.0, 2.0), band=2, loop_connections=((8, 0),), fix_scale=True, n_points=5), 3),
    "log_small_angle_unit_scale": (dict(seed=71, n=8, fixed=0, corrected_from=5, D=(1e-3, 1.0, 0.5), band=2, loop_connections=((7, 0),)), 2),
    "log_small_angle_scaled": (dict(seed=72, n=8, fixed=0, corrected_from=5, D=(1e-3, 1.1, 0.5), band=2, loop_connections=((7, 0),)), 2),
    "log_angle_unit_scale": (dict(seed=73, n=8, fixed=0, corrected_from=5, D=(0.3, 1.0, 2.0), band=2, loop_connections=((7, 0),)), 2),
    "log_angle_scaled": (dict(seed=74, n=8, fixed=0, corrected_from=5, D=(0.3, 1.1, 2.0), band=2, loop_connections=((7, 0),)), 2),
    "consistent": (dict(seed=75, n=8, fixed=0, corrected_from=8, band=2, loop_connections=((7, 0),), snc_differs=False), 3),
    "budget_0": (_BUDGET, 0),
    "budget_1": (_BUDGET, 1),
    "budget_2": (_BUDGET, 2),
    "budget_3": (_BUDGET, 3),
    "budget_20": (_BUDGET, 20),
    # a correction of almost half a turn and 30 units: the fourth Gauss-Newton step overshoots, nine trials are rejected with rho
    # well below 0 until lambda has grown from 1e-17 to 0.4, the tenth is accepted, and ten trials end the loop
    "rejected_trial": (dict(seed=316, n=12, fixed=0, corrected_from=3, D=(3.1, 1.0, 30.0), band=3, loop_connections=((11, 0),)), 6),
}
NAMES = tuple(SPECS)
GAUGE = ("no_fixed",)
# chi2 goes to about 0 (a consistent graph; one edge and one free vertex, which a step solves up to the Jacobian's noise): the
# final chi2 is compared absolutely, against the bar measured as the others are, and `consistent` against absolute_chi2_bar as well
ABSOLUTE_CHI2 = ("consistent", "kf2_one_edge")
# Errors near half a turn, where acos' derivative has no bound, and a lambda that climbs 16 orders of magnitude: the oracle's six
# variants of this case lie a thousand times further apart than those of any other.  It has bars of its own, made the same way, so
# that it does not widen everybody's.
ILL_CONDITIONED = ("rejected_trial",)
# the cases whose counts are decided by noise (see the module text); tests/tools/measure_eg_spread.py computes the list
CONVERGED = ("chain30", "no_fixed", "consistent", "budget_20")
# (|sigma| < eps, d > 1 - eps) that the case's boundary edges must start in
BRANCH_OF = {"log_small_angle_unit_scale": (True, True), "log_small_angle_scaled": (False, True),
             "log_angle_unit_scale": (True, False), "log_angle_scaled": (False, False)}



def _scale(n, n_iterations, **more):
    """n key frames, the first fixed, as a chain plus a band of 10 plus a loop of 10 edges (the shape of tools/bench_eg.py)"""
    return (dict(seed=n, n=n, fixed=0, corrected_from=n - 10, band=10, loop_connections=tuple((n - 1 - k, k) for k in range(10)), **more),
            n_iterations)


# The scale cases: what only a launch over several workgroups reaches (N = 7 free key frames unknowns).  They are a group of their
# own: they take no part in the common spread, the CONVERGED list or the case count of tolerance.json, and each has bars of its
# own there under "scale", made as the common ones are (4 x the spread of the oracle's six variants on that case alone): the
# spread grows with the condition of the system, and a pooled bar would let the small cases hide behind the large ones.
# One iteration at the large sizes: a second one of such a graph runs into rejected trials decided by noise.  Every one of them
# must keep decisions_clear(), so its counts are compared exactly.
SCALE_SPECS = {
    "scale_kf43": _scale(43, 2),                      # N = 294: k_eg_stage's second column block, k_spd_backward's second workgroup
    "scale_kf78": _scale(78, 1),                      # N = 539: k_spd_backward's third workgroup
    # more than 256 key frames, 2555 edges and N = 1813: k_eg_update / k_eg_output / k_eg_measure / k_eg_errors beyond one
    # workgroup, k_eg_reduce_out's loop strides twice; 300 points over all key frames: k_eg_points beyond one workgroup
    "scale_kf260": _scale(260, 1, n_points=300),
    "scale_kf438": _scale(438, 1),                    # ORBM_EG_MAX_KFS, N = 3059
}
SCALE_NAMES = tuple(SCALE_SPECS)
AT_THE_CAP = "scale_kf438"

_CASES, _ORACLE, _HOST = {}, {}, {}


def case(name):
    """(problem, n_iterations)"""
    if name not in _CASES:
        args, n_it = SPECS[name] if name in SPECS else SCALE_SPECS[name]
        _CASES[name] = (graph(**args), n_it)
    return _CASES[name]


def oracle(name, order="forward", nudge=0):
    key = (name, order, nudge)
    if key not in _ORACLE:
        pr, n_it = case(name)
        r = eo.optimize_essential_graph(pr, n_it, order, nudge)
        for a in (r["Scw"], r["Tcw"], r["xw"]):
            a.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def host(ms, name):
    """(code, Tcw, xw, Scw, stats) of the host path orbp_optimize_essential_graph for case `name`, computed once"""
    if name not in _HOST:
        pr, n_it = case(name)
        res = ms.optimize_essential_graph(pr, n_it)
        for a in res[1:4]:
            a.setflags(write=False)
        _HOST[name] = res
    return _HOST[name]


def tcw_of(Scw):
    """[R | t / s] in double (src/Optimizer.cc:999-1009)"""
    Scw = np.asarray(Scw, np.float64).reshape(-1, 8)
    T = np.zeros((len(Scw), 4, 4))
    T[:, :3, :3] = eo.quat_to_R(Scw[:, :4])
    T[:, :3, 3] = Scw[:, 4:7] * (1.0 / Scw[:, 7:8])
    T[:, 3, 3] = 1.0
    return T


def diffs(Tcw, s, xw, chi_f, chi_i, Tcw2, s2, xw2, chi_f2, chi_i2):
    """the six quantities of KEYS between two results (Tcw [n, 4, 4], the scales, the points, both chi2)"""
    def mx(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max()) if a.size else 0.0

    def rel(a, b):
        return abs(a - b) / abs(b) if b != 0 else (0.0 if a == b else np.inf)
    Tcw, Tcw2 = np.asarray(Tcw, np.float64).reshape(-1, 4, 4), np.asarray(Tcw2, np.float64).reshape(-1, 4, 4)
    return (mx(Tcw[:, :3, :3], Tcw2[:, :3, :3]), mx(Tcw[:, :3, 3], Tcw2[:, :3, 3]), mx(s, s2), mx(xw, xw2), rel(chi_f, chi_f2), rel(chi_i, chi_i2))


def decisions_clear(name):
    """every decision of the oracle stays MARGIN_FACTOR x its spread over the six variants away from its boundary, and the six
    transcripts agree"""
    runs = [oracle(name, *v) for v in VARIANTS]
    base = runs[0]
    if any(r["transcript"] != base["transcript"] or len(r["decisions"]) != len(base["decisions"]) for r in runs):
        return False
    for k, (kind, value) in enumerate(base["decisions"]):
        values = np.array([r["decisions"][k][1] for r in runs])
        if not np.isfinite(values).all():
            if not (values == values[0]).all():
                return False
            continue
        if abs(value) < MARGIN_FACTOR * float(values.max() - values.min()):
            return False
    return True


def absolute_chi2_bar(pr):
    """A consistent graph's errors are roundings of zero: each of the 7 components of an edge's error comes out of fewer than 1000
    roundings (three Sim3 products, an inverse, toRotationMatrix, a 3 x 3 LU solve) of quantities no larger than the largest
    translation, so chi2 stays below 7 E (1000 eps scale)^2."""
    scale = max(1.0, float(np.abs(np.asarray(pr["Scw"])[:, 4:7]).max()))
    return 7 * len(pr["edge_i"]) * (1000 * np.finfo(np.float64).eps * scale) ** 2


def bars(name):
    tol = json.load(open(TOLERANCE))
    if name in SCALE_SPECS:
        return tol["scale"][name]["bar"]
    return tol["ill_conditioned"][name]["bar"] if name in ILL_CONDITIONED else tol["bar"]


def assert_same(name, got, want_Tcw, want_s, want_xw, want_stats, what, counts, float_sides):
    """got = (code, Tcw float32, xw float32, Scw float64, stats).  The double Scw within the bars of tests/golden/eg/tolerance.json;
    the float Tcw and xw within the bars plus half a float ulp of the largest magnitude compared for each side that was rounded to
    float (float_sides); counts exactly where `counts`; chi2_initial at its own bar; a GAUGE case on counts and chi2 alone; an
    ABSOLUTE_CHI2 case's final chi2 absolutely."""
    code, Tcw, xw, Scw, stats = got
    pr = case(name)[0]
    bar = bars(name)
    assert code == 0, what
    if counts:
        for k in ("iterations", "trials"):
            assert stats[k] == want_stats[k], "%s: %s %s != %s" % (what, k, stats[k], want_stats[k])
    want_Tcw = np.asarray(want_Tcw, np.float64)
    d_double = diffs(tcw_of(Scw), Scw[:, 7], want_xw, stats["chi2_final"], stats["chi2_initial"], want_Tcw, want_s, want_xw,
                     want_stats["chi2_final"], want_stats["chi2_initial"])
    d_float = diffs(Tcw, Scw[:, 7], xw, 0, 0, want_Tcw, want_s, want_xw, 0, 0)
    t_scale = float(np.abs(want_Tcw[:, :3, 3]).max()) if len(want_Tcw) else 0.0
    x_scale = float(np.abs(want_xw).max()) if len(want_xw) else 0.0
    checks = []
    if name not in GAUGE:
        checks += [("rotation", d_double[0], bar["rotation"]), ("translation", d_double[1], bar["translation"]),
                   ("scale", d_double[2], bar["scale"]),
                   ("rotation (float)", d_float[0], bar["rotation"] + float_sides * 0.5 * FLOAT_ULP),
                   ("translation (float)", d_float[1], bar["translation"] + float_sides * 0.5 * FLOAT_ULP * t_scale),
                   ("point (float)", d_float[3], bar["point"] + float_sides * 0.5 * FLOAT_ULP * x_scale)]
    if name in ABSOLUTE_CHI2:
        checks += [("chi2_final (absolute)", abs(stats["chi2_final"] - want_stats["chi2_final"]), bar["chi2_final_absolute"])]
        if name == "consistent":
            checks += [("chi2_final (rounding)", max(stats["chi2_final"], want_stats["chi2_final"]), absolute_chi2_bar(pr)),
                       ("chi2_initial (rounding)", max(stats["chi2_initial"], want_stats["chi2_initial"]), absolute_chi2_bar(pr))]
        else:
            checks += [("chi2_initial_relative", d_double[5], bar["chi2_initial_relative"])]
    else:
        checks += [("chi2_initial_relative", d_double[5], bar["chi2_initial_relative"])]
        if name in GAUGE:       # see the module text: the step along the gauge is noise over 1e-16
            checks += [("chi2_final against chi2_initial", stats["chi2_final"], stats["chi2_initial"])]
        else:
            checks += [("chi2_final_relative", d_double[4], bar["chi2_final_relative"])]
    for key, x, allowed in checks:
        print("%s: |d %s| = %.3g (allowed %.3g)" % (what, key, x, allowed))
    for key, x, allowed in checks:
        assert x <= allowed, "%s: |d %s| = %.3g > %.3g" % (what, key, x, allowed)
