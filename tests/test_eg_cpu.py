"""No-GPU checks of Optimizer::OptimizeEssentialGraph (include/orbp.h orbp_optimize_essential_graph, include/orbm.h
orbm_optimize_essential_graph): the host path against the oracle tests/eg_oracle.py on every case of tests/eg_cases.py (estimates
and both chi2 within the bars of tests/golden/eg/tolerance.json; iteration and trial counts identical on the cases whose decisions
are clear of noise), the envelope solve against the all-dense build of the same system bit for bit (through the test-only switch
orbp_eg_set_dense: every row of the envelope then starts at column 0), what the header promises (fix_scale, a key frame without
edges, ref = -1, budgets), the exports and their declarations, and the argument checks made before any work.

Measured host against oracle, largest over the cases (the bars are 4 x the oracle's own spread): rotation 5.2e-07 of 3.9e-06,
translation 4.7e-06 of 2.2e-05, scale 5.7e-07 of 2.9e-06, point 2.1e-06 of 1.7e-05, final chi2 4.0e-08 of 1.2e-06 relative,
initial chi2 6.2e-16 of 3.7e-15 relative."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import eg_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = json.load(open(ec.TOLERANCE))


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_symbols_are_exported_and_declared(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("orbp_optimize_essential_graph", "orbm_optimize_essential_graph", "orbm_optimize_essential_graph_split"):
        assert hasattr(lib, name), name
    orbm = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    orbp = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+orbm_optimize_essential_graph\s*\(", orbm) and re.search(r"\bint\s+orbp_optimize_essential_graph\s*\(", orbp)
    assert int(re.search(r"#define\s+ORBM_EG_MAX_KFS\s+(\d+)", orbm).group(1)) == built.ORBM_EG_MAX_KFS == 438
    assert 7 * built.ORBM_EG_MAX_KFS <= built.ORBM_SPD_MAX_N < 7 * (built.ORBM_EG_MAX_KFS + 1)
    assert hasattr(built, "optimize_essential_graph") and hasattr(built.ORBmatcher, "optimize_essential_graph")
    assert C.sizeof(built.EgStats) == 32 and C.sizeof(built.EgProblem) == 80
    body = open(os.path.join(ROOT, "my-slam_amd", "csrc", "orbp_eg_body.h")).read()
    assert '#include "orbp_sim3opt_body.h"' in body and "struct S3oSim" not in body      # the Sim3 arithmetic is not copied


def test_the_tolerance_file_is_what_the_script_measures():
    """4 x the spread of the oracle's six variants over the cases, per quantity, and the list of noise-decided cases"""
    assert TOL["factor"] == 4
    for k in ec.KEYS:
        assert TOL["bar"][k] == 4 * TOL["spread"][k] and 0 < TOL["spread"][k] < 1e-4 and TOL["worst_case"][k] in ec.NAMES
    assert TOL["bar"]["chi2_initial_relative"] < 1e-13          # the tight bar: error evaluation and edge gather, no Jacobian in the way
    assert set(TOL["ill_conditioned"]) == set(ec.ILL_CONDITIONED)
    assert set(TOL["scale"]) == set(ec.SCALE_NAMES)             # each scale case has bars of its own, made the same way
    for name in ec.SCALE_NAMES:
        s = TOL["scale"][name]
        for k in ("rotation", "translation", "scale", "chi2_final_relative", "chi2_initial_relative"):
            assert s["bar"][k] == 4 * s["spread"][k] and 0 < s["spread"][k] and s["worst_case"][k] == name
        # a step of these graphs moves the corrected key frames by the correction itself (a translation of 2, an angle of 0.3): a
        # key frame that a launch left out misses every one of these bars by more than an order of magnitude
        assert s["bar"]["translation"] < 0.1 and s["bar"]["rotation"] < 1e-3 and s["bar"]["scale"] < 1e-3
        assert s["bar"]["chi2_initial_relative"] < 1e-13
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "measure_eg_spread.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_converged_list_is_the_oracles():
    assert tuple(TOL["converged"]) == ec.CONVERGED == tuple(n for n in ec.NAMES if not ec.decisions_clear(n))
    assert 3 * len(ec.CONVERGED) <= len(ec.NAMES)


def test_the_cases_cover_what_they_should():
    cs = {n: ec.case(n) for n in ec.NAMES}
    free = {n: len(c[0]["Scw"]) - (c[0]["fixed"] >= 0) - ("isolated" in c[0]) for n, c in cs.items()}
    assert {1, 6, 7, 14, 29} <= set(free.values())
    assert {0, 1, 63, 64, 65} <= {len(c[0]["xw"]) for c in cs.values()}
    assert {0, 1, 2, 3, 20} <= {c[1] for c in cs.values()}
    assert {True, False} == {bool(c[0]["fix_scale"]) for c in cs.values()}
    for name in ("fixed_first", "fixed_middle", "fixed_last", "no_fixed"):
        pr = cs[name][0]
        assert pr["fixed"] == {"fixed_first": 0, "fixed_middle": len(pr["Scw"]) // 2, "fixed_last": len(pr["Scw"]) - 1, "no_fixed": -1}[name]
    for name, count in (("pair_two_edges", 2), ("pair_three_edges", 3)):
        pr = cs[name][0]
        pairs = [tuple(sorted(e)) for e in zip(pr["edge_i"].tolist(), pr["edge_j"].tolist())]
        assert max(pairs.count(q) for q in pairs) == count
    pr = cs["isolated_kf"][0]
    assert pr["isolated"] not in set(pr["edge_i"]) | set(pr["edge_j"]) and pr["isolated"] != pr["fixed"]
    pr = cs["fixed_both_roles"][0]
    assert pr["fixed"] in set(pr["edge_i"]) and pr["fixed"] in set(pr["edge_j"])
    for name, want in ec.BRANCH_OF.items():                 # the branch of Sim3::log the boundary edges start in
        pr = cs[name][0]
        small_sigma, small_angle = ec.eo.log_branches(pr)
        chi = (ec.eo.edge_errors(*(lambda g: (g.meas, g.est[g.ei], g.est[g.ej]))(ec.eo.Graph(pr, "forward"))) ** 2).sum(-1)
        boundary = chi > 1e-6
        assert boundary.any() and (small_sigma[boundary] == want[0]).all() and (small_angle[boundary] == want[1]).all(), name
    mixed = cs["budget_3"][0]
    assert set(mixed["edge_corrected"]) == {0, 1} and not np.array_equal(mixed["Scw"], mixed["Snc"])
    tr = ec.oracle("rejected_trial")["transcript"]
    assert any(not t[2] for t in tr) and "rejected_trial" not in ec.CONVERGED
    for c in cs.values():
        if len(c[0]["xw"]) > 1:
            assert c[0]["ref"][0] == -1 and c[0]["ref"][-1] == c[0]["fixed"]


def test_the_scale_cases_reach_what_they_should():
    """the sizes at which the launches of csrc/orbm_eg.hip and csrc/orbm_spd.hip take a second and a third workgroup or stride, each
    with every decision of the oracle clear of noise in all six variants, so that the counts are compared exactly"""
    cs = {n: ec.case(n) for n in ec.SCALE_NAMES}
    N = {n: 7 * (len(c[0]["Scw"]) - 1) for n, c in cs.items()}
    assert N == {"scale_kf43": 294, "scale_kf78": 539, "scale_kf260": 1813, "scale_kf438": 3059}
    assert 256 < N["scale_kf43"] <= 512 < N["scale_kf78"] <= 768          # two and three workgroups of k_spd_backward, 256 entries each
    big = cs["scale_kf260"][0]
    assert len(big["Scw"]) > 256 and len(big["edge_i"]) == 2555 > 2 * 1024 and N["scale_kf260"] > 1024
    assert len(big["xw"]) == 300 > 256 and len(set(big["ref"][1:-1].tolist())) > 150 and big["ref"][1:-1].max() > 256
    assert len(cs[ec.AT_THE_CAP][0]["Scw"]) == 438 and len(cs[ec.AT_THE_CAP][0]["edge_i"]) == 4335
    assert [cs[n][1] for n in ec.SCALE_NAMES] == [2, 1, 1, 1]
    for n, (pr, n_it) in cs.items():
        assert pr["fixed"] == 0 and not pr["fix_scale"], n
        assert ec.decisions_clear(n), n
        stats = ec.oracle(n)["stats"]
        assert stats["iterations"] == n_it and all(ec.oracle(n, *v)["stats"][k] == stats[k] for v in ec.VARIANTS for k in ("iterations", "trials")), n


@pytest.mark.parametrize("name", ec.NAMES + ec.SCALE_NAMES)
def test_the_host_path_equals_the_oracle(built, name):
    o = ec.oracle(name)
    ec.assert_same(name, ec.host(built, name), o["Tcw"], o["Scw"][:, 7], o["xw"], o["stats"], "host " + name,
                   counts=name not in ec.CONVERGED, float_sides=1)


@pytest.mark.parametrize("name", ("kf2_one_edge", "free7", "chain30", "isolated_kf", "pair_three_edges", "no_fixed", "rejected_trial"))
def test_the_envelope_is_the_dense_factorisation_bit_for_bit(built, name):
    """Scw_out, Tcw, xw and the stats of the whole run: with every row of the envelope starting at column 0 the same code is the
    unblocked dense Cholesky, and skipping the structural zeros must change no bit"""
    pr, n_it = ec.case(name)
    env = ec.host(built, name)
    built.lib().orbp_eg_set_dense(1)
    try:
        dense = built.optimize_essential_graph(pr, n_it)
    finally:
        built.lib().orbp_eg_set_dense(0)
    assert env[0] == dense[0] == 0 and env[4] == dense[4]
    for a, b in zip(env[1:4], dense[1:4]):
        assert a.tobytes() == b.tobytes()


def test_fix_scale_keeps_every_scale_and_zeroes_the_seventh_update(built):
    pr, n_it = ec.case("fix_scale")
    code, Tcw, xw, Scw, stats = ec.host(built, "fix_scale")
    assert stats["iterations"] == n_it and Scw[:, 7].tobytes() == np.asarray(pr["Scw"])[:, 7].tobytes()
    free = [k for k in range(len(Scw)) if k != pr["fixed"]]
    assert np.abs(Scw[free, :7] - np.asarray(pr["Scw"])[free, :7]).max() > 1e-3       # the rest did move
    # without it the same graph moves its scales
    assert np.abs(built.optimize_essential_graph(dict(pr, fix_scale=False), n_it)[3][:, 7] - 1).max() > 1e-6


def test_fixed_isolated_and_unreferenced_keep_their_bits(built):
    for name in ec.NAMES:
        pr, n_it = ec.case(name)
        code, Tcw, xw, Scw, stats = ec.host(built, name)
        if pr["fixed"] >= 0:
            assert Scw[pr["fixed"]].tobytes() == np.asarray(pr["Scw"])[pr["fixed"]].tobytes(), name
        if "isolated" in pr:                                # its pivot is lambda and its update exactly zero
            assert np.array_equal(Scw[pr["isolated"]], np.asarray(pr["Scw"])[pr["isolated"]]), name
        if len(xw):
            assert xw[0].tobytes() == pr["xw"][0].tobytes(), name
            if n_it and len(xw) > 2:
                assert np.abs(xw[1:-1] - pr["xw"][1:-1]).max() > 1e-3, name
    pr, n_it = ec.case("budget_0")
    code, Tcw, xw, Scw, stats = ec.host(built, "budget_0")
    assert stats["iterations"] == stats["trials"] == 0 and stats["chi2_initial"] == stats["chi2_final"] > 1
    assert Scw.tobytes() == np.asarray(pr["Scw"]).tobytes()


def _call(built, pr, n_it=3, mutate=None, fn=None):
    s, a = built.pack_eg_problem({k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in pr.items()})
    T = np.full((max(s.n_kfs, 1), 16), 7.25, np.float32)
    if mutate:
        mutate(s, a)
    Lb = built.lib()
    if fn is None:
        rc = Lb.orbp_optimize_essential_graph(C.byref(s), n_it, p(T), p(a["xw"]), None, None)
        text = Lb.orbp_last_error()
    else:
        rc = fn(None, C.byref(s), n_it, p(T), p(a["xw"]), None, None)
        text = Lb.orbm_last_error()
    assert rc == 0 or (T == 7.25).all()
    return rc, text


def test_bad_arguments_are_refused_before_any_work(built):
    pr = ec.case("free6")[0]
    E_INV = built.ORBX_E_INVALID
    Lb = built.lib()
    assert _call(built, pr)[0] == 0
    for fn in (None, Lb.orbm_optimize_essential_graph):     # the GPU entry runs the same checks first, before the handle is looked at
        def bad(mutate, text, n_it=3):
            rc, got = _call(built, pr, n_it, mutate, fn)
            assert rc == E_INV and text in got, (text, got)
        bad(lambda s, a: setattr(s, "fixed", s.n_kfs), b"fixed")
        bad(lambda s, a: setattr(s, "fixed", -2), b"fixed")
        bad(lambda s, a: a["edge_i"].__setitem__(2, s.n_kfs), b"edge 2")
        bad(lambda s, a: a["edge_j"].__setitem__(3, -1), b"edge 3")
        bad(lambda s, a: a["edge_j"].__setitem__(4, a["edge_i"][4]), b"with itself")
        bad(lambda s, a: a["ref"].__setitem__(5, s.n_kfs), b"point 5")
        bad(lambda s, a: a["ref"].__setitem__(5, -2), b"point 5")
        bad(lambda s, a: setattr(s, "Snc", None), b"NULL")
        bad(lambda s, a: setattr(s, "edge_corrected", None), b"NULL")
        bad(lambda s, a: setattr(s, "ref", None), b"NULL")
        bad(lambda s, a: setattr(s, "n_edges", -1), b"negative")
        for value in (np.nan, np.inf):
            bad(lambda s, a, v=value: a["Scw"].__setitem__((1, 5), v), b"Scw of key frame 1 is not finite")
            bad(lambda s, a, v=value: a["Snc"].__setitem__((2, 7), v), b"Snc of key frame 2 is not finite")
        for value in (0.0, -1.0):
            bad(lambda s, a, v=value: a["Scw"].__setitem__((3, 7), v), b"Scw of key frame 3 has scale")
        for n_it in (-1, built.ORBP_BA_MAX_ITERATIONS + 1):
            bad(None, b"n_iterations", n_it)
    assert Lb.orbp_optimize_essential_graph(None, 3, None, None, None, None) == E_INV
    assert Lb.orbm_optimize_essential_graph(None, None, 3, None, None, None, None) == E_INV
    with pytest.raises(built.OrbxError):
        built.optimize_essential_graph(dict(pr, edge_j=pr["edge_j"][:-1]))


def big_counts(built, n_kfs):
    """a problem whose counts alone are large: no edges, no points"""
    S = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float64), (n_kfs, 1))
    keep = {"S": S, "T_out": np.full((n_kfs, 16), 7.25, np.float32)}
    s = built.EgProblem(n_kfs, S.ctypes.data, S.ctypes.data, 0, 0, 0, None, None, None, 0, None)
    return s, keep


def test_the_gpu_call_decides_capacity_before_the_handle_is_touched(built):
    Lb = built.lib()
    s, keep = big_counts(built, built.ORBM_EG_MAX_KFS + 1)
    assert Lb.orbm_optimize_essential_graph(None, C.byref(s), 20, p(keep["T_out"]), None, None, None) == built.ORBX_E_CAPACITY
    assert (keep["T_out"] == 7.25).all() and b"438" in Lb.orbm_last_error()
    # the host path has no cap
    assert Lb.orbp_optimize_essential_graph(C.byref(s), 20, p(keep["T_out"]), None, None, None) == 0
    assert np.array_equal(keep["T_out"], np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (len(keep["T_out"]), 1)))


def test_the_gpu_call_fails_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, text = _call(built, ec.case("free6")[0], fn=built.lib().orbm_optimize_essential_graph)
    assert rc == built.ORBX_E_HIP and b"no CPU path" in text
