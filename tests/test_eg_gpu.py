"""orbm_optimize_essential_graph (include/orbm.h) on the GPU against the host path orbp_optimize_essential_graph on the cases of
tests/eg_cases.py: estimates and both chi2 within the bars of tests/golden/eg/tolerance.json (4 x the spread of the oracle's six
variants, measured by tests/tools/measure_eg_spread.py) plus the float rounding of the two sides' outputs; iteration and trial
counts identical on the cases whose decisions are clear of noise.  Host and kernels run one text (csrc/orbp_eg_body.h); the
device's acos / sin / cos / log / exp, the trees of the chi2 and computeScale sums and the solve (csrc/orbm_spd.hip here, the
envelope Cholesky there) are what differs.  Also: the bytes of a second run and of a run after a bundle_adjustment on the same
handle (the solve's workspace is shared), fix_scale's exact zeros, the bits of ref = -1, the cap.  The scale cases (43, 78, 260
and 438 key frames: every launch of csrc/orbm_eg.hip beyond one workgroup) are held to the oracle itself, each within its own bars."""
import ctypes as C

import numpy as np
import pytest

import ba_cases as bc
import eg_cases as ec
from test_eg_cpu import big_counts, p

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    yield h
    h.close()


_GPU = {}


def run(h, name):
    pr, n_it = ec.case(name)
    return h.optimize_essential_graph(pr, n_it)


def gpu(m, name):
    """the GPU call's result for case `name` on the shared handle, computed once"""
    if name not in _GPU:
        _GPU[name] = run(m, name)
    return _GPU[name]


def same_bytes(a, b):
    return a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:4], b[1:4])) and a[4] == b[4]


@pytest.mark.parametrize("name", ec.NAMES)
def test_the_gpu_call_equals_the_host(m, orbx, name):
    want = ec.host(orbx, name)
    ec.assert_same(name, gpu(m, name), ec.tcw_of(want[3]), want[3][:, 7], want[2], want[4], "gpu " + name,
                   counts=name not in ec.CONVERGED, float_sides=2)


@pytest.mark.parametrize("name", ec.SCALE_NAMES)
def test_the_gpu_call_equals_the_oracle_where_launches_span_workgroups(m, name):
    """the scale cases of tests/eg_cases.py against the oracle's forward result: identical counts, Scw in double, Tcw, the scale,
    the points (scale_kf260 carries 300) and both chi2 within that case's own bars"""
    o = ec.oracle(name)
    ec.assert_same(name, gpu(m, name), o["Tcw"], o["Scw"][:, 7], o["xw"], o["stats"], "gpu " + name, counts=True, float_sides=1)


def test_the_small_scale_case_keeps_its_bytes_after_the_cap(m):
    """43 key frames before and after 438 on the same handle: the workspace grows from 0.7 MB to 75 MB in between"""
    h = m.__class__(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        first = run(h, "scale_kf43")
        assert same_bytes(first, gpu(m, "scale_kf43"))
        assert same_bytes(run(h, ec.AT_THE_CAP), gpu(m, ec.AT_THE_CAP))
        assert same_bytes(first, run(h, "scale_kf43"))
    finally:
        h.close()


def test_the_bytes_depend_on_the_problem_alone(m):
    """a second run, and a run after a bundle_adjustment on the same handle, whose reduced system lies in the same workspace"""
    names = ("kf2_one_edge", "free6", "free7", "chain30", "isolated_kf", "pair_three_edges", "rejected_trial")
    first = {n: gpu(m, n) for n in names}
    for n in names:
        assert same_bytes(first[n], run(m, n)), n
    pr, n_it, robust = bc.case("k9_p65_mixed")
    m.bundle_adjustment(pr, n_it, robust)
    for n in names:
        assert same_bytes(first[n], run(m, n)), "after bundle_adjustment: " + n


def test_fix_scale_keeps_every_scale_and_zeroes_the_seventh_update(m):
    pr, n_it = ec.case("fix_scale")
    code, Tcw, xw, Scw, stats = gpu(m, "fix_scale")
    assert stats["iterations"] == n_it and Scw[:, 7].tobytes() == np.asarray(pr["Scw"])[:, 7].tobytes()
    free = [k for k in range(len(Scw)) if k != pr["fixed"]]
    assert np.abs(Scw[free, :7] - np.asarray(pr["Scw"])[free, :7]).max() > 1e-3


def test_fixed_isolated_and_unreferenced_keep_their_bits(m):
    for name in ec.NAMES:
        pr, n_it = ec.case(name)
        code, Tcw, xw, Scw, stats = gpu(m, name)
        if pr["fixed"] >= 0:
            assert Scw[pr["fixed"]].tobytes() == np.asarray(pr["Scw"])[pr["fixed"]].tobytes(), name
        if "isolated" in pr:
            assert np.array_equal(Scw[pr["isolated"]], np.asarray(pr["Scw"])[pr["isolated"]]), name
        if len(xw):
            assert xw[0].tobytes() == pr["xw"][0].tobytes(), name


def test_beyond_the_capacity(m, orbx):
    """439 key frames are refused from the counts and the handle goes on; 438 run"""
    s, keep = big_counts(orbx, orbx.ORBM_EG_MAX_KFS + 1)
    assert m.L.orbm_optimize_essential_graph(m.h, C.byref(s), 20, p(keep["T_out"]), None, None, None) == orbx.ORBX_E_CAPACITY
    assert (keep["T_out"] == 7.25).all()
    assert same_bytes(gpu(m, "free7"), run(m, "free7"))
    s, keep = big_counts(orbx, orbx.ORBM_EG_MAX_KFS)
    assert m.L.orbm_optimize_essential_graph(m.h, C.byref(s), 20, p(keep["T_out"]), None, None, None) == 0
    assert np.array_equal(keep["T_out"], np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (len(keep["T_out"]), 1)))


def test_at_the_cap_with_edges(m, orbx):
    """438 key frames as a chain plus a band of 10 plus a loop of 10 edges (the largest shape of tools/bench_eg.py, 3059 unknowns),
    one iteration: the same counts as the host, the initial chi2 (4335 edges, no Jacobian in it), and a step that Levenberg
    accepted.  The initial chi2 is a sum
    of E non-negative terms, in edge order on the host and by a tree on the device: each order is within (E - 1) eps / 2 of the exact
    sum, so the two lie within (E - 1) eps of each other, on top of the bar, which covers what the terms themselves may differ by.
    The graph is the case scale_kf438 of tests/eg_cases.py: the estimates of the GPU and of the host are each held to the oracle's
    within that case's own bars."""
    n = orbx.ORBM_EG_MAX_KFS
    pr, n_it = ec.case(ec.AT_THE_CAP)
    assert len(pr["Scw"]) == n and n_it == 1
    host, got = ec.host(orbx, ec.AT_THE_CAP), gpu(m, ec.AT_THE_CAP)
    assert got[0] == host[0] == 0 and got[4]["iterations"] == host[4]["iterations"] == 1 and got[4]["trials"] == host[4]["trials"] == 1
    rel = abs(got[4]["chi2_initial"] - host[4]["chi2_initial"]) / host[4]["chi2_initial"]
    print("chi2_initial %.17g, relative difference %.3g; chi2_final gpu %.9g host %.9g" % (host[4]["chi2_initial"], rel, got[4]["chi2_final"],
                                                                                         host[4]["chi2_final"]))
    assert rel <= ec.bars("free6")["chi2_initial_relative"] + (len(pr["edge_i"]) - 1) * np.finfo(np.float64).eps
    assert np.isfinite(got[3]).all() and 0 <= got[4]["chi2_final"] < got[4]["chi2_initial"]
    assert got[3][0].tobytes() == np.asarray(pr["Scw"])[0].tobytes()
    o = ec.oracle(ec.AT_THE_CAP)
    for what, res in (("gpu", got), ("host", host)):
        ec.assert_same(ec.AT_THE_CAP, res, o["Tcw"], o["Scw"][:, 7], o["xw"], o["stats"], what + " at the cap", counts=True, float_sides=1)
