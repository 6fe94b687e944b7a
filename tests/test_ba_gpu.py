"""orbm_bundle_adjustment (include/orbm.h) on the GPU against the host path orbp_bundle_adjustment on the cases of
tests/ba_cases.py: iteration and trial counts identical, poses / points / final chi2 within the bar of
tests/golden/ba/tolerance.json (4 x the spread of the oracle's two summation orders, measured by tests/tools/measure_ba_spread.py)
plus the float rounding of the two outputs.  Host and kernels run one text (csrc/orbp_lba_body.h); the order of the sums over the
edges, the device's sin / cos and the solve of the reduced system (csrc/orbm_spd.hip here, dense Cholesky there) are what differs.
Also: the bytes of a second run, of a run after a LocalBundleAdjustment and after the largest case on the same handle; `stop` at
every read; the capacity bounds."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ba_cases as bc
import lba_cases as lc
from test_ba_cpu import big_counts, check_sweep, host_sweep, sweep_of, p

pytestmark = pytest.mark.gpu

TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba", "tolerance.json")))
BARS = tuple(TOL["bar"][k] for k in bc.KEYS)


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    yield h
    h.close()


_GPU = {}


def run(h, name, stop=None):
    pr, n_it, robust = bc.case(name)
    return h.bundle_adjustment(pr, n_it, robust, stop)


def gpu(m, name):
    """the GPU call's result for case `name` on the shared handle, computed once"""
    if name not in _GPU:
        _GPU[name] = run(m, name)
    return _GPU[name]


def same_bytes(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]


@pytest.mark.parametrize("name", bc.NAMES)
def test_the_gpu_call_equals_the_host(m, orbx, name):
    want = bc.host(orbx, name)
    bc.assert_same(gpu(m, name), want[1], want[2], want[3], BARS, "gpu " + name, coordinates=name not in bc.GAUGE, float_roundings=2)


@pytest.mark.parametrize("name", bc.SCALE_NAMES)
def test_the_gpu_call_equals_the_oracle_where_the_solve_spans_workgroups(m, name):
    """the scale cases of tests/ba_cases.py (dense reduced systems of 294, 534 and 3072 unknowns) against the oracle's forward
    result: identical counts; poses, points and final chi2 within that case's own bars plus the float rounding of the one output"""
    f = bc.oracle(name)[0]
    bars = tuple(TOL["scale"][name]["bar"][k] for k in bc.KEYS)
    bc.assert_same(gpu(m, name), f["Tcw"], f["xw"], f["stats"], bars, "gpu " + name, float_roundings=1)


def test_the_scale_cases_keep_their_bytes(m, orbx):
    """512 key frames with edges give the same bytes on a second run, and 49 the same bytes before and after them on one handle,
    whose workspace grows in between"""
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        first = run(h, "scale_k49")
        assert same_bytes(first, gpu(m, "scale_k49"))
        assert same_bytes(run(h, bc.AT_THE_CAP), gpu(m, bc.AT_THE_CAP))
        assert same_bytes(first, run(h, "scale_k49"))
    finally:
        h.close()


def test_vertices_without_edges_and_robust(m):
    pr = bc.case("empty_vertices")[0]
    xw = gpu(m, "empty_vertices")[2]
    assert xw[pr["empty_point"]].tobytes() == pr["xw"][pr["empty_point"]].tobytes()
    a, b = gpu(m, "k8_p64_robust"), gpu(m, "k8_p64_plain")
    assert np.abs(a[2] - b[2]).max() > 1e-3 and b[3]["chi2"] > 2 * a[3]["chi2"]


def test_the_bytes_depend_on_the_problem_alone(m, orbx):
    """a second run; a run after a LocalBundleAdjustment (the other user of the workspace, with the one-workgroup solve); a run
    after the largest case; and a fresh handle"""
    names = ("k7_p63_stereo", "k8_p64_robust", "k9_p65_mixed", "empty_vertices", "rejecting")
    first = {n: gpu(m, n) for n in names}
    for n in names:
        assert same_bytes(first[n], run(m, n)), n
    m.local_bundle_adjustment(lc.case("k11_p257_mixed"))
    for n in names:
        assert same_bytes(first[n], run(m, n)), "after LocalBundleAdjustment: " + n
    big = gpu(m, bc.LARGEST)
    assert same_bytes(big, run(m, bc.LARGEST))
    for n in names:
        assert same_bytes(first[n], run(m, n)), "after the largest case: " + n
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        assert same_bytes(first["k9_p65_mixed"], run(h, "k9_p65_mixed"))
    finally:
        h.close()


def test_beyond_the_capacity(m, orbx):
    """513 key frames without points, and a key frame x point table one point beyond 2^26 entries: both refused from the counts,
    and the handle goes on"""
    for n_local, n_points in ((orbx.ORBM_BA_MAX_KFS + 1, 0), (orbx.ORBM_BA_MAX_KFS, orbx.ORBM_BA_MAX_TABLE // orbx.ORBM_BA_MAX_KFS + 1)):
        s, keep = big_counts(orbx, n_local, n_points)
        rc = m.L.orbm_bundle_adjustment(m.h, C.byref(s), 10, 0, p(keep["T_out"]), p(keep["xw"]), None, None)
        assert rc == orbx.ORBX_E_CAPACITY and (keep["T_out"] == 7.25).all(), (n_local, n_points, m.L.orbm_last_error())
        assert same_bytes(gpu(m, "k8_p64_robust"), run(m, "k8_p64_robust"))
    # at the bound itself the call runs: 512 key frames without edges, every block of the reduced system the identity
    s, keep = big_counts(orbx, orbx.ORBM_BA_MAX_KFS, 0)
    assert m.L.orbm_bundle_adjustment(m.h, C.byref(s), 10, 0, p(keep["T_out"]), p(keep["xw"]), None, None) == 0
    assert np.array_equal(keep["T_out"], keep["Tcw"])


@pytest.mark.parametrize("name", ("k8_p64_robust", "rejecting"))
def test_the_gpu_call_reads_stop_where_the_host_does(m, orbx, name):
    sweep = sweep_of(orbx, m.bundle_adjustment, name)
    check_sweep(sweep, name, "gpu " + name)
    host = host_sweep(orbx, name)
    assert sweep["reads"] == host["reads"]
    for n in range(1, sweep["reads"] + 2):
        assert sweep[n][0] == host[n][0] and all(sweep[n][3][k] == host[n][3][k] for k in ("iterations", "trials")), (name, n)
    assert same_bytes(sweep[0], gpu(m, name))
