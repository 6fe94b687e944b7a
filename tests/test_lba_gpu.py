"""orbm_local_bundle_adjustment (include/orbm.h) on the GPU against the host path orbp_local_bundle_adjustment on the cases of
tests/lba_cases.py: erase flags and every count of the stats identical, poses / points / final chi2 within the bar of
tests/golden/lba/tolerance.json (4 x the spread of the oracle's two summation orders, measured by tests/tools/measure_lba_spread.py)
plus the float rounding of the two outputs.  Host and kernels run one text (csrc/orbp_lba_body.h); the order of the sums over the
edges, the device's sin / cos and the inside of the dense solve are what differs.  The cases keep every decision away from its
boundary in the oracle, so a flag or a trial cannot flip for rounding."""
import json
import os

import numpy as np
import pytest

import frustum_oracle as F
import oracle_lib as O
import lba_cases as lc

pytestmark = pytest.mark.gpu

TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lba", "tolerance.json")))
BARS = tuple(TOL["bar"][k] for k in lc.KEYS)


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


_GPU = {}


def gpu(m, name):
    """the GPU call's result for case `name` on the shared handle, computed once"""
    if name not in _GPU:
        _GPU[name] = m.local_bundle_adjustment(lc.case(name))
    return _GPU[name]


def against_host(orbx, got, name, what="gpu"):
    want = lc.host(orbx, name)
    lc.assert_same(got, want[1], want[2], want[3], want[4], BARS, "%s %s" % (what, name), coordinates=name not in lc.GAUGE,
                   float_roundings=2)


def same_bytes(a, b):
    return (a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3])
            and a[4] == b[4])


@pytest.mark.parametrize("name", lc.NAMES)
def test_the_gpu_call_equals_the_host(m, orbx, name):
    against_host(orbx, gpu(m, name), name)


@pytest.mark.parametrize("name", lc.SCALE_NAMES)
def test_the_gpu_call_equals_the_oracle_at_the_cap(m, name):
    """128 free local key frames with edges: k_lba_solve's 256 threads stride three times over the 768 unknowns and walk a trailing
    triangle of 290 thousand entries.  Against the oracle's forward result within the case's own bars, and a second run's bytes."""
    f = lc.oracle(name)[0]
    bars = tuple(TOL["scale"][name]["bar"][k] for k in lc.KEYS)
    lc.assert_same(gpu(m, name), f["Tcw"], f["xw"], f["erase"], f["stats"], bars, "gpu " + name)
    assert same_bytes(gpu(m, name), m.local_bundle_adjustment(lc.case(name))), name


def test_a_second_run_gives_the_same_bytes(m):
    for name in ("k11_p257_mixed", "bad_kf", "no_free"):
        assert same_bytes(gpu(m, name), m.local_bundle_adjustment(lc.case(name))), name


def test_a_larger_problem_in_between_changes_nothing(orbx):
    """the result is a function of the problem alone: what the 43-key-frame case left in the workspace does not show"""
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        first = {n: h.local_bundle_adjustment(lc.case(n)) for n in ("k2_p65_mixed", "stale_flip", "local_id0")}
        h.local_bundle_adjustment(lc.case("k43_p1500_mixed"))
        for n, want in first.items():
            assert same_bytes(want, h.local_bundle_adjustment(lc.case(n))), n
    finally:
        h.close()


def test_a_small_handle_grows(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        against_host(orbx, h.local_bundle_adjustment(lc.case("k1_p63_mono")), "k1_p63_mono", "small handle")
        against_host(orbx, h.local_bundle_adjustment(lc.case("k11_p257_mixed")), "k11_p257_mixed", "grown handle")
        against_host(orbx, h.local_bundle_adjustment(lc.case("k1_p63_mono")), "k1_p63_mono", "grown handle")
    finally:
        h.close()


def raw(m, orbx, pr, stop=None):
    return lc.raw_call(lambda *args: m.L.orbm_local_bundle_adjustment(m.h, *args), orbx, pr, stop=stop)


def test_guards_survive_and_stop_at_entry_launches_nothing(m, orbx):
    pr = lc.case("k2_p65_mixed")
    want = gpu(m, "k2_p65_mixed")
    code, (T, x, er, st), ok, a = raw(m, orbx, pr)
    assert code == orbx.ORBP_LBA_DONE and ok, m.L.orbm_last_error()
    assert T.tobytes() == want[1].tobytes() and x.tobytes() == want[2].tobytes() and np.array_equal(er.astype(bool), want[3])
    assert ((er == 0) | (er == 1)).all()
    code, (T, x, er, st), ok, a = raw(m, orbx, pr, stop=np.ones(1, np.uint8))
    assert code == orbx.ORBP_LBA_STOPPED and ok
    assert (T == 7.25).all() and x.tobytes() == a["xw"].tobytes() and (er == 0x5A).all() and (st == 0x5A).all()
    # a handle that never ran a bundle adjustment answers a stopped call without making its workspace
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        code, _, ok, _ = raw(h, orbx, pr, stop=np.ones(1, np.uint8))
        assert code == orbx.ORBP_LBA_STOPPED and ok
    finally:
        h.close()


def test_the_handle_keeps_its_grid_and_its_neighbours_results(m, orbx):
    """in the manner of tests/test_optimize_sim3_gpu.py: a grid query and a frustum call before and after a bundle adjustment"""
    scn = F.suite_scene(0)
    fr = F.make_frame(np.random.default_rng(31), scn)
    bounds = tuple(float(b) for b in scn.view["bounds"])
    m.grid_build(fr.kps, *bounds)
    og = O.FrameGrid(fr.kps, *bounds)
    rng = np.random.default_rng(5)
    qx, qy = rng.uniform(0, bounds[1], 200).astype(np.float32), rng.uniform(0, bounds[3], 200).astype(np.float32)

    def neighbours():
        off, idx = m.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        for q in (0, 17, 199):
            assert np.array_equal(idx[off[q]:off[q + 1]], og.features_in_area(float(qx[q]), float(qy[q]), 25.0, 0, 3))
        return (off, idx) + tuple(m.frustum(*scn.args(), 0.5))

    before = neighbours()
    against_host(orbx, m.local_bundle_adjustment(lc.case("k11_p257_mixed")), "k11_p257_mixed")
    assert m.grid_count() == len(fr.kps)
    after = neighbours()
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
