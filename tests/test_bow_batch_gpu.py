"""The four SearchByBoW entry points on the GPU (include/orbm.h): the tables and counts of one batch call, and of one one-candidate
call per candidate on a second handle, against the CPU oracle called once per candidate (tests/oracle_lib.py).  Both must equal the
oracle as arrays, with no tolerance.  Inputs: tests/bow_batch_cases.py.

Run as a program (`python tests/test_bow_batch_gpu.py`) it is the child of the forced-host-selection test: ORBM_BOW_HOST_SELECT is
read once per process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bow_batch_cases as B

pytestmark = pytest.mark.gpu


def batch(m, case):
    if case.variant == "frame":
        return m.SearchByBoWBatch([c.tup() for c in case.cands], case.shared.tup())
    return m.SearchByBoWKFBatch(case.shared.tup(), [c.tup() for c in case.cands])


def single(m, case, cand):
    s = case.shared
    if case.variant == "frame":
        return m.SearchByBoW(cand.kps, cand.desc, cand.fv, s.kps, s.desc, s.fv, valid_kf=cand.valid)
    return m.SearchByBoWKF(s.kps, s.desc, s.fv, s.valid, cand.kps, cand.desc, cand.fv, cand.valid)


def singles(m, case):
    table = np.full((len(case.cands), len(case.shared)), -1, np.int32)
    counts = np.zeros(len(case.cands), np.int32)
    for c, cand in enumerate(case.cands):
        table[c], counts[c] = single(m, case, cand)
    return table, counts


def check(orbx, case, ref=None):
    """one batch call on a fresh handle == the oracle == one call per candidate on a second handle (both calls are one
    implementation, so each is held against the oracle itself)"""
    want_t, want_n = ref if ref is not None else B.oracle(case)
    m, m2 = orbx.ORBmatcher(case.nnratio, case.check_ori), orbx.ORBmatcher(case.nnratio, case.check_ori)
    try:
        got_t, got_n = batch(m, case)
        one_t, one_n = singles(m2, case)
    finally:
        m.close(); m2.close()
    assert got_t.shape == want_t.shape and got_t.dtype == np.int32
    assert np.array_equal(got_n, want_n), (case.name, got_n, want_n)
    assert np.array_equal(got_t, want_t), (case.name, np.argwhere(got_t != want_t)[:8])
    assert np.array_equal(one_n, want_n), (case.name, one_n, want_n)
    assert np.array_equal(one_t, want_t), (case.name, np.argwhere(one_t != want_t)[:8])
    assert np.array_equal(one_n, got_n) and np.array_equal(one_t, got_t), case.name
    return got_t, got_n


@functools.lru_cache(maxsize=None)
def shape17(variant, sizes):
    case = B.shape_case(variant, sizes, 17)
    return case, B.oracle(case)


@pytest.mark.parametrize("k", [1, 2, 5, 17])
@pytest.mark.parametrize("sizes", ["one", "many"])
@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_staging_edges_and_mixed_workgroups(orbx, variant, sizes, k):
    """Shared side of 300 features.  In one node: five lane chunks in the frame variant, and the candidates' lists in that node have
    exactly 300, 65, 64, 63, 1 and 0 entries, all usable: serial counts around the staging batch of 64 in the frame variant (one full
    round, a full round and one more, several rounds), lane counts in the key-frame variant (300: beyond the 256 held in
    registers).  In about 100 nodes: the usual shape.  17 candidates put waves of different candidates into one workgroup."""
    case, (t, n) = shape17(variant, sizes)
    if sizes == "one":
        node = case.shared.fv[0][0]
        assert B.list_in_node(case.shared, node)[0] == 300
        for c, cand in enumerate(case.cands):
            if c not in (6, 7):                           # the absent and the all-invalid candidate
                want = B.SERIAL_COUNTS[c % len(B.SERIAL_COUNTS)]
                assert B.list_in_node(cand, node) == (want, want), (c, B.list_in_node(cand, node))
        assert {B.list_in_node(cand, node)[0] for cand in case.cands[:5]} == {300, 65, 64, 63, 1}
    _, counts = check(orbx, case.first(k), (t[:k], n[:k]))
    assert counts[0] >= 20


@pytest.mark.parametrize("nnratio", [0.6, 0.75, 0.9])
@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_mixed_candidates(orbx, variant, check_ori, nnratio):
    """different sizes, an empty candidate, one without a shared node, one whose valid is all zero, a NULL mask next to given ones"""
    case = B.variants_case(variant).with_params(nnratio, check_ori)
    table, counts = check(orbx, case)
    assert counts[1] == 0 and counts[2] == 0 and counts[3] == 0 and (table[1:4] == -1).all() and counts[0] >= 20
    if variant == "frame":
        assert case.cands[4].valid is None and case.cands[0].valid is not None


@pytest.mark.parametrize("nnratio", [0.75, 0.9, 1.5])
@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_contests_and_ties(orbx, variant, nnratio):
    """the planted contests are won by the first in list order; equal keys resolve to the first in the list (nnratio > 1 lets the
    tie through the ratio test).  For the key-frame variant the inverted table is the one compared."""
    case = B.contest_case(variant).with_params(nnratio, True)
    table, _ = check(orbx, case)
    for c, s1, s2, lane in case.contests:
        pairs = B.pairs_of(case, table[c])
        assert (s1, lane) in pairs and not any(s == s2 for s, _ in pairs)
    for c, s, l1, l2 in case.ties:
        pairs = B.pairs_of(case, table[c])
        if nnratio > 1:
            assert (s, l1) in pairs and not any(b == l2 for _, b in pairs)
        else:
            assert not any(a == s or b in (l1, l2) for a, b in pairs)


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_a_node_beyond_the_lanes_takes_the_host_selection(orbx, variant):
    """frame: 4200 lane-side features in the first node, 50 in the second; candidate 0 lives in the small node only and stays in the
    launch, candidates 1 and 2 are in both.  kf: candidate 1 brings a node of more than 4096 usable features of its own."""
    case = B.fallback_case(variant)
    if variant == "frame":
        assert list(np.diff(case.shared.fv[1])) == [4200, 50]
        big = case.shared.fv[0][0]
        assert big not in case.cands[0].fv[0] and big in case.cands[1].fv[0] and big in case.cands[2].fv[0]
    else:
        c1 = case.cands[1]
        node = case.shared.fv[0][0]
        k = list(c1.fv[0]).index(node)
        assert c1.valid[c1.fv[2][c1.fv[1][k]:c1.fv[1][k + 1]]].sum() > 4096
    _, counts = check(orbx, case)
    assert (counts >= 20).all()


def test_forced_host_selection_in_a_child_process():
    """ORBM_BOW_HOST_SELECT=1 sends every candidate of a batch call and every one-candidate call through the host selection"""
    env = dict(os.environ, ORBM_BOW_HOST_SELECT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "forced host selection ok: 2 cases" in r.stdout


# ---- handle state

def test_a_small_handle_takes_the_batch_as_its_first_call_and_grows(orbx):
    for variant in ("frame", "kf"):
        case = B.variants_case(variant)
        want_t, want_n = B.oracle(case)
        m = orbx.ORBmatcher(case.nnratio, case.check_ori, max_queries=64, max_train=64, max_pairs=64)
        try:
            got_t, got_n = batch(m, case)
            again_t, again_n = batch(m, case)               # the second call goes through the grown arena
        finally:
            m.close()
        assert np.array_equal(got_t, want_t) and np.array_equal(got_n, want_n)
        assert np.array_equal(again_t, want_t) and np.array_equal(again_n, want_n)


def test_single_batch_single_on_one_handle(orbx):
    for variant in ("frame", "kf"):
        case = B.contest_case(variant)
        m = orbx.ORBmatcher(case.nnratio, case.check_ori)
        try:
            before = [single(m, case, c) for c in case.cands]
            got_t, got_n = batch(m, case)
            after = [single(m, case, c) for c in case.cands]
        finally:
            m.close()
        for c in range(len(case.cands)):
            assert np.array_equal(before[c][0], after[c][0]) and before[c][1] == after[c][1]
            assert np.array_equal(before[c][0], got_t[c]) and before[c][1] == got_n[c]


def test_the_grid_slots_stay_as_they_were(orbx):
    case = B.variants_case("frame")
    m = orbx.ORBmatcher(case.nnratio, case.check_ori)
    try:
        kps = np.zeros(500, orbx.KP_DTYPE)
        rng = np.random.default_rng(4)
        kps["x"], kps["y"] = rng.uniform(0, 640, 500), rng.uniform(0, 480, 500)
        m.grid_build(kps, 0.0, 640.0, 0.0, 480.0)
        assert m.grid_count() == 500
        for v in ("frame", "kf"):
            batch(m, B.variants_case(v))
            assert m.grid_count() == 500
        # candidates that take the host selection, sides within the handle's max_train (8192 here); with sides beyond it:
        # test_no_search_by_bow_call_drops_the_grid
        fb = B.fallback_case("frame")
        assert max(len(fb.shared), max(len(c) for c in fb.cands)) <= 8192
        batch(m, fb)
        assert m.grid_count() == 500
    finally:
        m.close()


def test_a_small_handle_takes_a_one_candidate_call_as_its_first_call_and_grows(orbx):
    """the 220-feature candidate on a handle made for 64: the result buffer grows in the call"""
    for variant in ("frame", "kf"):
        case = B.variants_case(variant).first(1)
        assert len(case.cands[0]) >= 220 and len(case.shared) > 64
        want_t, want_n = B.oracle(case)
        m = orbx.ORBmatcher(case.nnratio, case.check_ori, max_queries=64, max_train=64, max_pairs=64)
        try:
            got = single(m, case, case.cands[0])
            again = single(m, case, case.cands[0])          # the second call goes through the grown arena
        finally:
            m.close()
        for t, n in (got, again):
            assert np.array_equal(t, want_t[0]) and n == want_n[0], variant


def test_no_search_by_bow_call_drops_the_grid(orbx):
    """A handle whose train capacity (64) is below every side: the calls grow the result buffer alone, so the Frame grid and what
    GetFeaturesInArea reads from it stay -- after a one-candidate call of either variant and after a batch whose candidates take the
    host selection."""
    m = orbx.ORBmatcher(0.75, True, max_train=64)
    try:
        kps = np.zeros(60, orbx.KP_DTYPE)
        rng = np.random.default_rng(6)
        kps["x"], kps["y"] = rng.uniform(0, 640, 60), rng.uniform(0, 480, 60)
        m.grid_build(kps, 0.0, 640.0, 0.0, 480.0)
        wx, wy, wr = np.array([100, 320, 500, 630], np.float32), np.array([80, 240, 400, 470], np.float32), np.float32(150)
        off0, idx0 = m.GetFeaturesInArea(wx, wy, wr)
        assert m.grid_count() == 60 and off0[-1] > 10

        def grid_as_it_was():
            off, idx = m.GetFeaturesInArea(wx, wy, wr)
            return m.grid_count() == 60 and np.array_equal(off, off0) and np.array_equal(idx, idx0)

        for variant in ("frame", "kf"):
            case = B.variants_case(variant)
            assert len(case.shared) > 64 and len(case.cands[0]) > 64
            _, n = single(m, case, case.cands[0])
            assert n >= 20 and grid_as_it_was(), variant
        fb = B.fallback_case("frame")
        assert len(fb.shared) > 64                      # the shared side of every host-selection call is above max_train
        _, counts = batch(m, fb)
        assert (counts >= 20).all() and grid_as_it_was()
    finally:
        m.close()


def _child():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest
    orbx = conftest._load_pkg()
    assert os.environ.get("ORBM_BOW_HOST_SELECT") == "1"
    n = 0
    for variant in ("frame", "kf"):
        case = B.variants_case(variant)
        want_t, want_n = B.oracle(case)
        m = orbx.ORBmatcher(case.nnratio, case.check_ori)
        got_t, got_n = batch(m, case)
        one_t, one_n = singles(m, case)
        m.close()
        if not (np.array_equal(got_t, want_t) and np.array_equal(got_n, want_n) and np.array_equal(one_t, want_t) and np.array_equal(one_n, want_n)):
            print("forced host selection: %s differs from the oracle" % case.name)
            return 1
        n += 1
    print("forced host selection ok: %d cases" % n)
    return 0


if __name__ == "__main__":
    sys.exit(_child())
