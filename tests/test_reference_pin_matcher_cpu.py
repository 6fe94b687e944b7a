"""The eleven ORBmatcher searches of the oracle (oracle/orb_oracle.c, oracle/orb_oracle_kf.c) against the reference's own
src/ORBmatcher.cc (oracle/_ref/ref_matcher: compiled unmodified behind oracle/ref/matcher_standin.h, Frame / KeyFrame / MapPoint
helper members sliced out of the reference, the OpenCV shim in its arithmetic variant C; DESIGN.md section 2, "What is pinned for
the ORBmatcher").  Everything is compared exactly: match tables and return values as integers, float in/out state as bits, Fuse's
best_idx read from the reference's call log.  Where oracle/_ref/ is absent the recorded responses of tests/golden/matcher/ answer
instead (cases they do not hold are skipped); one test always holds the oracle to the fixtures."""
import numpy as np
import pytest

import oracle_lib as O
import ref_matcher as R

CASES = R.all_cases()
FIXTURES = R.fixture_cases()
IDS = [c.name for c in CASES]


def _diff(a, b):
    return {f: (np.asarray(a[f]), np.asarray(b[f])) for f in a if not np.array_equal(np.asarray(a[f]), np.asarray(b[f]))}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_reference(case):
    want, rec = R.ask_case(case)
    got = R.run(O, case)
    assert R.same(got, want), _diff(got, want)
    for f, v in case.expect.items():                    # what the plant proves from its inputs
        assert np.array_equal(want[f], v), (f, want[f], v)
        assert np.array_equal(got[f], v), (f, got[f], v)
    if "mutations" in case.ref_only:                    # Fuse's effect on the key frame: the reference's alone
        assert R.fuse_mutations(rec) == case.ref_only["mutations"]
        for f in ("slot", "slotobs", "bad"):
            assert np.array_equal(rec.one(f).reshape(-1), case.ref_only[f]), f


def test_call_log_names_the_line_a_map_point_left_at():
    """The planted key frame of tests/window_cases.py under Fuse: the last call made on behalf of a MapPoint is the line the
    reference left the loop body at.  Proved from the inputs: `offl` / `offt` project left of / above mnMinX / mnMinY (:867);
    `offr` / `offb` lie inside the int bounds but beyond the last cell, `empty` has no key point near (:894); `none` has two
    neighbours, both outside the level window (:911), so it reaches the descriptor and GetMapPoint is never asked; the unused entries
    stop at the head of the loop; a fused point ends in AddObservation / AddMapPoint or Replace."""
    case = next(c for c in CASES if c.name == "wc-fuse-plain-all")
    import window_cases as wc
    names = wc.kf_case("plain")["names"]
    want, rec = R.ask_case(case)
    last = dict(zip(names, R.last_call_per_point(len(names), rec)))
    rows = R.log(rec)
    arg_of = lambda name, call: [int(a) for c, m, a in rows if m == names.index(name) and c == call]
    for name in ("offl", "offt"):
        assert last[name] == R.IS_IN_IMAGE and arg_of(name, R.IS_IN_IMAGE) == [0]
    for name in ("offr", "offb", "empty"):
        assert last[name] == R.FEATURES_IN_AREA and arg_of(name, R.FEATURES_IN_AREA) == [0]
    assert last["none"] == R.GET_DESCRIPTOR and arg_of("none", R.FEATURES_IN_AREA) == [2]
    for name in ("off", "off2"):
        assert last[name] in (0, R.IS_BAD, R.IS_IN_KEYFRAME)
    for name, bi in zip(names, want["best_idx"]):
        assert (bi >= 0) == (last[name] in (R.ADD_MAP_POINT, R.ADD_OBSERVATION, R.REPLACE, R.OBSERVATIONS)), name
        if bi >= 0:
            assert arg_of(name, R.GET_MAP_POINT) == [bi]
    levels = {n: arg_of(n, R.PREDICT_SCALE) for n in names}
    fx = wc.kf_case("plain")
    for n, lv in zip(names, fx["lv"]):                  # PredictScale is the reference's own text: the planted level comes back
        assert levels[n] in ([], [int(lv)])


def test_the_oracle_holds_to_the_committed_fixtures():
    """runs with and without oracle/_ref/: the recorded responses of the pin against the oracle"""
    held = 0
    for case in FIXTURES:
        want, _ = R.ask_case(case, "golden")
        got = R.run(O, case)
        assert R.same(got, want), (case.name, _diff(got, want))
        held += 1
    assert held == len(FIXTURES) and {c.kind for c in FIXTURES} == set(R.KINDS)


def test_fixtures_are_reproduced_byte_for_byte():
    if not R.have_binary():
        pytest.skip("oracle/_ref/ref_matcher is absent")
    assert len(R.golden()) == len(FIXTURES)
    for _, (path, name, rsp) in sorted(R.golden().items()):
        z = np.load(R.os.path.join(R.GOLDEN, path))
        rc, data, err = R.run_binary(z[name + "_req"].tobytes())
        assert rc == 0 and data == rsp, (path, name, err)


def test_every_request_passes_the_ubsan_copy():
    """nothing undefined is executed on any pinned case, and the instrumented copy answers as the pin does"""
    if not (R.have_binary() and R.have_binary("_ubsan")):
        pytest.skip("oracle/_ref/ref_matcher_ubsan is absent")
    for case in CASES:
        _, rec = R.ask_case(case, "binary")
        rc, data, err = R.run_binary(rec.request, "_ubsan")
        assert rc == 0 and err == "" and data == rec.data, (case.name, err)


def test_variant_a_agrees_on_every_planted_case():
    """Variant A of the shim (float dot, double scaling, no +0 rule) is the sensitivity run: a planted case is decided by the
    reference's text alone, so both variants answer alike; on the scene cases the disagreements are counted (0 of 27)."""
    if not (R.have_binary() and R.have_binary("_a")):
        pytest.skip("oracle/_ref/ref_matcher_a is absent (make -C oracle/ref measure)")
    differ = []
    for case in CASES:
        c, _ = R.ask_case(case, "binary")
        a, _ = R.ask_case(case, "binary", "_a")
        if not R.same(a, c):
            assert not case.planted, case.name
            differ.append(case.name)
    assert differ == []


def test_undefined_inputs_stop_the_ubsan_copy_at_predict_scale():
    """The inputs include/orbm.h lists as undefined in the reference: the UBSan copy reports the int conversion of
    MapPoint::PredictScale (the reference's own text, sliced into mappoint_scale.inc) and nothing else; they are compared with nothing."""
    if not R.have_binary("_ubsan"):
        pytest.skip("oracle/_ref/ref_matcher_ubsan is absent")
    for case in R.undefined_cases():
        rc, data, err = R.run_binary(R.request_of(case), "_ubsan")
        reports = [line for line in err.splitlines() if "runtime error" in line]
        assert rc != 0 and len(reports) == 1, (case.name, err)
        assert "mappoint_scale.inc" in reports[0] and "outside the range of representable values of type 'int'" in reports[0], reports
