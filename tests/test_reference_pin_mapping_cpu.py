"""The restatements behind orbm_frustum, orbm_distinctive_descriptors and orbm_triangulate_matches (tests/frustum_oracle.py,
tests/mappoint_oracle.py, tests/triangulation_oracle.py) against the reference's own text: src/MapPoint.cc compiled unmodified, and
Frame::isInFrustum, KeyFrame::UnprojectStereo and LocalMapping::CreateNewMapPoints / ComputeF12 sliced out of the reference at build
time and run on real MapPoint objects (oracle/ref/ref_mapping.cc).  tests/ref_mapping.py has the cases and their plants.

  exactly   isInFrustum's result, mnTrackScaleLevel, the bits of mTrackProjX / Y / XR and mTrackViewCos; the inputs on which the int
            conversion of src/MapPoint.cc:410 is undefined (the UBSan copy reports it on exactly those, each asked alone); the row that
            ComputeDistinctiveDescriptors copies into mDescriptor, and that it leaves mDescriptor alone where nothing is left to choose
            from; per pair whether CreateNewMapPoints makes a MapPoint of it, whether it went through UnprojectStereo and of which key
            frame, the bits of the unprojected point, and the pairs that ask UnprojectStereo for a feature without depth
  by value  x3D of the 4x4 SVD (src/LocalMapping.cc:331) and F12, each within 4 x its spread between the reference's own arithmetic
            variants C and B (tests/golden/mapping/tolerance.json)

The whole loop (oracle/_ref/ref_newpoints: the same driver with the reference's src/ORBmatcher.cc linked unmodified): the numpy loop of
tests/newmappoints_batch_oracle.py, sequential and as snapshot plus replay, must give the reference's new MapPoints in its order.

The reference shows only mDescriptor: rows are distinct wherever the winning index is the point of a plant, and best_median stays
held by tests/mappoint_oracle.py alone (tests/test_mappoint_cpu.py, _gpu.py).  Of a refused pair the reference shows only that it was
refused; the line that refused it is the restatement's word, used here only to count that every line decides some pairs.

The tests on recorded fixtures (tests/golden/mapping/) run everywhere; the ones that run the binaries need the reference checkout."""
import numpy as np
import pytest

import frustum_oracle as fo
import mappoint_oracle as mo
import ref_mapping as rm
import triangulation_oracle as to

FIXTURES = rm.load_fixtures()
TOL = rm.load_tolerance()
FRUSTUM = sorted(n for k, n in FIXTURES if k == "frustum")
TRI = sorted(n for k, n in FIXTURES if k == "newpoints")


@pytest.fixture(scope="module")
def binaries():
    if not rm.ensure():
        pytest.skip("no reference checkout: the fixtures stand in")
    return True


# ---- the fixtures are the cases of today

def test_fixtures_hold_todays_cases():
    """a changed case cannot keep an old answer"""
    assert FIXTURES[("mappoint", "batch")]["req"] == rm.dd_request(rm.dd_points())
    cases = rm.frustum_cases()
    assert FRUSTUM == sorted(cases)
    for name, (sc, limit, want) in cases.items():
        fx = FIXTURES[("frustum", name)]
        sc = rm._noskip(sc)
        assert fx["full"] == rm.frustum_request(sc, limit), name
        assert fx["req"] == rm.frustum_request(sc.take(np.flatnonzero(~fx["undef"])), limit), name
    tri = rm.tri_cases()
    assert set(TRI) == set(tri) | {"mono_mono_n0", "mono_mono_n1"}
    for name in TRI:
        c = tri[name[:9] if name.startswith("mono_mono_n") else name]
        pairs = c[5]
        kept = rm.Records(FIXTURES[("newpoints", name)]["req"]).one("pairs")
        assert FIXTURES[("newpoints", name)]["req"] == rm.tri_request(*c[:5], kept, *c[6:]), name
        it = iter(map(tuple, pairs))
        assert all(tuple(p) in it for p in kept), name          # a subsequence of the case's pairs
    counts = sorted(len(rm.Records(FIXTURES[("newpoints", n)]["req"]).one("pairs")) for n in TRI)
    assert {0, 1, 63, 64, 65} <= set(counts)
    sizes = {len(rm.Records(FIXTURES[("frustum", n)]["full"]).one("xw")) for n in FRUSTUM}
    assert {0, 1, 63, 64, 65, 130} <= sizes


# ---- MapPoint::ComputeDistinctiveDescriptors

def test_distinctive_descriptor_restatement_equals_the_recorded_reference():
    fx = FIXTURES[("mappoint", "batch")]
    req, rsp = rm.Records(fx["req"]), rm.Records(fx["rsp"])
    off, desc = rm.dd_library_input(req)
    best, _ = mo.distinctive_descriptors(off, desc)
    rm.dd_check(req, rsp, best)
    pts = rm.dd_points()
    for p, (name, rows, kfbad, mpbad, want) in enumerate(pts):
        good = rows[kfbad == 0]
        if want is not None:                                    # the planted winner, straight from the reference's record
            assert (rsp.one("desc")[p] == good[want]).all(), name
        if mpbad or len(good) == 0:
            assert best[p] == -1 and (rsp.one("desc")[p] == rm.DD_INIT).all(), name
    assert set(rm.DD_SIZES) <= set(np.diff(off).tolist())


# ---- Frame::isInFrustum

@pytest.mark.parametrize("name", FRUSTUM)
def test_frustum_restatement_equals_the_recorded_reference(name):
    fx = FIXTURES[("frustum", name)]
    sc, limit = rm.frustum_scene(rm.Records(fx["full"]))
    rm.frustum_check(fx, fo.frustum(*sc.args(), limit), name)


def test_frustum_plants_hold_on_the_reference_record():
    """the flags worked out from the inputs in exact arithmetic, against what the reference returned"""
    n = 0
    for name, (sc, limit, want) in rm.frustum_cases().items():
        if want is not None:
            fx = FIXTURES[("frustum", name)]
            assert not fx["undef"].any(), name
            assert rm.Records(fx["rsp"]).one("flag").reshape(-1).tolist() == list(want), name
            n += len(want)
    assert n == 39
    und = sum(int(FIXTURES[("frustum", n)]["undef"].sum()) for n in FRUSTUM)
    flags = np.concatenate([rm.Records(FIXTURES[("frustum", n)]["rsp"]).one("flag").reshape(-1) for n in FRUSTUM])
    assert und >= 10 and flags.sum() >= 200 and (flags == 0).sum() >= 200


# ---- CreateNewMapPoints, pairs given

@pytest.mark.parametrize("name", TRI)
def test_triangulation_restatement_equals_the_recorded_reference(name):
    fx = FIXTURES[("newpoints", name)]
    req, rsp = rm.Records(fx["req"]), rm.Records(fx["rsp"])
    cam1, kf1, cams2, off2, kf2, pairs = rm.tri_inputs(req)
    status, x3d = to.triangulate(cam1, kf1, cams2, off2, kf2, pairs)
    dev = rm.tri_check(rsp, status, x3d, TOL["tolerance"], pairs[:, 2])
    print(name, "x3D deviates %.3g of %.3g" % (dev, TOL["tolerance"]))
    # the neighbours that pass :251-263: all by construction (a tenth of a baseline per metre of depth, monocular), but for the two gate
    # cases, whose first neighbour alone is removed by margins worked out from the inputs (ref_mapping.gate_case)
    assert rsp.one("gate").reshape(-1).tolist() == rm.EXPECTED_GATES.get(name, [1] * len(cams2)), name
    if name in rm.EXPECTED_GATES:
        removed = pairs[:, 2] == 0
        assert removed.sum() == 12 and (rsp.one("acc").reshape(-1)[removed] == 0).all() and (rsp.one("acc").reshape(-1)[~removed] == 1).sum() >= 5
        assert int(req.scalar("mono")) == (0 if name == "gate_baseline" else 1)
    if name in ("quirk315", "quirk408"):                        # accepted by the reference; refused under the other reading (see the case)
        assert (rsp.one("acc") == 1).all() and (rsp.one("path") == 0).all()


@pytest.mark.parametrize("name", TRI)
def test_f12_restatement_equals_the_recorded_reference(name):
    """newmappoints_batch_oracle.compute_f12, which feeds F12 to every test of orbm_create_new_map_points, against the F12 the reference's
    own ComputeF12 handed its matcher, within 4 x the spread of that matrix between the reference's variants C and B"""
    import newmappoints_batch_oracle as nb
    fx = FIXTURES[("newpoints", name)]
    cam1, _, cams2, _, _, _ = rm.tri_inputs(rm.Records(fx["req"]))
    dev = rm.f12_check(rm.Records(fx["rsp"]), cam1, cams2, nb.compute_f12, TOL["f12_tolerance"])
    print(name, "F12 deviates %.3g of %.3g" % (dev, TOL["f12_tolerance"]))


def test_every_line_of_the_loop_decides_some_pairs():
    """counted with the restatement's statuses on pairs whose accept / refuse the reference confirms: :321 (svd), :342, :346, :351, :335,
    :357, :361, :376 / :387, :402 / :413, :424, :432, and features without depth"""
    seen = np.zeros(13, int)
    ms = np.zeros((2, 2), int)                                  # [reprojection in key frame 1 / 2][monocular / stereo feature]
    for name in TRI:
        req = rm.Records(FIXTURES[("newpoints", name)]["req"])
        cam1, kf1, cams2, off2, kf2, pairs = rm.tri_inputs(req)
        status, _ = to.triangulate(cam1, kf1, cams2, off2, kf2, pairs)
        seen += np.bincount(status, minlength=13)[:13]
        if len(pairs):
            st1 = kf1.u_right[pairs[:, 0]] >= 0
            st2 = kf2.u_right[off2[pairs[:, 2]] + pairs[:, 1]] >= 0
            for g, (code, st) in enumerate(((to.REPROJ1, st1), (to.REPROJ2, st2))):
                for s in (0, 1):
                    ms[g, s] += int(((status == code) & (st == bool(s))).sum())
    assert (seen[:12] >= 3).all(), dict(zip(to.STATUS_NAMES, seen))
    assert (ms >= 3).all(), ms                                  # :376 and :387, :402 and :413


# ---- the binaries

def test_binaries_reproduce_the_fixtures_and_the_ubsan_copy_is_clean(binaries):
    keys = sorted(FIXTURES)
    jobs = [(FIXTURES[k]["req"], v) for k in keys for v in ("", "_ubsan")]
    res = rm.run_many(jobs)
    for i, k in enumerate(keys):
        for (rc, data, err), v in zip(res[2 * i:2 * i + 2], ("", "_ubsan")):
            assert rc == 0 and "runtime error" not in err, (k, v, err)
            assert data == FIXTURES[k]["rsp"], (k, v)


def test_ubsan_copy_reports_the_conversion_on_exactly_the_undefined_inputs(binaries):
    n = 0
    for name in FRUSTUM:
        fx = FIXTURES[("frustum", name)]
        sc, limit = rm.frustum_scene(rm.Records(fx["full"]))
        assert not (fx["undef"] & ~rm.maybe_undefined(sc)).any(), name
        assert (rm.split_undefined(sc, limit) == fx["undef"]).all(), name
        n += int(fx["undef"].sum())
    assert n >= 10


def test_the_tolerance_is_the_measured_spread(binaries):
    if not rm.ensure(variants=("", "_b")):
        pytest.skip("variant B of the reference is not built")
    spread, bad, n = rm.measure_tri([(name, FIXTURES[("newpoints", name)]["req"]) for name in TRI])
    assert not bad, bad                                         # C and B make every accept / refuse decision alike: the allowed share is zero
    assert n == TOL["pairs"] and spread == TOL["spread_c_b"] and TOL["tolerance"] == rm.FACTOR * spread
    assert rm.F12_SPREAD[0] == TOL["f12_spread_c_b"] and TOL["f12_tolerance"] == rm.FACTOR * rm.F12_SPREAD[0]
    rm.tri_pinned()                                             # how many pairs ride on that noise today: the recorded number, zero
    assert rm.DROPPED == TOL["pairs_dropped_because_c_and_b_decide_differently"] and not any(rm.DROPPED.values())


# ---- CreateNewMapPoints, the whole loop

LOOP = rm.load_loop_fixtures()


def _loop(name):
    import newmappoints_batch_oracle as nb
    sc, mono, depths = rm.loop_scene(name)
    fx = LOOP[name]
    assert fx["req"] == rm.loop_requests(sc, mono, depths)[0], name                          # the fixture holds today's case
    s2, live = rm.surviving_scene(sc, rm.Records(fx["gate_rsp"]))
    return nb, sc, s2, live, rm.Records(fx["rsp"])


@pytest.mark.parametrize("name", sorted(rm.LOOP_CASES))
def test_numpy_loop_and_snapshot_replay_equal_the_reference_loop(name):
    """the reference's own CreateNewMapPoints with its own SearchForTriangulation, neighbour after neighbour, against the sequential numpy
    loop (procedure A) and against every neighbour searched and triangulated on one snapshot with the loop replayed afterwards (procedure B,
    section 12b's claim): the new MapPoints and their order exactly"""
    nb, sc, s2, live, rsp = _loop(name)
    for lists in (nb.procedure_a(s2), nb.procedure_b(s2)):
        dev = rm.loop_check(rsp, live, lists, TOL["tolerance"])
    print(name, "%d new points, x3D deviates %.3g of %.3g" % (len(rsp.one("acc")), dev, TOL["tolerance"]))
    removed = [v for v in range(sc.nviews) if v not in live]
    assert removed == rm.LOOP_REMOVED.get(name, []), name
    assert len(sc.kf1) == 120 and int(rm.Records(LOOP[name]["req"]).scalar("mono")) == rm.LOOP_CASES[name][1]


def test_the_loop_cases_make_the_order_matter():
    """counted on the reference's log, with the snapshot's matches of the other neighbours: features the reference accepted for one
    neighbour that a later neighbour matches again (the replay must drop them there), and features a neighbour's triangulation refused
    that the reference accepted for a later one (the replay must keep them); one neighbour removed by each gate of :251-263"""
    again, later = {}, {}
    for name in rm.LOOP_CASES:
        nb, sc, s2, live, rsp = _loop(name)
        m12, st, _, _ = nb.snapshot(s2)
        again[name] = later[name] = 0
        for v, i1, _ in rsp.one("acc").reshape(-1, 3):
            w = live.index(v)
            again[name] += int((m12[w + 1:, i1] >= 0).any())
            later[name] += int(((m12[:w, i1] >= 0) & (st[:w, i1] > to.STEREO2)).any())
    assert max(again.values()) >= 20 and max(later.values()) >= 20, (again, later)
    assert {len(rm.LOOP_CASES[n][0]) and rm.LOOP_CASES[n][0]["nviews"] for n in rm.LOOP_CASES} == {1, 2, 3, 5}
    assert rm.LOOP_CASES["stereo-5"][1] == 0 and rm.LOOP_CASES["mono-5"][1] == 1        # :253 needs !mbMonocular, :258-262 mbMonocular


def test_loop_binaries_reproduce_the_fixtures(binaries):
    if not rm.ensure_loop():
        pytest.skip("the whole-loop build of the reference is not there")
    for name, fx in LOOP.items():
        assert rm.run_loop(fx["req"]) == fx["rsp"] and rm.run_loop(fx["req"], "_ubsan") == fx["rsp"], name
        assert rm.run_ok(rm.loop_requests(*rm.loop_scene(name))[1]).data == fx["gate_rsp"], name
