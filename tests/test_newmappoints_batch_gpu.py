"""orbm_create_new_map_points on the MI355X (include/orbm.h): every neighbour of LocalMapping::CreateNewMapPoints searched and
triangulated in one call.  All comparisons are exact: indices and statuses equal, x3D equal as bit patterns.  The batch call is
compared with the two existing entry points called view by view (orbm_search_for_triangulation, orbm_triangulate_matches) and
with the oracles (tests/newmappoints_batch_oracle.py), which also pins the existing entry points to each other."""
import copy

import numpy as np
import pytest

import newmappoints_batch_oracle as B
import triangulation_oracle as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(orbx):
    m = orbx.ORBmatcher(0.6, False)             # LocalMapping.cc:217
    yield m
    m.close()


_snapshots = {}


def suite(name):
    """(scene, the oracle's dense outputs), computed once per scene"""
    if name not in _snapshots:
        sc = B.degenerate_scene() if name == "degenerate" else B.suite_scene(name)
        _snapshots[name] = (sc, B.snapshot(sc))
    return _snapshots[name]


def same_dense(got, want, what):
    for g, w, field in zip(got, want, ("matches12", "status", "x3d", "nmatches")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, field, g.shape, w.shape, g.dtype, w.dtype)
        if field == "x3d":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s differs at %s: %s, expected %s" % (what, field, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def per_view_calls(m, sc):
    """the loop the batch call replaces, on the snapshot: the dense outputs from the two existing entry points"""
    n1 = len(sc.kf1)
    m12 = np.full((sc.nviews, n1), -1, np.int32)
    status = np.full((sc.nviews, n1), B.NO_MATCH, np.uint8)
    x3d = np.zeros((sc.nviews, n1, 3), np.float32)
    nm = np.zeros(sc.nviews, np.int32)
    for v in range(sc.nviews):
        kf2 = sc.kfs2[v]
        Cw, T2w, K2, F12, sf2, sigma2 = sc.search_args(v)
        m12[v], nm[v] = m.SearchForTriangulation(sc.kf1.kps_un, sc.desc1, sc.has1, sc.kf1.u_right, sc.fv1, kf2.kps_un, sc.descs2[v], sc.has2[v],
                                                 kf2.u_right, sc.fvs2[v], Cw, T2w, K2, F12, sf2, sigma2, sc.only_stereo)
        i1 = np.nonzero(m12[v] >= 0)[0]
        matches = np.stack([i1, m12[v, i1], np.zeros(len(i1), np.int64)], 1).astype(np.int32)
        st, x = m.triangulate_matches(sc.cam1, sc.kf1.kps_un, sc.kf1.keys_xy, sc.kf1.u_right, sc.kf1.depth, [sc.cams2[v]], [0, len(kf2)],
                                      kf2.kps_un, kf2.keys_xy, kf2.u_right, kf2.depth, matches)
        status[v, i1], x3d[v, i1] = st, x
    return m12, status, x3d, nm


def check(m, sc, want=None, existing=True):
    want = B.snapshot(sc) if want is None else want
    got = m.create_new_map_points(*sc.batch_args())
    same_dense(got, want, "batch call against the oracle")
    if existing:
        same_dense(per_view_calls(m, sc), want, "per-view entry points against the oracle")
    assert ((got[1] == B.NO_MATCH) == (got[0] < 0)).all()
    return got


def count_queries(sc):
    """(view, feature of key frame 1) pairs the search visits: no MapPoint, the stereo filter, a node the view holds features in"""
    nodes1 = np.repeat(sc.fv1[0], np.diff(sc.fv1[1]))
    usable = (sc.has1[sc.fv1[2]] == 0) & ((sc.kf1.u_right[sc.fv1[2]] >= 0) | (not sc.only_stereo))
    total = 0
    for v in range(sc.nviews):
        if len(sc.kfs2[v]) == 0:
            continue
        held = sc.fvs2[v][0][np.diff(sc.fvs2[v][1]) > 0]
        total += int((usable & np.isin(nodes1, held)).sum())
    return total


# ---- the suite

@pytest.mark.parametrize("name", list(B.SUITE) + ["degenerate"])
def test_batch_equals_per_view_calls_and_oracle(matcher, name):
    sc, want = suite(name)
    got = check(matcher, sc, want)
    assert got[3].sum() > 0
    assert B.same_lists(B.replay(sc, got), B.procedure_a(sc))           # and through the replay, the reference's order


def test_every_status_occurs_in_the_batch_outputs():
    """On the oracle: every orbm_tri_status that tests/test_triangulate_gpu.py reaches (all but BAD_INDEX) is in some slot."""
    total = np.zeros(256, np.int64)
    for name in list(B.SUITE) + ["degenerate"]:
        total += np.bincount(suite(name)[1][1].ravel(), minlength=256)
    print(dict(zip(T.STATUS_NAMES, total[:13])), "empty slots", total[B.NO_MATCH])
    for code in range(T.UNDEFINED + 1):
        assert total[code] >= 1, (T.STATUS_NAMES[code], total[:13])
    assert total[T.BAD_INDEX] == 0 and total[B.NO_MATCH] > 0


def test_the_suite_reaches_the_shapes_it_names():
    """nviews 1 and 8, nodes of more than 64 and more than 256 candidates, duplicated descriptors, different levels and calibration"""
    assert suite("mono-1")[0].nviews == 1 and suite("mixed-8")[0].nviews == 8
    assert 64 < np.diff(suite("mixed-8")[0].fvs2[0][1]).max() <= 256
    assert np.diff(suite("mixed-2-one-node")[0].fvs2[0][1]).max() > 256
    sc = suite("duplicates-3")[0]
    assert len(np.unique(sc.descs2[0], axis=0)) < len(sc.descs2[0]) / 2
    sc = suite("mixed-5-calib")[0]
    assert len({int(c["nlevels"]) for c in sc.cams2}) == 3 and len({float(c["fx"]) for c in sc.cams2}) == 2


def test_ties_take_the_last_candidate(matcher):
    """The property is asserted on the oracle's output, which the call has just been found equal to: among a node's identical
    descriptors the candidate with the highest position that passes the tests is the match (here every one passes the epipolar
    test: sigma2 = 1e12)."""
    sc, want = suite("duplicates-3")
    check(matcher, sc, want, existing=False)
    got = want
    node1 = np.repeat(sc.fv1[0], np.diff(sc.fv1[1]))[np.argsort(sc.fv1[2])]           # node of every feature of key frame 1
    later = 0
    for v in range(sc.nviews):
        node, off, idx = sc.fvs2[v]
        for i1 in np.nonzero(got[0][v] >= 0)[0]:
            a = np.searchsorted(node, node1[i1])
            members = idx[off[a]:off[a + 1]]
            eligible = members[(sc.has2[v][members] == 0)]
            stereo_pair = (sc.kf1.u_right[i1] >= 0) | (sc.kfs2[v].u_right[eligible] >= 0)
            if stereo_pair.all():                                                   # no epipole test: every eligible member ties
                assert got[0][v, i1] == eligible[-1]
                later += len(eligible) > 1
    assert later >= 10


# ---- sizes at the edges of the decomposition

def single_view_scene():
    return B.make_scene(seed=120, nviews=1, npts=200, stereo1=0.4, stereo2=0.4, node_size=1, baselines=(0.5, 2.0), has_mp=0.0)


@pytest.mark.parametrize("nq", [0, 1, 3, 4, 5])
def test_total_queries_at_the_workgroup_edge(matcher, nq):
    """four waves per workgroup in the search: 0 (no launch), 1, 3, 4, 5 queries"""
    sc = single_view_scene()
    seen = np.isin(sc.fv1[0], sc.fvs2[0][0])                # node_size 1: feature c of fv1 is a query iff its node is in the view
    keep = sc.fv1[2][seen][:nq]
    sc.has1[:] = 1
    sc.has1[keep] = 0
    assert count_queries(sc) == nq
    got = check(matcher, sc)
    assert (got[0][:, sc.has1 == 1] < 0).all()


@pytest.mark.parametrize("npairs", [0, 1, 63, 64, 65])
def test_total_pairs_at_the_wave_edge(matcher, npairs):
    """one lane per query in the triangulation: 0, 1, 63, 64 and 65 matched pairs (asserted on the oracle's count)"""
    sc = single_view_scene()
    full = B.snapshot(sc)
    matched = np.nonzero(full[0][0] >= 0)[0]
    assert len(matched) >= 65
    sc.has1[matched[npairs:]] = 1
    want = B.snapshot(sc)
    assert want[3].sum() == npairs and count_queries(sc) > npairs
    check(matcher, sc, want)


def three_views():
    return B.make_scene(seed=121, nviews=3, npts=150, node_size=4, baselines=(0.5, 3.0))


def test_a_view_without_features(matcher):
    sc = three_views()
    sc.kfs2[1] = T.KeyFrame(np.zeros(0, T.KP_DTYPE), np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    sc.descs2[1], sc.has2[1] = np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8)
    sc.fvs2[1] = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    got = check(matcher, sc, existing=False)
    assert got[3][1] == 0 and got[3][0] > 0 and got[3][2] > 0


def test_a_view_sharing_no_node(matcher):
    sc = three_views()
    node, off, idx = sc.fvs2[0]
    sc.fvs2[0] = (node + 10 ** 7, off, idx)
    got = check(matcher, sc)
    assert got[3][0] == 0 and got[3][1] > 0 and got[3][2] > 0


def test_a_view_whose_every_feature_has_a_map_point(matcher):
    sc = three_views()
    sc.has2[2][:] = 1
    got = check(matcher, sc)
    assert got[3][2] == 0 and got[3][0] > 0 and got[3][1] > 0


def test_key_frame_1_with_every_slot_taken_needs_no_launch(matcher):
    sc = three_views()
    sc.has1[:] = 1
    got = check(matcher, sc)
    assert (got[0] == -1).all() and (got[1] == B.NO_MATCH).all() and not got[2].any() and not got[3].any()


# ---- the handle

def test_a_call_larger_than_the_handle_grows_it(orbx):
    sc, want = suite("mixed-8")
    m = orbx.ORBmatcher(0.6, False, max_queries=8, max_train=8, max_pairs=8)
    try:
        assert count_queries(sc) > 8 * 3
        for _ in range(2):                       # the growing call and a call on the grown handle
            same_dense(m.create_new_map_points(*sc.batch_args()), want, "small handle")
    finally:
        m.close()


def test_the_grid_in_the_handle_is_left_as_it_was(orbx):
    sc, want = suite("mono-5")
    m = orbx.ORBmatcher(0.6, False, max_queries=64, max_train=512, max_pairs=64)
    try:
        kps = sc.kf1.kps_un
        m.grid_build(kps, 0.0, 1241.0, 0.0, 376.0)
        x, y = kps["x"][:50].copy(), kps["y"][:50].copy()
        before = m.GetFeaturesInArea(x, y, 40.0)
        assert m.grid_count() == len(kps) and len(before[1]) > 50
        same_dense(m.create_new_map_points(*sc.batch_args()), want, "handle with a grid")       # grows the query workspace on the way
        assert m.grid_count() == len(kps)
        after = m.GetFeaturesInArea(x, y, 40.0)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        m.close()


def test_repeated_calls_on_one_handle_agree(matcher):
    """the staging arena and the result buffer are reused: a larger call, a smaller one, the larger again"""
    big, small = suite("mixed-8"), suite("mono-1")
    for sc, want in (big, small, big):
        same_dense(matcher.create_new_map_points(*copy.deepcopy(sc).batch_args()), want, "repeated call")
