"""orbm_search_for_triangulation and orbm_create_new_map_points share one search kernel and one host preparation
(csrc/orbm_newpoints.hip): they refuse the same malformed FeatureVectors, and the one-view call's view record does not leak
into a batch call on the same handle, nor the other way round."""
import copy
import ctypes as C

import numpy as np
import pytest

import newmappoints_batch_oracle as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(orbx):
    m = orbx.ORBmatcher(0.6, False)
    yield m
    m.close()


# ---- FeatureVector refusal: two key frames of 8 features in 3 nodes (3 + 3 + 2)

def tiny_scene():
    sc = B.make_scene(seed=808, nviews=1, npts=8, node_size=3, seen=1.0, has_mp=0.0, outliers=0.0, baselines=(0.5, 1.0))
    assert len(sc.kf1) == 8 and len(sc.kfs2[0]) == 8 and len(sc.fv1[0]) == 3 and len(sc.fvs2[0][0]) == 3
    return sc


def malformed(fv, kind, n):
    node, off, idx = [np.array(a, np.int32) for a in fv]
    if kind == "offset":
        off[2] = off[1] - 1                      # a decreasing offset
    elif kind == "node":
        node[1], node[2] = node[2], node[1]      # node ids not ascending
    elif kind == "index":
        idx[4] = n                               # an index equal to n
    return node, off, idx


def raw_search(orbx, m, sc):
    """the C call itself, on outputs filled with junk: (status, matches12, nmatches)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    kf1, kf2 = sc.kf1, sc.kfs2[0]
    Cw, T2w, K2, F12, sf2, sg2 = sc.search_args(0)
    keep = [np.ascontiguousarray(kf1.kps_un), sc.desc1, sc.has1, f32(kf1.u_right), *[i32(a) for a in sc.fv1],
            np.ascontiguousarray(kf2.kps_un), sc.descs2[0], sc.has2[0], f32(kf2.u_right), *[i32(a) for a in sc.fvs2[0]],
            f32(Cw).reshape(3), f32(T2w).reshape(16), f32(F12).reshape(9), f32(sf2), f32(sg2)]
    k1, d1, h1, u1, n1n, n1o, n1i, k2, d2, h2, u2, n2n, n2o, n2i, cw, t2w, f12, sf, sg = keep
    m12, nm = np.full(len(d1), 7, np.int32), C.c_int(5)
    rc = m.L.orbm_search_for_triangulation(m.h, p(k1), p(d1), len(d1), p(h1), p(u1), p(n1n), p(n1o), p(n1i), len(n1n),
                                           p(k2), p(d2), len(d2), p(h2), p(u2), p(n2n), p(n2o), p(n2i), len(n2n),
                                           p(cw), p(t2w), *K2, p(f12), p(sf), p(sg), len(sf), 0, 0, p(m12), C.byref(nm))
    return rc, m12, nm.value


def test_the_valid_tiny_scene_passes_both_entry_points(orbx, matcher):
    sc = tiny_scene()
    rc, m12, nm = raw_search(orbx, matcher, sc)
    assert rc == orbx.ORBX_OK
    want = B.search_view(sc, 0, sc.has1)
    assert np.array_equal(m12, want) and nm == int((want >= 0).sum())
    got = matcher.create_new_map_points(*sc.batch_args())
    assert np.array_equal(got[0][0], want)


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("kind", ["offset", "node", "index"])
def test_both_entry_points_refuse_a_malformed_feature_vector(orbx, matcher, which, kind):
    sc = copy.copy(tiny_scene())
    if which == 1:
        sc.fv1 = malformed(sc.fv1, kind, 8)
    else:
        sc.fvs2 = [malformed(sc.fvs2[0], kind, 8)]
    rc, m12, nm = raw_search(orbx, matcher, sc)
    assert rc == orbx.ORBX_E_INVALID, (rc, matcher.L.orbm_last_error())
    assert (m12 == -1).all() and nm == 0
    with pytest.raises(orbx.OrbxError) as e:
        matcher.create_new_map_points(*sc.batch_args())
    assert e.value.code == orbx.ORBX_E_INVALID
    # the handle is as usable as before
    good = tiny_scene()
    rc, m12, _ = raw_search(orbx, matcher, good)
    assert rc == orbx.ORBX_OK and np.array_equal(m12, B.search_view(good, 0, good.has1))


# ---- the one-view record next to a batch call's records on one handle

def per_view(m, sc, v):
    kf2 = sc.kfs2[v]
    Cw, T2w, K2, F12, sf2, sigma2 = sc.search_args(v)
    return m.SearchForTriangulation(sc.kf1.kps_un, sc.desc1, sc.has1, sc.kf1.u_right, sc.fv1, kf2.kps_un, sc.descs2[v], sc.has2[v],
                                    kf2.u_right, sc.fvs2[v], Cw, T2w, K2, F12, sf2, sigma2, sc.only_stereo)


def same_dense(got, want):
    for g, w, field in zip(got, want, ("matches12", "status", "x3d", "nmatches")):
        if field == "x3d":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), field


def test_one_view_search_after_a_batch_call_and_before_one(orbx):
    sc = B.make_scene(seed=121, nviews=3, npts=150, node_size=4, baselines=(0.5, 3.0))
    want = B.snapshot(sc)
    assert (want[3] > 0).all()
    m = orbx.ORBmatcher(0.6, False)
    same_dense(m.create_new_map_points(*sc.batch_args()), want)
    for v in (2, 1, 0):                          # view 2's features start at a base > 0 in the batch call; here every base is 0
        m12, nm = per_view(m, sc, v)
        assert np.array_equal(m12, want[0][v]) and nm == want[3][v], v
    m.close()
    m = orbx.ORBmatcher(0.6, False)              # the reverse order, on a fresh handle
    m12, nm = per_view(m, sc, 2)
    assert np.array_equal(m12, want[0][2]) and nm == want[3][2]
    same_dense(m.create_new_map_points(*sc.batch_args()), want)
    m12, nm = per_view(m, sc, 1)
    assert np.array_equal(m12, want[0][1]) and nm == want[3][1]
    m.close()
