"""No-GPU checks of orbm_create_new_map_points (include/orbm.h): the replay rule on the oracles, and the entry point's argument
checks through ctypes.

The batch call searches and triangulates every neighbour on one snapshot; the caller then drops, at each neighbour's turn, the
pairs whose feature of key frame 1 has received a MapPoint since (tests/newmappoints_batch_oracle.py, procedure B).  That this
equals the reference's neighbour-by-neighbour order (procedure A) is an argument about the reference's code (DESIGN.md section
12b); here it is checked on the C oracle of SearchForTriangulation and the numpy restatement of the per-match loop."""
import ctypes as C

import numpy as np
import pytest

import newmappoints_batch_oracle as B
import triangulation_oracle as T


@pytest.fixture(scope="module")
def suite():
    """name -> (scene, procedure A's lists, the snapshot's dense outputs), computed once"""
    out = {}
    for name in B.SUITE:
        sc = B.suite_scene(name)
        out[name] = (sc, B.procedure_a(sc), B.snapshot(sc))
    return out


@pytest.mark.parametrize("name", list(B.SUITE))
def test_replay_of_the_snapshot_equals_the_sequential_order(suite, name):
    sc, a, dense = suite[name]
    b = B.replay(sc, dense)
    assert len(a) == sc.nviews
    for v, ((pa, sa, xa), (pb, sb, xb)) in enumerate(zip(a, b)):
        assert np.array_equal(pa, pb), "view %d: pair lists differ" % v
        assert np.array_equal(sa, sb), "view %d: statuses differ" % v
        assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32)), "view %d: x3D differs" % v
    assert B.same_lists(a, b)


def test_the_suite_covers_what_it_is_about(suite):
    """On procedure A's output: the skip matters, the retry matters, every view of the 5-view scene contributes."""
    assert {sc.nviews for sc, _, _ in suite.values()} >= {1, 2, 5, 8}
    assert {sc.only_stereo for sc, _, _ in suite.values()} == {False, True}
    skipped = retried = 0
    for name, (sc, a, dense) in suite.items():
        m12 = dense[0]
        accepted_in = np.full(len(sc.kf1), -1)          # the view that gave the feature its MapPoint
        rejected_in = np.full(len(sc.kf1), -1)          # the first view whose triangulation refused it
        for v, (pairs, st, _) in enumerate(a):
            ok = pairs[st <= T.STEREO2, 0]
            assert (accepted_in[ok] < 0).all(), "a feature was given two MapPoints"
            retried += int((rejected_in[ok] >= 0).sum())
            accepted_in[ok] = v
            bad = pairs[st > T.STEREO2, 0]
            rejected_in[bad] = np.where(rejected_in[bad] < 0, v, rejected_in[bad])
        for v in range(sc.nviews):                      # matched on the snapshot in a view after the one that accepted it
            skipped += int(((m12[v] >= 0) & (accepted_in >= 0) & (accepted_in < v)).sum())
    print("skipped %d, retried %d" % (skipped, retried))
    assert skipped >= 20 and retried >= 20
    for v, (pairs, st, _) in enumerate(suite["mono-5"][1]):
        assert (st <= T.STEREO2).sum() >= 1, "view %d of the 5-view scene accepts nothing" % v


def test_the_suite_spans_the_node_sizes_and_camera_kinds(suite):
    sizes = {B.SUITE[n].get("node_size", 6) for n in B.SUITE}
    assert 1 in sizes and max(sizes) >= 10 ** 6 and len(sizes) >= 4
    kinds = set()
    for sc, _, _ in suite.values():
        s1 = (sc.kf1.u_right >= 0).mean()
        s2 = np.mean([(k.u_right >= 0).mean() for k in sc.kfs2])
        kinds.add(("mono" if s1 == 0 else "stereo" if s1 > 0.9 else "mixed", "mono" if s2 == 0 else "stereo" if s2 > 0.9 else "mixed"))
    assert ("mono", "mono") in kinds and ("stereo", "stereo") in kinds and any("mixed" in k for k in kinds)


# ---- the library without a GPU

@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


NAMES = ("cam1", "k1", "x1", "u1", "z1", "d1", "n1", "h1", "f1n", "f1o", "f1i", "f1c", "cams2", "F12", "nviews", "off2", "k2", "x2", "u2", "z2",
         "d2", "h2", "fvo", "f2n", "f2o", "f2i", "only_stereo", "m12", "st", "x", "nm")


def _args(nviews=3):
    sc = B.make_scene(seed=9, nviews=nviews, npts=40, node_size=4)
    (cam1, k1, x1, u1, z1, d1, h1, fv1, cams2, F12, off2, k2, x2, u2, z2, d2, h2, fvo, fv2, only_stereo) = sc.batch_args()
    n1 = len(k1)
    a = dict(cam1=np.array([cam1]), k1=k1.copy(), x1=x1, u1=u1, z1=z1, d1=d1, n1=n1, h1=h1.copy(), f1n=fv1[0].copy(), f1o=fv1[1].copy(),
             f1i=fv1[2].copy(), f1c=len(fv1[0]), cams2=cams2.copy(), F12=F12, nviews=nviews, off2=off2.copy(), k2=k2.copy(), x2=x2, u2=u2, z2=z2, d2=d2,
             h2=h2, fvo=fvo.copy(), f2n=fv2[0].copy(), f2o=fv2[1].copy(), f2i=fv2[2].copy(), only_stereo=0,
             m12=np.full((nviews, n1), 77, np.int32), st=np.full((nviews, n1), 77, np.uint8), x=np.full((nviews, n1, 3), 77, np.float32),
             nm=np.full(nviews, 77, np.int32))
    return a


def _call(Lb, a, handle=None):
    return Lb.orbm_create_new_map_points(handle, *[a[k] if isinstance(a[k], int) else p(a[k]) for k in NAMES])


def _untouched(a):
    return all(a[k] is None or (a[k] == 77).all() for k in ("m12", "st", "x", "nm"))


def test_the_symbol_and_its_wrapper_exist(built):
    """Fails on a library built without my-slam_amd/csrc/orbm_newpoints.hip."""
    assert hasattr(C.CDLL(built.LIB_PATH), "orbm_create_new_map_points")
    assert hasattr(built.ORBmatcher, "create_new_map_points")
    assert built.ORBM_TRI_NO_MATCH == B.NO_MATCH == 255


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument gets ORBX_E_INVALID and a text, and no output is
    written."""
    Lb = built.lib()
    E = built.ORBX_E_INVALID

    def bad(mutate, text):
        b = _args()
        mutate(b)
        assert _call(Lb, b) == E and text in Lb.orbm_last_error(), Lb.orbm_last_error()
        assert _untouched(b)

    bad(lambda b: b["off2"].__setitem__(0, 1), b"off2[0]")
    bad(lambda b: b["off2"].__setitem__(2, 0), b"off2 not monotone")
    bad(lambda b: b["fvo"].__setitem__(0, 2), b"fv2_view_off[0]")
    bad(lambda b: b["fvo"].__setitem__(1, int(b["fvo"][2]) + 1), b"fv2_view_off not monotone")
    bad(lambda b: b["f2i"].__setitem__(3, int(b["off2"][1])), b"feature index")           # first view: one past its last feature
    bad(lambda b: b["f2i"].__setitem__(len(b["f2i"]) - 1, -1), b"feature index -1")
    bad(lambda b: b["f1i"].__setitem__(0, b["n1"]), b"feature index")
    bad(lambda b: b["f1o"].__setitem__(1, -1), b"monotone")
    bad(lambda b: b["cams2"]["nlevels"].__setitem__(1, 0), b"nlevels=0")
    bad(lambda b: b["cam1"]["nlevels"].__setitem__(0, 0), b"nlevels=0")
    bad(lambda b: b["cams2"]["nlevels"].__setitem__(2, 17), b"nlevels=17")
    bad(lambda b: b["k1"]["octave"].__setitem__(5, 8), b"octave 8")
    bad(lambda b: b["k2"]["octave"].__setitem__(7, -1), b"octave -1")
    bad(lambda b: b.__setitem__("n1", -1), b"n1=-1")
    bad(lambda b: b.__setitem__("nviews", -2), b"nviews=-2")
    for key in ("m12", "st", "x", "nm", "cam1", "k1", "x1", "u1", "z1", "d1", "h1", "f1n", "f1o", "f1i", "cams2", "F12", "off2", "k2", "x2", "u2",
                "z2", "d2", "h2", "fvo", "f2n", "f2o", "f2i"):
        bad(lambda b: b.__setitem__(key, None), b"NULL")


def test_nothing_to_do_is_a_success_that_touches_nothing(built):
    Lb = built.lib()
    a = _args()
    for key, val in (("nviews", 0), ("n1", 0)):
        b = dict(a)
        b[key] = val
        assert _call(Lb, b) == built.ORBX_OK
        assert _untouched(b)
    assert Lb.orbm_create_new_map_points(None, *([None] * 6), 0, *([None] * 4), 0, None, None, 0, *([None] * 11), 0, *([None] * 4)) == built.ORBX_OK


def test_a_call_without_a_query_is_answered_on_the_host(built):
    """Every feature of key frame 1 has a MapPoint: nothing is searched, the handle is not needed, every slot is empty."""
    Lb = built.lib()
    a = _args()
    a["h1"][:] = 1
    assert _call(Lb, a) == built.ORBX_OK
    assert (a["m12"] == -1).all() and (a["st"] == 255).all() and (a["x"] == 0).all() and (a["nm"] == 0).all()


def test_the_entry_point_fails_loudly_without_a_handle(built):
    import torch
    Lb = built.lib()
    a = _args()
    if torch.cuda.is_available():                                        # with a device the NULL handle is the caller's mistake
        assert _call(Lb, a) == built.ORBX_E_INVALID and b"NULL handle" in Lb.orbm_last_error()
    else:
        assert _call(Lb, a) == built.ORBX_E_HIP and b"no CPU path" in Lb.orbm_last_error()
    assert _untouched(a)                                                 # no half answer
