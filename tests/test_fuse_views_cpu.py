"""No-GPU checks of orbm_fuse_views (include/orbm.h): the replay rule on the oracles, the planted fixtures against their hand-derived
answers, and the entry point's argument checks and host answers through ctypes.

The batch call searches every (view, MapPoint) slot on one snapshot; the adapter then replays the reference's bookkeeping in order
and re-selects on the host for the slots whose MapPoint's descriptor has changed since (tests/fuse_views_oracle.py: replay).  That
this equals the reference's key frame by key frame order (sequential) is an argument about the reference's code (DESIGN.md section
17); here it is checked on the C oracle of Fuse and an object-graph model whose Replace updates the survivor's descriptor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frustum_oracle as F
import fuse_views_cases as FC
import fuse_views_oracle as FV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def suite():
    """name -> (scene, the snapshot's dense outputs), computed once"""
    return {name: (sc, FV.snapshot(sc)) for name, sc in ((n, FV.suite_scene(n)) for n in FV.SUITE)}


@pytest.fixture(scope="module")
def planted():
    return FC.cases()


@pytest.mark.parametrize("name", list(FV.SUITE))
def test_replay_of_the_snapshot_equals_the_sequential_order(suite, name):
    sc, dense = suite[name]
    a, counts_a = FV.sequential(sc)
    b, counts_b, _ = FV.replay(sc, dense)
    ga, gb = a.graph(), b.graph()
    for k, (ma, mb) in enumerate(zip(ga[0], gb[0])):
        assert ma == mb, "MapPoint %d differs: (bad, replaced, observations, nObs, descriptor) %r / %r" % (k, ma[:4], mb[:4])
    for k, (sa, sb) in enumerate(zip(ga[1], gb[1])):
        assert sa == sb, "key frame %d: slots differ" % k
    assert counts_a == counts_b
    assert sum(counts_a) == sum(counts_b)


def test_the_reselection_rule_is_needed(suite):
    """On the planted scene the snapshot's selection for (view 1, P) is the feature the reference does not take: without the rule
    the replay ends in another graph, with it in the reference's."""
    sc, dense = suite["reselect"]
    a, counts_a = FV.sequential(sc)
    without, counts_w, _ = FV.replay(sc, dense, reselect=False)
    with_rule, counts_r, nres = FV.replay(sc, dense)
    assert counts_a == [1, 1]
    assert dense[1][1, 0] == 0 and a.kfs[1].slots[0] is None and a.kfs[1].slots[1] is a.mps[0]      # the snapshot says c1, the reference takes c2
    assert a.mps[1].bad and a.mps[1].replaced is a.mps[0] and a.mps[0].desc.tobytes() != dense[8][0].tobytes()
    assert without.graph() != a.graph() and counts_w == counts_a         # same counts, another feature
    assert with_rule.graph() == a.graph() and counts_r == counts_a and nres == 1


def test_reselection_happens_on_the_random_scenes_too(suite):
    """descriptors do change between key frames of the random scenes: the rule is exercised beyond the planted one"""
    n = {name: FV.replay(sc, dense)[2] for name, (sc, dense) in suite.items()}
    print(n)
    assert n["mix-5"] >= 10 and n["n64-4"] >= 1


def test_the_two_logf_agree_on_the_suite(suite, orbx):
    """frustum_oracle.predict_scale (correctly rounded logf, the library's kernels) and orbm_predict_scale (the host's logf, the
    existing per-view path and the C oracle) give the same level for every slot that reaches :887: no slot has to be left out of
    a comparison between the two."""
    orbx.build()
    L = orbx.lib()
    total = differ = 0
    for name, (sc, _) in suite.items():
        for k, (st, _, _, _, lv, dist) in enumerate(sc.projection()):
            V = sc.views[k]
            for i in np.flatnonzero(st == FV.NO_MATCH):
                host = L.orbm_predict_scale(C.c_float(sc.mf_max[i]), C.c_float(dist[i]), C.c_float(V["log_scale_factor"]), int(V["nlevels"]))
                total += 1
                differ += int(host != lv[i])
    print("slots that reach :887: %d, levels that differ: %d" % (total, differ))
    assert total > 300 and differ == 0


def test_the_suite_covers_what_it_is_about(suite):
    seen = np.zeros(8, np.int64)
    for sc, dense in suite.values():
        seen += np.bincount(dense[0].ravel(), minlength=8)
    print(dict(zip(FV.STATUS_NAMES, seen)))
    assert (seen > 0).all(), "a status value does not occur: %s" % dict(zip(FV.STATUS_NAMES, seen))
    sizes = [len(f) for sc, _ in suite.values() for f in sc.feats]
    assert 0 in sizes and 1 in sizes and 70 in sizes and max(sizes) >= 400
    assert {sc.n_mp for sc, _ in suite.values()} >= {1, 63, 64, 65, 200}
    assert {sc.nviews for sc, _ in suite.values()} >= {1, 2, 3, 4, 5}
    mixed = [f for sc, _ in suite.values() for f in sc.feats if (f.u_right >= 0).any() and (f.u_right < 0).any()]
    assert len(mixed) >= 3, "no view with monocular and stereo features"
    sc, dense = suite["skipview-3"]
    assert (dense[0][1] == FV.SKIPPED).all() and len(sc.feats[1]) > 0, "no view with every slot skipped"
    assert any(any(m is None for m in sc.state().vp) for sc, _ in suite.values()), "no NULL entry in a MapPoint list"
    # both directions of Replace and the plain AddObservation occur in the sequential order
    sc, dense = suite["mix-5"]
    a, _ = FV.sequential(sc)
    replaced = [m for m in a.mps if m.replaced is not None]
    in_list = {id(m) for m in a.vp if m is not None}
    assert any(id(m) in in_list for m in replaced) and any(id(m) not in in_list for m in replaced)


@pytest.mark.parametrize("name", list(FC.cases()))
def test_the_oracles_give_the_hand_derived_answers(planted, name):
    c = planted[name]
    feat = c.features()
    st, u, v, ur, lv, _ = FV.project(c.view, c.skip[0], c.xw, c.normal, c.mf_max, c.mf_min)
    reached = st == FV.NO_MATCH
    bi, bd = np.full(len(st), -1, np.int32), np.full(len(st), 256, np.int32)
    for i in np.flatnonzero(reached):
        idx, d = FV.select(c.view, feat, u[i], v[i], ur[i], lv[i], c.mp_desc[i], c.th)
        bd[i] = d
        if d <= FV.TH_LOW:
            bi[i], st[i] = idx, FV.MATCH
    assert st.tolist() == c.status.tolist()
    assert bi.tolist() == c.best_idx.tolist()
    assert bd.tolist() == c.best_dist.tolist()
    if c.oro:
        obi = FV.oro_fuse(c.view, feat, reached.astype(np.uint8), c.xw, c.normal, c.mf_max, c.mf_min, c.mp_desc, c.th)
        assert obi.tolist() == c.best_idx.tolist()


def test_the_planted_gate_edges_are_one_float_apart(planted):
    mi, mo, si, so = planted["gates"].edges
    assert np.nextafter(np.float32(mi), np.float32(1e9)) == np.float32(mo) and np.nextafter(np.float32(si), np.float32(0)) == np.float32(so)
    assert abs(mi - 100.0 - 5.99 ** 0.5) < 1e-4 and abs(260.0 - si - 7.8 ** 0.5) < 1e-4


# ---- the library without a GPU

@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


NAMES = ("views", "nviews", "off", "kps", "ur", "dk", "n_mp", "skip", "xw", "normal", "mf_max", "mf_min", "mp_desc", "th", "status", "bi", "bd",
         "pu", "pv", "pr", "lv", "nf")
OUTS = ("status", "bi", "bd", "pu", "pv", "pr", "lv", "nf")


def _args(name="n64-4"):
    sc = FV.suite_scene(name)
    views, off, kps, ur, dk, skip, xw, normal, mf_max, mf_min, mp_desc = sc.inputs()
    nv, n = sc.nviews, sc.n_mp
    a = dict(views=views.copy(), nviews=nv, off=off.copy(), kps=kps, ur=ur, dk=dk, n_mp=n, skip=skip.copy(), xw=xw, normal=normal, mf_max=mf_max,
             mf_min=mf_min, mp_desc=mp_desc, th=C.c_float(3.0),
             status=np.full((nv, n), 77, np.uint8), bi=np.full((nv, n), 77, np.int32), bd=np.full((nv, n), 77, np.int32),
             pu=np.full((nv, n), 77, np.float32), pv=np.full((nv, n), 77, np.float32), pr=np.full((nv, n), 77, np.float32),
             lv=np.full((nv, n), 77, np.int32), nf=np.full(nv, 77, np.int32))
    return sc, a


def _call(Lb, a, handle=None):
    return Lb.orbm_fuse_views(handle, *[a[k] if isinstance(a[k], (int, C.c_float)) else p(a[k]) for k in NAMES])


def _untouched(a):
    return all(a[k] is None or (a[k] == 77).all() for k in OUTS)


def test_the_symbol_the_wrapper_and_the_record_exist(built):
    """Fails on a library built without my-slam_amd/csrc/orbm_fuse.hip."""
    assert hasattr(C.CDLL(built.LIB_PATH), "orbm_fuse_views")
    assert hasattr(built.ORBmatcher, "fuse_views")
    assert built.FUSE_VIEW_DTYPE == FV.VIEW_DTYPE
    assert [built.ORBM_FUSE_MATCH, built.ORBM_FUSE_SKIPPED, built.ORBM_FUSE_BEHIND, built.ORBM_FUSE_OUT_IMAGE, built.ORBM_FUSE_DISTANCE,
            built.ORBM_FUSE_VIEW_ANGLE, built.ORBM_FUSE_UNDEFINED, built.ORBM_FUSE_NO_MATCH] == list(range(8))


def test_the_record_has_the_size_and_layout_of_the_c_struct(built, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbm.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(orbm_fuse_view),'
                   ' offsetof(orbm_fuse_view, bounds), offsetof(orbm_fuse_view, nlevels), offsetof(orbm_fuse_view, inv_level_sigma2),'
                   ' offsetof(orbm_fuse_view, grid), (int)ORBM_FUSE_NO_MATCH);return 0;}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    dt = built.FUSE_VIEW_DTYPE
    assert got == [dt.itemsize, dt.fields["bounds"][1], dt.fields["nlevels"][1], dt.fields["inv_level_sigma2"][1], dt.fields["grid"][1], 7]


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument gets its status and a text, and no output is written."""
    Lb = built.lib()

    def bad(mutate, text, code=built.ORBX_E_INVALID):
        _, b = _args()
        mutate(b)
        assert _call(Lb, b) == code and text in Lb.orbm_last_error(), Lb.orbm_last_error()
        assert _untouched(b)

    bad(lambda b: b.__setitem__("nviews", -1), b"nviews=-1")
    bad(lambda b: b.__setitem__("n_mp", -3), b"n_mp=-3")
    bad(lambda b: b["off"].__setitem__(0, 1), b"off[0]")
    bad(lambda b: b["off"].__setitem__(2, 0), b"off not monotone")
    bad(lambda b: b["views"]["nlevels"].__setitem__(1, 0), b"nlevels=0")
    bad(lambda b: b["views"]["nlevels"].__setitem__(3, 17), b"nlevels=17")
    bad(lambda b: b["views"]["grid"]["inv_w"].__setitem__(0, 0.0), b"cell sizes")
    bad(lambda b: b["views"]["grid"]["inv_h"].__setitem__(2, -1.0), b"cell sizes")
    bad(lambda b: b["views"]["grid"]["inv_h"].__setitem__(2, np.nan), b"cell sizes")
    for key in ("views", "off", "kps", "ur", "dk", "skip", "xw", "normal", "mf_max", "mf_min", "mp_desc") + OUTS:
        bad(lambda b: b.__setitem__(key, None), b"NULL")
    bad(lambda b: (b.__setitem__("nviews", 1 << 15), b.__setitem__("n_mp", (1 << 13) + 1)), b"2^28", built.ORBX_E_CAPACITY)
    bad(lambda b: b.__setitem__("nviews", 70000), b"65535 views", built.ORBX_E_CAPACITY)


def test_nothing_to_do_is_a_success_that_touches_nothing(built):
    Lb = built.lib()
    _, a = _args()
    for key in ("nviews", "n_mp"):
        b = dict(a)
        b[key] = 0
        assert _call(Lb, b) == built.ORBX_OK
        assert _untouched(b)
    assert Lb.orbm_fuse_views(None, None, 0, *([None] * 4), 0, *([None] * 6), C.c_float(3.0), *([None] * 8)) == built.ORBX_OK


def test_a_call_with_every_slot_skipped_is_answered_on_the_host(built):
    Lb = built.lib()
    _, a = _args()
    a["skip"][:] = 1
    assert _call(Lb, a) == built.ORBX_OK
    assert (a["status"] == FV.SKIPPED).all() and (a["bi"] == -1).all() and (a["bd"] == 256).all() and (a["nf"] == 0).all()
    assert all((a[k] == 0).all() for k in ("pu", "pv", "pr", "lv"))


def test_a_call_whose_views_are_all_empty_is_answered_on_the_host(built):
    """Not one key-frame feature: every window is empty, the projection half is the host's (the same arithmetic): statuses,
    projections and levels equal the numpy oracle bit for bit."""
    Lb = built.lib()
    sc, a = _args("mix-5")
    a["off"][:] = 0
    a["kps"] = a["ur"] = a["dk"] = None
    assert _call(Lb, a) == built.ORBX_OK
    seen = set()
    for k in range(sc.nviews):
        st, u, v, ur, lv, _ = FV.project(sc.views[k], a["skip"][k], sc.xw, sc.normal, sc.mf_max, sc.mf_min)
        assert np.array_equal(a["status"][k], st)
        for got, want in ((a["pu"][k], u), (a["pv"][k], v), (a["pr"][k], ur)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(a["lv"][k], lv)
        seen |= set(st.tolist())
    assert seen == set(range(1, 8))                                      # every status but MATCH
    assert (a["bi"] == -1).all() and (a["bd"] == 256).all() and (a["nf"] == 0).all()


def test_the_entry_point_fails_loudly_without_a_handle(built):
    import torch
    Lb = built.lib()
    _, a = _args()
    if torch.cuda.is_available():                                        # with a device the NULL handle is the caller's mistake
        assert _call(Lb, a) == built.ORBX_E_INVALID and b"NULL handle" in Lb.orbm_last_error()
    else:
        assert _call(Lb, a) == built.ORBX_E_HIP and b"no CPU path" in Lb.orbm_last_error()
    assert _untouched(a)                                                 # no half answer
