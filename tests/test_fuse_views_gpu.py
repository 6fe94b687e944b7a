"""orbm_fuse_views on the GPU against its oracles (tests/fuse_views_oracle.py), the planted fixtures (tests/fuse_views_cases.py) and
the existing per-view path.  Every comparison is exact: statuses, indices and distances equal, floats equal as bit patterns.  The
shapes are the smallest at which the kernels can go wrong (1 to 5 views; 1, 63, 64, 65, 200 MapPoints; views of 0, 1, 70 and
about 400 features); the oracle side of every scene is computed once per module."""
import ctypes as C

import numpy as np
import pytest

import fuse_views_cases as FC
import fuse_views_oracle as FV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(orbx):
    m = orbx.ORBmatcher(0.6, True, device=0, max_queries=256, max_train=512, max_pairs=4096)
    yield m
    m.close()


@pytest.fixture(scope="module")
def suite():
    """name -> (scene, its inputs before the loop, the snapshot from the oracles)"""
    out = {}
    for name in FV.SUITE:
        sc = FV.suite_scene(name)
        out[name] = (sc, sc.inputs(), FV.snapshot(sc))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what=""):
    """two results of fuse_views (or the oracle's first eight arrays), exactly"""
    for k, name in enumerate(("status", "best_idx", "best_dist")):
        assert np.array_equal(got[k], want[k]), "%s %s differs at %s" % (what, name, np.argwhere(got[k] != want[k])[:5].tolist())
    for k, name in ((3, "proj_u"), (4, "proj_v"), (5, "proj_ur")):
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s %s differs" % (what, name)
    assert np.array_equal(got[6], want[6]), "%s pred_level differs" % what
    assert np.array_equal(got[7], want[7]), "%s nfused differs" % what


@pytest.mark.parametrize("name", list(FV.SUITE))
def test_the_batch_equals_the_oracles(matcher, suite, name):
    """status, projection and level against the numpy restatement of :852-890, best_idx against the C oracle's Fuse per view,
    best_dist against the window loop on the C oracle's grid.  mix-5 is the one bulk scene (5 views x 200 points x up to 400
    features)."""
    sc, inp, dense = suite[name]
    got = matcher.fuse_views(*inp, th=sc.th)
    same(got, dense[:8], name)
    assert got[7].sum() == (got[0] == FV.MATCH).sum() and ((got[1] >= 0) == (got[0] == FV.MATCH)).all()
    again = matcher.fuse_views(*inp, th=sc.th)                              # and does not depend on the run
    same(again, got, name + " (second run)")


def existing_path(orbx, m, view, feat, skip, xw, normal, mf_max, mf_min, mp_desc, undefined, th):
    """The per-view path the adapter's single-key-frame Fuse takes: orbm_project_points_kf, the two distance getters and
    orbm_predict_scale on the host, orbm_grid_build_kf, orbm_fuse.  Slots the batch calls UNDEFINED are left out: the host's
    PredictScale converts a non-finite float to int there."""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = view["Rcw"].reshape(3, 3)
    T[:3, 3] = view["tcw"]
    K = tuple(float(view[k]) for k in ("fx", "fy", "cx", "cy"))
    u, v, iz, d3, ok = orbx.ORBmatcher.ProjectPointsKF(T, K, view["bounds"], xw, normal, view["Ow"])
    with np.errstate(all="ignore"):
        use = (skip == 0) & (ok != 0) & ~(d3 < np.float32(0.8) * mf_min) & ~(d3 > np.float32(1.2) * mf_max) & ~undefined
        ur = u - view["mbf"] * iz
    nl = int(view["nlevels"])
    lv = np.zeros(len(u), np.int32)
    lv[use] = orbx.ORBmatcher.PredictScale(mf_max[use], d3[use], float(view["log_scale_factor"]), nl)
    if len(feat) == 0:
        return np.full(len(u), -1, np.int32)
    m.grid_build_kf(feat.kps, FV.grid_tuple(view))
    return m.Fuse(use, u, v, ur, lv, mp_desc, view["scale_factors"][:nl], view["inv_level_sigma2"][:nl], feat.kps, feat.u_right, feat.desc, th)[0]


@pytest.mark.parametrize("name", ["mix-5", "n64-4", "skipview-3"])
def test_the_batch_equals_the_existing_per_view_path(orbx, matcher, suite, name):
    sc, inp, _ = suite[name]
    got = matcher.fuse_views(*inp, th=sc.th)
    skip, mp_desc = inp[5], inp[10]
    for k in range(sc.nviews):
        bi = existing_path(orbx, matcher, sc.views[k], sc.feats[k], skip[k], sc.xw, sc.normal, sc.mf_max, sc.mf_min, mp_desc,
                           got[0][k] == FV.UNDEFINED, sc.th)
        assert np.array_equal(bi, got[1][k]), "view %d: best_idx differs at %s" % (k, np.flatnonzero(bi != got[1][k])[:5])


def subset(inp, order):
    """the inputs with the views `order` only, in that order"""
    views, off, kps, ur, dk, skip = inp[:6]
    sl = [slice(int(off[v]), int(off[v + 1])) for v in order]
    noff = np.zeros(len(order) + 1, np.int32)
    noff[1:] = np.cumsum([s.stop - s.start for s in sl])
    cat = lambda a: np.concatenate([a[s] for s in sl]) if sl else a[:0]
    return (views[order], noff, cat(kps), cat(ur), cat(dk), skip[order]) + tuple(inp[6:])


def test_a_view_does_not_depend_on_the_views_around_it(matcher, suite):
    sc, inp, _ = suite["mix-5"]
    whole = matcher.fuse_views(*inp, th=sc.th)
    for v in range(sc.nviews):
        alone = matcher.fuse_views(*subset(inp, [v]), th=sc.th)
        same(alone, [a[v:v + 1] for a in whole], "view %d alone" % v)
    order = [3, 0, 4, 2, 1]
    perm = matcher.fuse_views(*subset(inp, order), th=sc.th)
    same(perm, [a[order] for a in whole], "permuted")


@pytest.mark.parametrize("name", list(FC.cases()))
def test_the_planted_cases(matcher, name):
    c = FC.cases()[name]
    st, bi, bd, pu, pv, pr, lv, nf = matcher.fuse_views(*c.args(), th=c.th)
    assert st[0].tolist() == c.status.tolist()
    assert bi[0].tolist() == c.best_idx.tolist()
    assert bd[0].tolist() == c.best_dist.tolist()
    assert nf[0] == (c.status == FV.MATCH).sum()
    ost, u, v, ur, olv, _ = FV.project(c.view, c.skip[0], c.xw, c.normal, c.mf_max, c.mf_min)
    assert np.array_equal(bits(pu[0]), bits(u)) and np.array_equal(bits(pv[0]), bits(v)) and np.array_equal(bits(pr[0]), bits(ur))
    assert np.array_equal(lv[0], olv)


def test_all_planted_cases_as_one_batch(matcher):
    """the cases as views of one call: another camera, pyramid and feature count per view, padded to the longest MapPoint list"""
    cs = list(FC.cases().values())
    n = max(len(c.xw) for c in cs)
    # the MapPoint arrays are shared by all views of a call: one call per case shape would not test the batch.  So every view sees
    # the points of every case, and only the slots of its own case are not skipped
    xw = np.concatenate([c.xw for c in cs]); normal = np.concatenate([c.normal for c in cs])
    mf_max = np.concatenate([c.mf_max for c in cs]); mf_min = np.concatenate([c.mf_min for c in cs])
    mp_desc = np.concatenate([c.mp_desc for c in cs])
    start = np.cumsum([0] + [len(c.xw) for c in cs])
    skip = np.ones((len(cs), len(xw)), np.uint8)
    for k in range(len(cs)):
        skip[k, start[k]:start[k + 1]] = 0
    off = np.zeros(len(cs) + 1, np.int32)
    off[1:] = np.cumsum([len(c.kps) for c in cs])
    views = np.array([c.view for c in cs], FV.VIEW_DTYPE)
    st, bi, bd, *_ = matcher.fuse_views(views, off, np.concatenate([c.kps for c in cs]), np.concatenate([c.u_right for c in cs]),
                                        np.concatenate([c.desc_kf for c in cs]), skip, xw, normal, mf_max, mf_min, mp_desc, th=3.0)
    assert n >= 8
    for k, c in enumerate(cs):
        own = slice(start[k], start[k + 1])
        assert st[k, own].tolist() == c.status.tolist() and bi[k, own].tolist() == c.best_idx.tolist() and bd[k, own].tolist() == c.best_dist.tolist()
        rest = np.ones(len(xw), bool)
        rest[own] = False
        assert (st[k, rest] == FV.SKIPPED).all() and (bi[k, rest] == -1).all()


def test_the_handle_is_left_as_found(orbx, suite):
    """orbm_grid_count() and a following single-view Fuse are the same before and after batch calls, on a handle of its own: the
    first batch call allocates the batch storage, the second is several times larger and grows it; a failing call leaves its
    outputs untouched."""
    matcher = orbx.ORBmatcher(0.6, True, device=0, max_queries=256, max_train=512, max_pairs=4096)
    sc, inp, _ = suite["n64-4"]
    big, big_inp, _ = suite["mix-5"]
    c = FC.cases()["ties"]
    feat = c.features()
    nl = 8
    matcher.grid_build_kf(feat.kps, FV.grid_tuple(c.view))

    def single():
        lv = np.zeros(len(c.xw), np.int32)
        return matcher.Fuse(np.ones(len(c.xw), np.uint8), c.xw[:, 0], c.xw[:, 1], c.xw[:, 0], lv, c.mp_desc, c.view["scale_factors"][:nl],
                            c.view["inv_level_sigma2"][:nl], feat.kps, feat.u_right, feat.desc, 3.0)

    count = matcher.grid_count()
    before = single()
    assert count == len(feat) and before[0].tolist() == c.best_idx.tolist()
    got = matcher.fuse_views(*c.args(), th=c.th)                        # one view, three points: allocates the batch storage
    assert matcher.grid_count() == count and got[1][0].tolist() == c.best_idx.tolist()
    matcher.fuse_views(*big_inp, th=big.th)                             # five views, 200 points: the batch storage grows
    assert matcher.grid_count() == count
    after = single()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]

    # a failing call: off not monotone
    L = orbx.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    views, off, kps, ur, dk, skip, xw, normal, mf_max, mf_min, mp_desc = inp
    off = off.copy()
    off[2] = 0
    nv, n = sc.nviews, sc.n_mp
    outs = [np.full((nv, n), 77, t) for t in (np.uint8, np.int32, np.int32, np.float32, np.float32, np.float32, np.int32)] + [np.full(nv, 77, np.int32)]
    rc = L.orbm_fuse_views(matcher.h, p(views), nv, p(off), p(kps), p(ur), p(dk), n, p(skip), p(xw), p(normal), p(mf_max), p(mf_min), p(mp_desc),
                           C.c_float(3.0), *[p(o) for o in outs])
    assert rc == orbx.ORBX_E_INVALID and b"monotone" in L.orbm_last_error()
    assert all((o == 77).all() for o in outs)
    assert matcher.grid_count() == count
    matcher.close()
