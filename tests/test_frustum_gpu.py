"""orbm_frustum / orbm_frustum_device / orbm_search_local_points (include/orbm.h) on the GPU against tests/frustum_oracle.py:
statuses with ==, the four floats as bit patterns, levels and nToMatch; the fused call against the oracle's frustum followed by
the C oracle's SearchByProjection(F, vpMapPoints, th), and against the library's own two calls; the handle's grid and a
neighbouring call's results after each call."""
import numpy as np
import pytest

import frustum_oracle as F
import oracle_lib as O

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


def same_frustum(got, want, what=""):
    names = ("status", "proj_x", "proj_y", "proj_xr", "pred_level", "view_cos")
    for name, g, w in zip(names, got[:6], want[:6]):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype == np.float32:                           # bit patterns; IEEE 754 leaves sign and payload of a NaN open: any NaN equals any NaN
            g, w = np.where(np.isnan(g), np.uint32(0x7FC00000), g.view(np.uint32)), np.where(np.isnan(w), np.uint32(0x7FC00000), w.view(np.uint32))
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s %s: %d differ, first at %d: %s != %s" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]])
    assert got[6] == want[6], what


@pytest.mark.parametrize("k", range(len(F.SUITE)))
@pytest.mark.parametrize("limit", [0.5, 0.9])
def test_frustum_equals_oracle_on_the_suite(m, k, limit):
    """mono, stereo, a camera looking away, other calibrations and level counts, mfLogScaleFactor = 0; viewingCosLimit 0.5 as
    Tracking passes it, and a stricter one"""
    sc = F.suite_scene(k)
    want = F.frustum(*sc.args(), limit)
    got = m.frustum(*sc.args(), limit)
    same_frustum(got, want, "scene %d" % k)
    out = got[0] != F.IN_VIEW
    assert not (got[1][out].any() or got[2][out].any() or got[3][out].any() or got[4][out].any() or got[5][out].any())


def test_every_status_occurs_on_the_gpu(m):
    seen = np.zeros(8, int)
    for k in range(len(F.SUITE)):
        seen += np.bincount(m.frustum(*F.suite_scene(k).args(), 0.5)[0], minlength=8)
    assert (seen >= 20).all(), dict(zip(F.STATUS_NAMES, seen))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000])
def test_wave_edges(m, n):
    sc = F.make_scene(np.random.default_rng(100 + n), max(n, 1)).head(n)
    same_frustum(m.frustum(*sc.args(), 0.5), F.frustum(*sc.args(), 0.5), "n=%d" % n)


def test_more_points_than_the_handle_holds(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        for n in (1000, 9000, 300):
            sc = F.make_scene(np.random.default_rng(n), n)
            same_frustum(h.frustum(*sc.args(), 0.5), F.frustum(*sc.args(), 0.5), "n=%d" % n)
    finally:
        h.close()


def test_quirks_on_the_gpu(m):
    for name, (sc, limit, want) in F.quirk_cases().items():
        got = m.frustum(*sc.args(), limit)
        same_frustum(got, F.frustum(*sc.args(), limit), name)
        assert list(got[0]) == want, name


def test_ceil_boundary_on_the_gpu(m):
    for sc, _ in F.ceil_boundary_scenes():
        same_frustum(m.frustum(*sc.args(), 0.5), F.frustum(*sc.args(), 0.5), "scale factor %s" % sc.view["scale_factors"][1])


def test_device_pointer_form_gives_the_same_bits(m, orbx):
    import torch
    sc = F.suite_scene(0)
    n = len(sc)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_view, d_skip, d_xw, d_n, d_max, d_min = (t(np.asarray(a)) for a in (np.array([sc.view]), sc.skip, sc.xw, sc.normal, sc.mf_max, sc.mf_min))
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_f = [torch.full((n,), 7.0, dtype=torch.float32, device=dev) for _ in range(4)]
    d_lv = torch.full((n,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    m.frustum_device(d_view.data_ptr(), n, d_skip.data_ptr(), d_xw.data_ptr(), d_n.data_ptr(), d_max.data_ptr(), d_min.data_ptr(), 0.5,
                     d_st.data_ptr(), d_f[0].data_ptr(), d_f[1].data_ptr(), d_f[2].data_ptr(), d_lv.data_ptr(), d_f[3].data_ptr(),
                     stream.cuda_stream)
    stream.synchronize()
    want = F.frustum(*sc.args(), 0.5)
    got = (d_st.cpu().numpy(), d_f[0].cpu().numpy(), d_f[1].cpu().numpy(), d_f[2].cpu().numpy(), d_lv.cpu().numpy(), d_f[3].cpu().numpy(), want[6])
    same_frustum(got, want, "device form")
    m.frustum_device(None, 0, *([None] * 5), 0.5, *([None] * 6))          # n == 0: nothing is read
    with pytest.raises(orbx.OrbxError) as e:
        m.frustum_device(d_view.data_ptr() + 1, n, d_skip.data_ptr(), d_xw.data_ptr(), d_n.data_ptr(), d_max.data_ptr(), d_min.data_ptr(), 0.5,
                         d_st.data_ptr(), d_f[0].data_ptr(), d_f[1].data_ptr(), d_f[2].data_ptr(), d_lv.data_ptr(), d_f[3].data_ptr())
    assert e.value.code == orbx.ORBX_E_INVALID


# ---- the fused call

def _bounds(sc):
    return tuple(float(b) for b in sc.view["bounds"])


def _oracle_search(sc, fr, th, nnratio, limit=0.5):
    """the oracle's frustum, then ORBmatcher::SearchByProjection(F, vpMapPoints, th) on the C oracle"""
    want = F.frustum(*sc.args(), limit)
    stereo = sc.view["mbf"] > 0
    cur = fr.cur_obs.copy()
    cm, nm = np.full(len(fr.kps), -1, np.int32), 0
    if want[6] > 0:                                                     # src/Tracking.cc:1189
        og = O.FrameGrid(fr.kps, *_bounds(sc))
        cm, nm = O.search_by_projection_map((want[0] == F.IN_VIEW).astype(np.uint8), want[1], want[2], want[4], want[5], fr.mp_desc, fr.mp_obs,
                                            sc.view["scale_factors"][:int(sc.view["nlevels"])], og, fr.desc, cur, th, nnratio,
                                            want[3] if stereo else None, fr.u_right if stereo else None)
    return want, cur, cm, nm


def _fused(m, sc, fr, th, limit=0.5):
    cur = fr.cur_obs.copy()
    m.grid_build(fr.kps, *_bounds(sc))
    out = m.search_local_points(*sc.args(), fr.mp_desc, fr.mp_obs, fr.kps, fr.desc, cur, th, fr.u_right if sc.view["mbf"] > 0 else None, limit)
    return out, cur


def _two_calls(m, sc, fr, th, limit=0.5):
    """what the library offered before: orbm_frustum, its outputs on the host, orbm_search_by_projection_map"""
    cur = fr.cur_obs.copy()
    stereo = sc.view["mbf"] > 0
    fo = m.frustum(*sc.args(), limit)
    cm, nm = np.full(len(fr.kps), -1, np.int32), 0
    if fo[6] > 0:
        m.grid_build(fr.kps, *_bounds(sc))
        cm, nm = m.SearchByProjectionMap((fo[0] == F.IN_VIEW).astype(np.uint8), fo[1], fo[2], fo[4], fo[5], fr.mp_desc, fr.mp_obs,
                                         sc.view["scale_factors"][:int(sc.view["nlevels"])], fr.kps, fr.desc, cur, th,
                                         fo[3] if stereo else None, fr.u_right if stereo else None)
    return fo, cur, cm, nm


@pytest.mark.parametrize("k,th", [(0, 1.0), (0, 3.0), (0, 5.0), (1, 1.0), (1, 3.0), (2, 5.0), (3, 3.0), (4, 1.0), (5, 5.0)])
def test_search_local_points_equals_the_oracle_and_the_two_calls(m, k, th):
    """stereo frames with a stereo u_right, mono frames, occupied slots, th 1 / 3 / 5; scene 4 has nToMatch == 0"""
    sc = F.suite_scene(k)
    fr = F.make_frame(np.random.default_rng(50 + k), sc)
    want, wcur, wcm, wnm = _oracle_search(sc, fr, th, 0.8)
    out, cur = _fused(m, sc, fr, th)
    same_frustum(out, want, "scene %d" % k)
    assert out[8] == wnm and np.array_equal(out[7], wcm) and np.array_equal(cur, wcur)
    fo, tcur, tcm, tnm = _two_calls(m, sc, fr, th)
    same_frustum(out, fo)
    assert out[8] == tnm and np.array_equal(out[7], tcm) and np.array_equal(cur, tcur)
    assert (fr.cur_obs > 0).any() and np.array_equal(cur[fr.cur_obs > 0], fr.cur_obs[fr.cur_obs > 0])     # occupied slots keep their point
    if k == 4:
        assert out[6] == 0 and out[8] == 0 and (out[7] == -1).all()
    if k in (0, 1) and th >= 3.0:
        assert out[8] > 300                                             # most visible points find their key point


def test_search_local_points_edges(m, orbx):
    sc = F.suite_scene(0)
    fr = F.make_frame(np.random.default_rng(9), sc)
    m.grid_build(fr.kps, *_bounds(sc))
    e = sc.head(0)
    out = m.search_local_points(*e.args(), fr.mp_desc[:0], fr.mp_obs[:0], fr.kps, fr.desc, fr.cur_obs.copy(), 1.0, fr.u_right)
    assert out[6] == 0 and out[8] == 0 and (out[7] == -1).all()
    with pytest.raises(orbx.OrbxError) as ei:                           # another frame's grid in the handle
        m.search_local_points(*sc.args(), fr.mp_desc, fr.mp_obs, fr.kps[:-1], fr.desc[:-1], fr.cur_obs[:-1].copy(), 1.0, fr.u_right[:-1])
    assert ei.value.code == orbx.ORBX_E_INVALID
    for n in (1, 63, 64, 65):
        s = sc.head(n)
        f = F.FrameSide(fr.kps, fr.desc, fr.u_right, fr.cur_obs, fr.mp_desc[:n], fr.mp_obs[:n])
        want, wcur, wcm, wnm = _oracle_search(s, f, 3.0, 0.8)
        out, cur = _fused(m, s, f, 3.0)
        same_frustum(out, want, "n=%d" % n)
        assert out[8] == wnm and np.array_equal(out[7], wcm) and np.array_equal(cur, wcur)
    none = F.FrameSide(fr.kps[:0], fr.desc[:0], fr.u_right[:0], fr.cur_obs[:0], fr.mp_desc, fr.mp_obs)     # a frame without key points
    out = m.search_local_points(*sc.args(), none.mp_desc, none.mp_obs, none.kps, none.desc, none.cur_obs.copy(), 1.0, none.u_right)
    same_frustum(out, F.frustum(*sc.args(), 0.5))
    assert out[8] == 0 and len(out[7]) == 0


def test_search_local_points_grows_a_small_handle(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=4096, max_pairs=256)
    try:
        sc = F.suite_scene(0)
        fr = F.make_frame(np.random.default_rng(77), sc)
        want, wcur, wcm, wnm = _oracle_search(sc, fr, 5.0, 0.8)
        out, cur = _fused(h, sc, fr, 5.0)
        same_frustum(out, want)
        assert out[8] == wnm and np.array_equal(out[7], wcm) and np.array_equal(cur, wcur)
        assert h.grid_count() == len(fr.kps)                            # growing queries and pairs keeps the grid
    finally:
        h.close()


def test_the_handle_keeps_its_grid_and_its_neighbours_results(m, orbx):
    """in the manner of test_handle_state_gpu.py: one handle, a neighbouring call before and after each of the three entry points"""
    sc = F.suite_scene(0)
    fr = F.make_frame(np.random.default_rng(31), sc)
    bounds = _bounds(sc)
    m.grid_build(fr.kps, *bounds)
    og = O.FrameGrid(fr.kps, *bounds)
    rng = np.random.default_rng(5)
    qx, qy = rng.uniform(0, bounds[1], 200).astype(f32), rng.uniform(0, bounds[3], 200).astype(f32)

    def neighbour():
        off, idx = m.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        for q in (0, 17, 199):
            assert np.array_equal(idx[off[q]:off[q + 1]], og.features_in_area(float(qx[q]), float(qy[q]), 25.0, 0, 3))
        return off, idx

    off0, idx0 = neighbour()
    want = F.frustum(*sc.args(), 0.5)
    same_frustum(m.frustum(*sc.args(), 0.5), want)
    assert m.grid_count() == len(fr.kps)
    off1, idx1 = neighbour()
    assert np.array_equal(off0, off1) and np.array_equal(idx0, idx1)
    cur = fr.cur_obs.copy()
    out = m.search_local_points(*sc.args(), fr.mp_desc, fr.mp_obs, fr.kps, fr.desc, cur, 3.0, fr.u_right)
    assert m.grid_count() == len(fr.kps)
    off2, idx2 = neighbour()
    assert np.array_equal(off0, off2) and np.array_equal(idx0, idx2)
    w, wcur, wcm, wnm = _oracle_search(sc, fr, 3.0, 0.8)
    assert out[8] == wnm and np.array_equal(out[7], wcm)
    big = F.make_scene(np.random.default_rng(8), 30000)                 # larger than the handle: the queries grow, the grid stays
    same_frustum(m.frustum(*big.args(), 0.5), F.frustum(*big.args(), 0.5))
    assert m.grid_count() == len(fr.kps)
    off3, idx3 = neighbour()
    assert np.array_equal(off0, off3) and np.array_equal(idx0, idx3)
    out2 = m.search_local_points(*sc.args(), fr.mp_desc, fr.mp_obs, fr.kps, fr.desc, fr.cur_obs.copy(), 3.0, fr.u_right)
    same_frustum(out2, out)
    assert out2[8] == out[8] and np.array_equal(out2[7], out[7])
