"""One long-lived handle through a realistic mix of calls, every result against the oracle (not against a fresh handle).
The matcher handle carries its grid slots from call to call (only some calls rebuild them, workspace growth drops them); the
extractor handle carries its per-shape plan, a single-frame HIP graph per shape, per-chunk batch graphs, the clear-after-error
flag and options baked into the graphs.  Per-call parity is covered elsewhere; these tests catch state that one call leaves
behind for the next: (a) orbm_search_by_sim3 with nothing to search used to return early and keep an earlier call's grid, which
the adapter then relabelled as key frame 1's; (b) one small matcher through a thread's day of producers, consumers and non-grid
calls; (c) one extractor through shapes, options and errors, and a batch handle through chunk-graph replays."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_kf_matchers import BASE, FX, K, H, W, Scene, _kf_grid, _sim3

F32 = np.float32
GRID, BOUNDS = _kf_grid(False)
FBOUNDS = (0.0, float(W), 0.0, float(H))


@pytest.fixture(scope="module")
def sc(orbx, synth, tmp_path_factory):
    s = Scene(orbx, synth)
    s.fv = s.featvecs(orbx, tmp_path_factory.mktemp("voc"), 2)
    s.mirror = s.k[0].copy()                                   # key frame X: KF1 mirrored, same N and descriptors, other cells
    s.mirror["x"] = F32(W - 1) - s.k[0]["x"]
    s.g = [O.KeyFrameGrid(s.k[i], GRID) for i in (0, 1)]
    s.fg1 = O.FrameGrid(s.k[1], *FBOUNDS)
    return s


def _err(orbx, code, fn, *a):
    with pytest.raises(orbx.OrbxError) as e:
        fn(*a)
    assert e.value.code == code, str(e.value)


# ---- the calls of the key-frame matchers, each with its oracle twin (the set-ups of test_kf_matchers.py) ----
def _sim3_inputs(orbx, sc, n1=None):
    """SearchBySim3 on the true relative motion; n1 = (i, i + 1) keeps one feature of key frame 1"""
    rng = np.random.default_rng(12)
    R12, t12 = np.eye(3, dtype=F32), np.array([BASE, 0.0, 0.0], F32)
    usable = [(rng.random(len(sc.k[i])) < 0.85).astype(np.uint8) for i in (0, 1)]
    sR12, sR21, t21 = orbx.ORBmatcher.Sim3Relative(1.0, R12, t12)
    u1, v1, d1, ok1 = orbx.ORBmatcher.ProjectPointsSim3(sc.T[0], sR21, t21, K, BOUNDS, sc.xw[0])
    u2, v2, d2, ok2 = orbx.ORBmatcher.ProjectPointsSim3(sc.T[1], sR12, t12, K, BOUNDS, sc.xw[1])
    use1 = usable[0].astype(bool) & ok1.astype(bool) & ~(d1 < sc.min_inv[0]) & ~(d1 > sc.max_inv[0])
    use2 = usable[1].astype(bool) & ok2.astype(bool) & ~(d2 < sc.min_inv[1]) & ~(d2 > sc.max_inv[1])
    lv1 = orbx.ORBmatcher.PredictScale(sc.mf_max[0], d1, sc.logsf, 8); lv2 = orbx.ORBmatcher.PredictScale(sc.mf_max[1], d2, sc.logsf, 8)
    s1 = slice(*n1) if n1 else slice(None)
    hip = [use1[s1].astype(np.uint8), u1[s1], v1[s1], lv1[s1], sc.d[0][s1], use2.astype(np.uint8), u2, v2, lv2, sc.d[1],
           sc.k[0][s1], sc.d[0][s1], GRID, sc.sf, sc.k[1], sc.d[1], GRID, sc.sf, 7.5]
    side = lambda i, s, us, g: dict(usable=us[s], xw=sc.xw[i][s], min_inv=sc.min_inv[i][s], max_inv=sc.max_inv[i][s], mf_max=sc.mf_max[i][s],
                                    mp_desc=sc.d[i][s], Tw=sc.T[i], bounds=BOUNDS, sf=sc.sf, log_sf=sc.logsf, grid=g, desc=sc.d[i][s])
    g1 = O.KeyFrameGrid(sc.k[0][s1], GRID) if n1 else sc.g[0]
    return hip, (side(0, s1, usable[0], g1), side(1, slice(None), usable[1], sc.g[1]), K, 1.0, R12, t12, 7.5)


def _search_sim3(m, orbx, sc, n1=None, zero=None):
    """SearchBySim3 == oracle; zero = 1 / 2 empties that side's use, "n2" passes key frame 2 without features"""
    a, oa = _sim3_inputs(orbx, sc, n1)
    if zero == 1:
        a[0] = np.zeros_like(a[0]); oa[0]["usable"] = np.zeros_like(oa[0]["usable"])
    elif zero == 2:
        a[5] = np.zeros_like(a[5]); oa[1]["usable"] = np.zeros_like(oa[1]["usable"])
    elif zero == "n2":
        for i in (5, 6, 7, 8, 9, 14, 15):
            a[i] = a[i][:0]
    m12, nf = m.SearchBySim3(*a)
    if zero == "n2":
        assert nf == 0 and (m12 == -1).all()
    else:
        om12, onf = O.search_by_sim3(*oa)
        assert nf == onf and np.array_equal(m12, om12)
    searched = zero is None and a[0].any() and a[5].any()
    assert m.grid_count() == (len(a[10]) if searched else -1)
    return nf


def _fuse_sim3_kf1(m, orbx, sc, zero=False):
    """FuseSim3 of key frame 2's points into key frame 1 (its grid must be in the handle) == oracle"""
    u, v, iz, d3, ok = orbx.ORBmatcher.ProjectPointsKF(sc.T[0], K, BOUNDS, sc.xw[1], sc.normal[1], None)
    usable = np.zeros(len(sc.k[1]), np.uint8) if zero else np.ones(len(sc.k[1]), np.uint8)
    use = usable.astype(bool) & ok.astype(bool) & ~(d3 < sc.min_inv[1]) & ~(d3 > sc.max_inv[1])
    lv = orbx.ORBmatcher.PredictScale(sc.mf_max[1], d3, sc.logsf, 8)
    bi, nf = m.FuseSim3(use.astype(np.uint8), u, v, lv, sc.d[1], sc.sf, sc.k[0], sc.d[0], 4.0)
    obi, onf = O.fuse_sim3(usable, sc.xw[1], sc.normal[1], sc.min_inv[1], sc.max_inv[1], sc.mf_max[1], sc.d[1], np.eye(4, dtype=F32), K, BOUNDS,
                           sc.sf, sc.logsf, sc.g[0], sc.d[0], 4.0)
    assert nf == onf and np.array_equal(bi, obi)
    assert (nf == 0) if zero else (nf > 100)
    return nf


def _fuse(m, orbx, sc, pts=slice(None), kf=slice(None), zero=False):
    """Fuse of key frame 1's points (pts) into key frame 2 (the features kf; that grid must be in the handle) == oracle"""
    rng = np.random.default_rng(33)
    n2 = len(sc.k[1])
    T = sc.T[1]; Ow = O.camera_center(T); bf = F32(FX * BASE)
    usable = (rng.random(len(sc.k[0])) < 0.85).astype(np.uint8)[pts]
    if zero:
        usable[:] = 0
    ur_kf = np.full(n2, -1, F32)
    st = rng.random(n2) < 0.6
    ur_kf[st] = (sc.k[1]["x"] - bf / (sc.xw[1][:, 2] + T[2, 3]))[st].astype(F32)
    ur_kf = ur_kf[kf]
    xw, nrm, mn, mx, mf, d = sc.xw[0][pts], sc.normal[0][pts], sc.min_inv[0][pts], sc.max_inv[0][pts], sc.mf_max[0][pts], sc.d[0][pts]
    u, v, iz, d3, ok = orbx.ORBmatcher.ProjectPointsKF(T, K, BOUNDS, xw, nrm, Ow)
    use = usable.astype(bool) & ok.astype(bool) & ~(d3 < mn) & ~(d3 > mx)
    lv = orbx.ORBmatcher.PredictScale(mf, d3, sc.logsf, 8)
    bi, nf = m.Fuse(use.astype(np.uint8), u, v, (u - bf * iz).astype(F32), lv, d, sc.sf, sc.inv_sigma2, sc.k[1][kf], ur_kf, sc.d[1][kf], 3.0)
    og = sc.g[1] if kf == slice(None) else O.KeyFrameGrid(sc.k[1][kf], GRID)
    obi, onf = O.fuse(usable, xw, nrm, mn, mx, mf, d, T, Ow, K, float(bf), BOUNDS, sc.sf, sc.inv_sigma2, sc.logsf, og, ur_kf, sc.d[1][kf], 3.0)
    assert nf == onf and np.array_equal(bi, obi)
    return nf


def _proj_sim3(m, orbx, sc, zero=False):
    """SearchByProjection(KF, Scw) of key frame 1's points into key frame 2 (its grid in the handle) == oracle"""
    rng = np.random.default_rng(44)
    Scw = _sim3(1.0)
    usable = np.zeros(len(sc.k[0]), np.uint8) if zero else (rng.random(len(sc.k[0])) < 0.85).astype(np.uint8)
    matched0 = (rng.random(len(sc.k[1])) < 0.2).astype(np.uint8)
    ma, mb = matched0.copy(), matched0.copy()
    T, Ow = orbx.ORBmatcher.Sim3Decompose(Scw)
    u, v, iz, d3, ok = orbx.ORBmatcher.ProjectPointsKF(T, K, BOUNDS, sc.xw[0], sc.normal[0], Ow)
    use = usable.astype(bool) & ok.astype(bool) & ~(d3 < sc.min_inv[0]) & ~(d3 > sc.max_inv[0])
    lv = orbx.ORBmatcher.PredictScale(sc.mf_max[0], d3, sc.logsf, 8)
    km, nm = m.SearchByProjectionSim3(use.astype(np.uint8), u, v, lv, sc.d[0], sc.sf, sc.k[1], sc.d[1], ma, 10)
    okm, onm = O.search_by_projection_sim3(usable, sc.xw[0], sc.normal[0], sc.min_inv[0], sc.max_inv[0], sc.mf_max[0], sc.d[0], Scw, K, BOUNDS,
                                           sc.sf, sc.logsf, sc.g[1], sc.d[1], mb, 10)
    assert nm == onm and np.array_equal(km, okm) and np.array_equal(ma, mb)
    assert (nm == 0) if zero else (nm > 200)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) SearchBySim3 with nothing to search leaves no grid behind
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("empty", [1, 2, "n2"])
def test_search_by_sim3_with_nothing_to_search_leaves_no_grid(orbx, sc, empty):
    """X has key frame 1's N, so a stale grid of X passes every count check a later key-frame-1 search makes."""
    m = orbx.ORBmatcher(0.75, True, max_queries=4096, max_train=4096, max_pairs=1 << 21)
    n1 = len(sc.k[0])
    m.grid_build_kf(sc.mirror, GRID)
    assert m.grid_count() == n1
    assert _search_sim3(m, orbx, sc, zero=empty) == 0                 # nfound 0, every entry -1, grid_count() == -1
    _err(orbx, orbx.ORBX_E_INVALID, _fuse_sim3_kf1, m, orbx, sc)
    m.grid_build_kf(sc.k[0], GRID)
    _fuse_sim3_kf1(m, orbx, sc)


@pytest.mark.gpu
def test_search_by_sim3_leaves_key_frame_1_grid(orbx, sc):
    m = orbx.ORBmatcher(0.75, True, max_queries=4096, max_train=4096, max_pairs=1 << 21)
    m.grid_build_kf(sc.mirror, GRID)
    assert _search_sim3(m, orbx, sc) > 200                            # grid_count() == N1 afterwards
    _fuse_sim3_kf1(m, orbx, sc)                                # no rebuild: slot 1 is key frame 1's


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) one small matcher through the thread's day
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_matcher_through_a_mixed_sequence(orbx, sc):
    m = orbx.ORBmatcher(0.9, True, max_queries=64, max_train=64, max_pairs=256)      # small on purpose: it grows mid-sequence
    k0, d0, k1, d1 = sc.k[0], sc.d[0], sc.k[1], sc.d[1]
    n0, n1 = len(k0), len(k1)
    rng = np.random.default_rng(7)
    # windows around the last frame's keypoints, some without a level window
    x = (k0["x"] - 4 + rng.uniform(-3, 3, n0)).astype(F32); y = (k0["y"] + rng.uniform(-3, 3, n0)).astype(F32)
    r = (12.0 * sc.sf[k0["octave"]]).astype(F32)
    mn = np.maximum(k0["octave"] - 1, -1).astype(np.int32); mx = (k0["octave"] + 1).astype(np.int32)
    mn[::5] = -1; mx[::5] = -1

    def area(og):
        off, idx = m.GetFeaturesInArea(x, y, r, mn, mx)
        for i in range(0, n0, 7):
            assert np.array_equal(idx[off[i]:off[i + 1]], og.features_in_area(float(x[i]), float(y[i]), float(r[i]), int(mn[i]), int(mx[i]))), i
        return off, idx

    def best2_area(og, train):
        got = m.search_area_best2(d0, x, y, r, mn, mx, train)
        want = og.search_area_best2(d0, x, y, r, mn, mx, train)
        assert all(np.array_equal(p, q) for p, q in zip(got, want))
        return got

    def init():
        pa = np.ascontiguousarray(np.stack([k0["x"], k0["y"]], 1), F32); pb = pa.copy()
        m12, nm = m.SearchForInitialization(k0, d0, k1, d1, pa, 100)
        om12, onm = O.search_for_initialization(k0, d0, sc.fg1, d1, pb, 100, 0.9, True)
        assert nm == onm and np.array_equal(m12, om12) and np.array_equal(pa, pb) and nm > 50

    def dense(q, t, rows=None):
        got = m.best2(q, t)
        want = O.best2(q[:rows], t)
        assert all(np.array_equal(p[:rows], w) for p, w in zip(got, want))

    def bow(zero=False):
        fv = sc.fv
        mf, nm = m.SearchByBoW(k1, d1, fv[1], k0, d0, fv[0], np.zeros(n1, np.uint8) if zero else None)
        omf, onm = O.search_by_bow(d1, k1["angle"], fv[1], d0, k0["angle"], fv[0], 0.9, True, np.zeros(n1, np.uint8) if zero else None)
        assert nm == onm and np.array_equal(mf, omf) and (nm == 0 if zero else nm > 10)

    def proj_last(zero=False):
        has = np.zeros(n0, np.uint8) if zero else (np.random.default_rng(3).random(n0) < 0.85).astype(np.uint8)
        obs = np.random.default_rng(4).integers(0, 4, n0).astype(np.int32)
        cur0 = np.full(n1, -1, np.int32); cur0[::11] = 1
        ca, cb = cur0.copy(), cur0.copy()
        args = (has, sc.xw[0], d0, obs, k0, sc.T[1], sc.T[0], K, 0.54, 386.1448, FBOUNDS, sc.sf)
        cm, nm = m.SearchByProjectionLast(*args, k1, d1, ca, 15.0, True)
        ocm, onm = O.search_by_projection_last(*args, sc.fg1, d1, cb, 15.0, True, True)
        assert nm == onm and np.array_equal(cm, ocm) and np.array_equal(ca, cb) and (nm == 0 if zero else nm > 300)

    def proj_kf(zero=False):
        usable = np.zeros(n0, np.uint8) if zero else (np.random.default_rng(5).random(n0) < 0.8).astype(np.uint8)
        has0 = (np.random.default_rng(6).random(n1) < 0.15).astype(np.uint8)
        ha, hb = has0.copy(), has0.copy()
        u, v, iz, d3, inside = m.ProjectPoints(sc.T[1], K, FBOUNDS, sc.xw[0])
        lv = m.PredictScale(sc.mf_max[0], d3, sc.logsf, 8)
        use = (usable.astype(bool) & inside.astype(bool) & ~(d3 < sc.min_inv[0]) & ~(d3 > sc.max_inv[0])).astype(np.uint8)
        cm, nm = m.SearchByProjectionKF(use, u, v, lv, d0, k0["angle"], sc.sf, k1, d1, ha, 10.0, 100)
        ocm, onm = O.search_by_projection_kf(usable, sc.xw[0], sc.min_inv[0], sc.max_inv[0], sc.mf_max[0], d0, k0["angle"], sc.T[1], K, FBOUNDS,
                                             sc.sf, sc.logsf, sc.fg1, d1, hb, 10.0, 100, True)
        assert nm == onm and np.array_equal(cm, ocm) and np.array_equal(ha, hb) and (nm == 0 if zero else nm > 250)

    def proj_map(zero=False):
        g = np.random.default_rng(8)
        in_view = np.zeros(n0, np.uint8) if zero else (g.random(n0) < 0.8).astype(np.uint8)
        px = (k0["x"] - 4 + g.normal(0, 0.7, n0)).astype(F32); py = (k0["y"] + g.normal(0, 0.7, n0)).astype(F32)
        lv = np.clip(k0["octave"] + g.integers(0, 2, n0), 0, 7).astype(np.int32)
        vc = np.where(g.random(n0) < 0.5, 0.9985, 0.99).astype(F32)
        obs = g.integers(1, 5, n0).astype(np.int32)
        cur0 = np.full(n1, -1, np.int32); cur0[::9] = 2
        ca, cb = cur0.copy(), cur0.copy()
        cm, nm = m.SearchByProjectionMap(in_view, px, py, lv, vc, d0, obs, sc.sf, k1, d1, ca, 3.0)
        ocm, onm = O.search_by_projection_map(in_view, px, py, lv, vc, d0, obs, sc.sf, sc.fg1, d1, cb, 3.0, 0.9)
        assert nm == onm and np.array_equal(cm, ocm) and np.array_equal(ca, cb) and (nm == 0 if zero else nm > 50)

    def tri():
        has1 = (np.random.default_rng(9).random(n0) < 0.3).astype(np.uint8); has2 = (np.random.default_rng(10).random(n1) < 0.3).astype(np.uint8)
        ur1 = np.full(n0, -1, F32); ur2 = np.full(n1, -1, F32)
        Kinv = np.linalg.inv(np.array([[FX, 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]))
        F12 = (Kinv.T @ np.array([[0, 0, 0], [0, 0, -BASE], [0, BASE, 0]]) @ Kinv).astype(F32)
        Cw = O.camera_center(sc.T[0])
        a = (k0, d0, has1, ur1, sc.fv[0], k1, d1, has2, ur2, sc.fv[1], Cw, sc.T[1], K, F12, sc.sf, sc.sigma2, False)
        m12, nm = m.SearchForTriangulation(*a)
        om12, onm = O.search_for_triangulation(*a, True)
        assert nm == onm and np.array_equal(m12, om12) and nm > 30

    def bow_kf():
        v1 = (np.random.default_rng(11).random(n0) < 0.75).astype(np.uint8); v2 = (np.random.default_rng(12).random(n1) < 0.75).astype(np.uint8)
        m12, nm = m.SearchByBoWKF(k0, d0, sc.fv[0], v1, k1, d1, sc.fv[1], v2)
        om12, onm = O.search_by_bow_kf(d0, k0["angle"], v1, sc.fv[0], d1, k1["angle"], v2, sc.fv[1], 0.9, True)
        assert nm == onm and np.array_equal(m12, om12) and nm > 30

    # -- the frame grid: built once, consumed after non-grid calls in between
    m.grid_build(k1, *FBOUNDS)
    assert m.grid_count() == n1
    off, idx = area(sc.fg1)
    dense(d0, d1)
    bi, bd, sd = m.best2(d0, d1, off, idx)                      # CSR on the lists the grid gave
    obi, obd, osd = O.best2(d0, d1, off, idx)
    assert np.array_equal(bi, obi) and np.array_equal(bd, obd) and np.array_equal(sd, osd)
    bow()
    best2_area(sc.fg1, d1)                                      # the grid of four calls ago
    init()
    proj_last(); proj_kf(); proj_map()
    # -- a non-grid call that grows max_train drops the grid: the next frame search is refused, not answered from freed cells
    q = rng.integers(0, 256, (9000, 32), dtype=np.uint8); t = rng.integers(0, 256, (8300, 32), dtype=np.uint8)
    dense(q, t, 300)
    assert m.grid_count() == -1
    _err(orbx, orbx.ORBX_E_INVALID, init)
    _err(orbx, orbx.ORBX_E_INVALID, proj_last)
    m.grid_build(k1, *FBOUNDS)
    init()
    # -- zero queries / empty train side / nothing usable: zero matches, and the next call is still right
    e_off, e_idx = m.GetFeaturesInArea(x[:0], y[:0], r[:0], mn[:0], mx[:0])
    assert list(e_off) == [0] and len(e_idx) == 0
    e = m.search_area_best2(d0[:0], x[:0], y[:0], r[:0], mn[:0], mx[:0], d1)
    assert all(len(a) == 0 for a in e)
    e12, en = m.SearchForInitialization(k0[:0], d0[:0], k1, d1, np.zeros((0, 2), F32), 100)
    assert en == 0 and len(e12) == 0
    proj_last(zero=True); proj_kf(zero=True); proj_map(zero=True); bow(zero=True)
    area(sc.fg1)
    proj_map()
    # -- two frames with equal N one after the other: the mirrored frame, then frame 1 again
    fgm = O.FrameGrid(sc.mirror, *FBOUNDS)
    m.grid_build(sc.mirror, *FBOUNDS)
    assert m.grid_count() == n0
    best2_area(fgm, d0)
    m.grid_build(k0, *FBOUNDS)
    assert m.grid_count() == n0
    best2_area(O.FrameGrid(k0, *FBOUNDS), d0)
    m.grid_build(k1[:0], *FBOUNDS)                              # a frame without features
    assert m.grid_count() == 0
    best2_area(O.FrameGrid(k1[:0], *FBOUNDS), d1[:0])
    m.grid_build(k1, *FBOUNDS)
    proj_kf()
    # -- key-frame grids: Fuse, non-grid LocalMapping calls, then more consumers of the same grid
    m.grid_build_kf(k1, GRID)
    assert _fuse(m, orbx, sc) > 250
    tri(); bow_kf()
    _proj_sim3(m, orbx, sc)
    assert _fuse(m, orbx, sc, zero=True) == 0
    _proj_sim3(m, orbx, sc, zero=True)
    assert _fuse(m, orbx, sc, pts=slice(100, 101)) <= 1         # one MapPoint
    assert _fuse(m, orbx, sc) > 250
    # -- SearchBySim3 as the producer: key frame 1 in slot 1, no rebuild for the Fuse(Scw) that follows; then the empty cases
    assert _search_sim3(m, orbx, sc) > 200
    bow_kf()
    _fuse_sim3_kf1(m, orbx, sc)
    _fuse_sim3_kf1(m, orbx, sc, zero=True)
    assert _search_sim3(m, orbx, sc, zero=1) == 0
    _err(orbx, orbx.ORBX_E_INVALID, _fuse_sim3_kf1, m, orbx, sc)
    m.grid_build_kf(k0, GRID)
    _fuse_sim3_kf1(m, orbx, sc)
    # -- one-feature sides
    i1 = int(np.nonzero(_sim3_inputs(orbx, sc)[0][0])[0][0])   # a key-frame-1 feature whose MapPoint is searched
    _search_sim3(m, orbx, sc, n1=(i1, i1 + 1))                         # grid_count() == 1 afterwards
    m.grid_build_kf(k1[5:6], GRID)
    _fuse(m, orbx, sc, kf=slice(5, 6))                          # every point into a key frame of one feature
    assert m.grid_count() == 1
    m.grid_build_kf(k1, GRID)
    assert _fuse(m, orbx, sc) > 250


# ---------------------------------------------------------------------------------------------------------------------------------
# (b') the host-input staging: a fresh handle stages the inputs of its first call in a block of the call's own, so does the first
# call larger than any before it, and the calls after that go through the handle's pinned arena
# ---------------------------------------------------------------------------------------------------------------------------------
def _window_calls(m, orbx, sc, qstep, tstep):
    """The entry points that upload window queries, on every qstep-th feature of key frame 1 (the queries) against every tstep-th
    feature of key frame 2 (the train frame), each compared with the oracle.  Every call builds the grid it needs."""
    sub = lambda a, st: np.ascontiguousarray(a[::st])
    k0, d0, k1, d1 = sub(sc.k[0], qstep), sub(sc.d[0], qstep), sub(sc.k[1], tstep), sub(sc.d[1], tstep)
    xw, nrm, mfm, mni, mxi = (sub(a[0], qstep) for a in (sc.xw, sc.normal, sc.mf_max, sc.min_inv, sc.max_inv))
    n0, n1 = len(k0), len(k1)
    rng = np.random.default_rng(7)
    x = (k0["x"] - 4 + rng.uniform(-3, 3, n0)).astype(F32); y = (k0["y"] + rng.uniform(-3, 3, n0)).astype(F32)
    r = (12.0 * sc.sf[k0["octave"]]).astype(F32)
    mn = np.maximum(k0["octave"] - 1, -1).astype(np.int32); mx = (k0["octave"] + 1).astype(np.int32)
    mn[::5] = -1; mx[::5] = -1

    def frame_grid():
        m.grid_build(k1, *FBOUNDS)
        return O.FrameGrid(k1, *FBOUNDS)

    def area():
        fg = frame_grid()
        off, idx = m.GetFeaturesInArea(x, y, r, mn, mx)
        for i in range(0, n0, 3):
            assert np.array_equal(idx[off[i]:off[i + 1]], fg.features_in_area(float(x[i]), float(y[i]), float(r[i]), int(mn[i]), int(mx[i]))), i
        return int(off[-1])

    def best2_area():
        fg = frame_grid()
        skip = (np.random.default_rng(2).random(n1) < 0.1).astype(np.uint8)
        for sk in (None, skip):
            got = m.search_area_best2(d0, x, y, r, mn, mx, d1, sk)
            want = fg.search_area_best2(d0, x, y, r, mn, mx, d1, sk)
            assert all(np.array_equal(p, q) for p, q in zip(got, want))
        return int((got[0] >= 0).sum())

    def init():
        fg = frame_grid()
        pa = np.ascontiguousarray(np.stack([k0["x"], k0["y"]], 1), F32); pb = pa.copy()
        m12, nm = m.SearchForInitialization(k0, d0, k1, d1, pa, 100)
        om12, onm = O.search_for_initialization(k0, d0, fg, d1, pb, 100, 0.9, True)
        assert nm == onm and np.array_equal(m12, om12) and np.array_equal(pa, pb)
        return nm

    def proj_last():
        fg = frame_grid()
        has = (np.random.default_rng(3).random(n0) < 0.85).astype(np.uint8)
        obs = np.random.default_rng(4).integers(0, 4, n0).astype(np.int32)
        cur0 = np.full(n1, -1, np.int32); cur0[::11] = 1
        ca, cb = cur0.copy(), cur0.copy()
        args = (has, xw, d0, obs, k0, sc.T[1], sc.T[0], K, 0.54, 386.1448, FBOUNDS, sc.sf)
        cm, nm = m.SearchByProjectionLast(*args, k1, d1, ca, 15.0, True)
        ocm, onm = O.search_by_projection_last(*args, fg, d1, cb, 15.0, True, True)
        assert nm == onm and np.array_equal(cm, ocm) and np.array_equal(ca, cb)
        return nm

    def proj_kf():
        fg = frame_grid()
        usable = (np.random.default_rng(5).random(n0) < 0.8).astype(np.uint8)
        has0 = (np.random.default_rng(6).random(n1) < 0.15).astype(np.uint8)
        ha, hb = has0.copy(), has0.copy()
        u, v, iz, d3, inside = m.ProjectPoints(sc.T[1], K, FBOUNDS, xw)
        lv = m.PredictScale(mfm, d3, sc.logsf, 8)
        use = (usable.astype(bool) & inside.astype(bool) & ~(d3 < mni) & ~(d3 > mxi)).astype(np.uint8)
        cm, nm = m.SearchByProjectionKF(use, u, v, lv, d0, k0["angle"], sc.sf, k1, d1, ha, 10.0, 100)
        ocm, onm = O.search_by_projection_kf(usable, xw, mni, mxi, mfm, d0, k0["angle"], sc.T[1], K, FBOUNDS, sc.sf, sc.logsf, fg, d1, hb, 10.0,
                                             100, True)
        assert nm == onm and np.array_equal(cm, ocm) and np.array_equal(ha, hb)
        return nm

    def proj_map():
        fg = frame_grid()
        g = np.random.default_rng(8)
        in_view = (g.random(n0) < 0.8).astype(np.uint8)
        px = (k0["x"] - 4 + g.normal(0, 0.7, n0)).astype(F32); py = (k0["y"] + g.normal(0, 0.7, n0)).astype(F32)
        lv = np.clip(k0["octave"] + g.integers(0, 2, n0), 0, 7).astype(np.int32)
        vc = np.where(g.random(n0) < 0.5, 0.9985, 0.99).astype(F32)
        obs = g.integers(1, 5, n0).astype(np.int32)
        cur0 = np.full(n1, -1, np.int32); cur0[::9] = 2
        ca, cb = cur0.copy(), cur0.copy()
        cm, nm = m.SearchByProjectionMap(in_view, px, py, lv, vc, d0, obs, sc.sf, k1, d1, ca, 3.0)
        ocm, onm = O.search_by_projection_map(in_view, px, py, lv, vc, d0, obs, sc.sf, fg, d1, cb, 3.0, 0.9)
        assert nm == onm and np.array_equal(cm, ocm) and np.array_equal(ca, cb)
        return nm

    def proj_sim3():
        m.grid_build_kf(k1, GRID)
        kg = O.KeyFrameGrid(k1, GRID)
        Scw = _sim3(1.0)
        usable = (np.random.default_rng(44).random(n0) < 0.85).astype(np.uint8)
        matched0 = (np.random.default_rng(45).random(n1) < 0.2).astype(np.uint8)
        ma, mb = matched0.copy(), matched0.copy()
        T, Ow = orbx.ORBmatcher.Sim3Decompose(Scw)
        u, v, iz, d3, ok = orbx.ORBmatcher.ProjectPointsKF(T, K, BOUNDS, xw, nrm, Ow)
        use = usable.astype(bool) & ok.astype(bool) & ~(d3 < mni) & ~(d3 > mxi)
        lv = orbx.ORBmatcher.PredictScale(mfm, d3, sc.logsf, 8)
        km, nm = m.SearchByProjectionSim3(use.astype(np.uint8), u, v, lv, d0, sc.sf, k1, d1, ma, 10)
        okm, onm = O.search_by_projection_sim3(usable, xw, nrm, mni, mxi, mfm, d0, Scw, K, BOUNDS, sc.sf, sc.logsf, kg, d1, mb, 10)
        assert nm == onm and np.array_equal(km, okm) and np.array_equal(ma, mb)
        return nm

    return dict(area=area, best2_area=best2_area, init=init, proj_last=proj_last, proj_kf=proj_kf, proj_map=proj_map, proj_sim3=proj_sim3)


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["area", "best2_area", "init", "proj_last", "proj_kf", "proj_map", "proj_sim3"])
def test_first_call_then_larger_calls_on_one_handle(orbx, sc, call):
    """A thinned-out pair of frames first (a few KiB of inputs), then the whole frames twice: the full-size inputs are larger than
    the arena the first call asked for, so the second call stages them in a block of its own again and the third is the first to
    go through the arena.  All three against the oracle."""
    m = orbx.ORBmatcher(0.9, True, max_queries=64, max_train=64, max_pairs=256)
    _window_calls(m, orbx, sc, 30, 12)[call]()
    for _ in range(2):
        assert _window_calls(m, orbx, sc, 1, 1)[call]() > 50


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) one extractor through shapes, options and errors
# ---------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(img, mode):
    if mode not in _ORACLE:
        _ORACLE[mode] = O.Extractor(1000, blur_mode=mode)
    k, d, _ = _ORACLE[mode].extract(img)
    return k, d


def _same(got, img, mode):
    k, d = got
    ok, od = _oracle(img, mode)
    assert len(k) == len(ok) > 100 and k.tobytes() == ok.tobytes() and np.array_equal(d, od), (img.shape, mode)


def _raw(orbx, ex, img, cap):
    """orbx_extract with a caller capacity of its own; img None = the empty image"""
    kps = np.zeros(max(cap, 1), orbx.KP_DTYPE); desc = np.zeros((max(cap, 1), 32), np.uint8); n = C.c_int(-1)
    if img is None:
        rc = ex.L.orbx_extract(ex.h, None, 0, 0, 0, orbx._p(kps), orbx._p(desc), cap, C.byref(n))
    else:
        rc = ex.L.orbx_extract(ex.h, orbx._p(img), img.shape[1], img.shape[0], img.strides[0], orbx._p(kps), orbx._p(desc), cap, C.byref(n))
    return rc, n.value


@pytest.mark.gpu
def test_one_extractor_through_shapes_options_and_errors(orbx, synth):
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480)
    seed = iter(range(300, 400))
    img = lambda w=640, h=480: synth.texture(next(seed), w, h)
    for _ in range(3):                                          # plain, capture, replay
        a = img(); _same(ex(a), a, 0)
    a = img(322, 241); _same(ex(a), a, 0)
    for _ in range(2):                                          # plain (shape changed), then the graph captured before the change
        a = img(); _same(ex(a), a, 0)
    t26 = synth.texture(26, 640, 480)
    k0, d0 = _oracle(t26, 0); k1, d1 = _oracle(t26, 1)
    assert k0.tobytes() != k1.tobytes() or not np.array_equal(d0, d1)     # the image tells the two blur modes apart
    ex.set_blur_rounding(1)
    for _ in range(2):
        _same(ex(t26), t26, 1)
    ex.set_blur_rounding(0)
    _same(ex(t26), t26, 0)
    a = img()
    rc, n = _raw(orbx, ex, a, 10)
    assert rc == orbx.ORBX_E_CAPACITY
    a = img(); _same(ex(a), a, 0)
    _err(orbx, orbx.ORBX_E_SHAPE, ex, img(640, 481))
    a = img(); _same(ex(a), a, 0)
    assert _raw(orbx, ex, None, ex.cap) == (orbx.ORBX_OK, 0)
    a = img(); _same(ex(a), a, 0)
    a = img(); ex.extract_begin(a); _same(ex.extract_end(), a, 0)
    a = img(); _same(ex(a), a, 0)


@pytest.mark.gpu
def test_batch_extractor_through_chunk_graphs(orbx, synth):
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480, max_batch=4)
    ex.set_batch_chunk(2)
    seed = iter(range(400, 500))
    t26 = synth.texture(26, 640, 480)

    def batch(n, mode, first=None):
        imgs = [synth.texture(next(seed), 640, 480) for _ in range(n)]
        if first is not None:
            imgs[0] = first
        imgs = np.stack(imgs)
        for got, a in zip(ex.extract_batch(imgs), imgs):
            _same(got, a, mode)

    for n in (4, 4, 3, 1, 4):                                   # the second 4 replays the chunk graphs of the first
        batch(n, 0)
    ex.set_blur_rounding(1)
    batch(4, 1, t26); batch(4, 1, t26)
    ex.set_blur_rounding(0)
    batch(4, 0, t26)


@pytest.mark.gpu
def test_shape_refused_by_the_planner_then_the_old_shape(orbx, synth):
    """640x481 above is refused before planning; 120x400 is refused inside it (level 0's box is 88 wide and 368 high, the quadtree
    root count rounds to 0).  The handle must stay planned for 322x241: its tables, its resize modes, its graph."""
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480)
    seed = iter(range(500, 600))
    img = lambda w, h: synth.texture(next(seed), w, h)
    for _ in range(3):                                          # plain, capture, replay
        a = img(322, 241); _same(ex(a), a, 0)
    _err(orbx, orbx.ORBX_E_SHAPE, ex, img(120, 400))
    for _ in range(2):
        a = img(322, 241); _same(ex(a), a, 0)
    a = img(640, 480); _same(ex(a), a, 0)


@pytest.mark.gpu
def test_batch_extractor_across_a_shape_change(orbx, synth):
    """The repeat of each shape replays the chunk graphs captured by the call before it; a shape change rewrites the tables while
    chunk graphs of the other shape exist."""
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480, max_batch=4)
    ex.set_batch_chunk(2)
    seed = iter(range(600, 700))
    for w, h in ((322, 241), (322, 241), (640, 480), (640, 480), (322, 241), (322, 241)):
        imgs = np.stack([synth.texture(next(seed), w, h) for _ in range(4)])
        for got, a in zip(ex.extract_batch(imgs), imgs):
            _same(got, a, 0)


@pytest.mark.gpu
def test_tile_switch_across_a_shape_change(orbx, synth, monkeypatch):
    """ORBX_PYRAMID_TILES on one handle through 640x480, 322x241, 640x480: a tile plan left over from the other shape would show
    in the upper pyramid levels."""
    monkeypatch.setenv("ORBX_PYRAMID_TILES", "2,32,32,1")
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480)
    opyr = O.Extractor(1000)
    for i, (w, h) in enumerate(((640, 480), (322, 241), (640, 480))):
        a = synth.texture(700 + i, w, h)
        ex(a)
        for l, (got, want) in enumerate(zip(ex.image_pyramid(), opyr.pyramid(a))):
            assert np.array_equal(got, want), "call %d (%dx%d): level %d differs" % (i, w, h, l)


@pytest.mark.gpu
def test_extractor_lifecycle_repeats(orbx, synth):
    """Three create .. destroy cycles of one batch handle through everything it owns lazily: the chunk graphs and chunk events, the
    colour blocks, the profiling ring, the pyramid download staging, the staging threads.  Every result against the oracle."""
    import gray_oracle as G
    W, Hh, B = 322, 241, 4
    grey = [np.stack([synth.texture(800 + 4 * i + k, W, Hh) for k in range(B)]) for i in range(4)]
    colour = [np.ascontiguousarray(np.stack([g, np.roll(g, 37, axis=2), 255 - g], -1)) for g in grey[:2]]
    opyr = O.Extractor(1000)
    for cycle in range(3):
        ex = orbx.ORBextractor(1000, max_width=W, max_height=Hh, max_batch=B)
        ex.set_batch_chunk(1)
        for imgs in grey[:3]:                                   # plain, chunk-graph capture, replay
            for got, a in zip(ex.extract_batch(imgs), imgs):
                _same(got, a, 0)
        ex.set_input_format(orbx.ORBX_FMT_BGR8)
        for imgs in colour:                                     # capture in the new format, replay
            for got, a in zip(ex.extract_batch(imgs), imgs):
                _same(got, G.to_gray(a, G.FMT_BGR8), 0)
        ex.set_input_format(orbx.ORBX_FMT_GRAY8)
        ex.set_profiling(2)
        for got, a in zip(ex.extract_batch(grey[3]), grey[3]):  # the call waits for its stream: the ring can be read
            _same(got, a, 0)
        ms = ex.stage_ms_ring()
        assert ms.shape == (1, 4) and np.isfinite(ms).all() and (ms > 0).all(), (cycle, ms)
        ex.set_profiling(0)
        for l, (got, want) in enumerate(zip(ex.image_pyramid_all(border=0), opyr.pyramid(grey[3][0]))):
            assert np.array_equal(got, want), "cycle %d: level %d differs" % (cycle, l)
        ex.close()
