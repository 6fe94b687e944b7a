"""The planted fixtures of tests/window_cases.py on the CPU: the oracle returns, for every planted query, the answer written down
here by hand from the reference's lines (src/ORBmatcher.cc, src/KeyFrame.cc), and the fixtures meet their own preconditions:
  - the library's host helpers (ProjectPointsKF, ProjectPointsSim3, ProjectPoints, PredictScale) reproduce the planted u, v, level;
  - `use` is 1 wherever planned;
  - every distance that is not planted exceeds FAR = 120 (which covers the TH_LOW and ORBdist = 64 variants' 80 as well).
tests/test_window_cases_gpu.py then pins the library to the oracle on the same fixtures."""
import numpy as np
import pytest

import oracle_lib as O
import window_cases as WC

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------------------
# Part 1: hand answers per query: (Fuse, Fuse(Scw), SearchBySim3 1 -> 2); a tag names the planted key point, None = -1
# ---------------------------------------------------------------------------------------------------------------------------------
SAME = lambda t: (t, t, t)
HAND = {
    # (a) `dist<bestDist` is strict (:944, :1074, :1214, :1294): the first of two equal distances in vIndices order wins, whether the
    # two sit in one round of 64, in two rounds of a cell column, in two columns, in one lane, or (a5) where the second one's slot
    # in its round is lower than the first one's
    "a1": SAME("a1.first"), "a2": SAME("a2.first"), "a3": SAME("a3.first"), "a4": SAME("a4.first"), "a5": SAME("a5.first"),
    # (b) :911 / :1067 / :1207 `continue` before the distance: a first candidate on octave lv + 1 (b1) or lv - 2 (b2) keeps its place
    # in vIndices but never sets bestDist, so the second wins; b2's second sits on lv - 1, which is accepted
    "b1": SAME("b1.second"), "b2": SAME("b2.second"),
    # (c) lv - 1 accepted; lv = 0: octave 1 (10 bits) dropped, octave 0 (20 bits) wins; lv = 7: octave 5 (10) dropped, 6 (15) beats 7 (20)
    "c1": SAME("c1.only"), "c0": SAME("c0.on0"), "c7": SAME("c7.on6"),
    # (d) `bestDist<=TH_LOW` (:952, :1082) takes 50 and drops 51; `bestDist<=TH_HIGH` (:1221, :1301) takes 100 and drops 101
    "d50": SAME("d50.only"), "d51": (None, None, "d51.only"), "d100": (None, None, "d100.only"), "d101": SAME(None),
    # (e) KeyFrame.cc:601 `fabs(distx)<r`: |dx| == r = 8 is outside (the 10-bit candidate), the float below is inside (20 bits);
    # :574-588: the four early returns; a window clamped at the corner finds the key point of cell (0, 0);
    # Frame.cc:384 round(): the key point just below k + 0.5 lies in column k and precedes its twin of column k + 1 (rlo), the one
    # at k + 0.5 shares the twin's cell and follows it, having the higher index (rhi)
    "ex": SAME("ex.in"), "ey": SAME("ey.in"), "offl": SAME(None), "offr": SAME(None), "offt": SAME(None), "offb": SAME(None),
    "clamp": SAME("clamp.in"), "rlo": SAME("rlo.edge"), "rhi": SAME("rhi.right"),
    # (f) empty window (:894, :1053, :1193, :1273 `continue`), one member, every member on a wrong octave (bestDist stays 256 > TH), use = 0
    "empty": SAME(None), "one": SAME("one.only"), "none": SAME(None), "off": SAME(None), "off2": SAME(None),
    # (g) :925 `e2*mvInvLevelSigma2>7.8`, :936 `>5.99`: float product against a double literal, e2 == 1 so the product is the table
    # entry.  (float)5.99 < 5.99: kept; the next float: dropped; the float below (float)7.8: kept; (float)7.8 > 7.8: dropped;
    # er = 1 adds 1 to e2: 2 * 7.79.. > 7.8 dropped; u_right == 0.0 is stereo (`>=0` :914): 7.79.. kept where mono's 5.99 would drop.
    # A dropped near candidate (10 bits) leaves the far one (30 bits).  Fuse(Scw) and SearchBySim3 have no gate.
    "g599": SAME("g599.near"), "g599up": ("g599up.far", "g599up.near", "g599up.near"), "g78dn": SAME("g78dn.near"),
    "g78": ("g78.far", "g78.near", "g78.near"), "ger": ("ger.far", "ger.near", "ger.near"), "gzero": SAME("gzero.near"),
    # (h) the first of a tie dropped by the gate (e2 = 1 on the octave of the next float above 5.99), the second has e2 = 0.25
    "h": ("h.second", "h.first", "h.first"),
    # (i) :1310-1323: i1 -> i2 is kept only if i2 -> i1; cross: i2's MapPoint lands on another key point; nouse: i2 has none
    "cross": ("cross.only", "cross.only", None), "nouse": ("nouse.only", "nouse.only", None),
}


@pytest.fixture(scope="module", params=WC.KF_GRIDS)
def kf(request):
    return WC.kf_case(request.param)


def _want(fx, col):
    return np.array([-1 if HAND[n][col] is None else fx["idx"][HAND[n][col]] for n in fx["names"]], np.int32)


def test_kf_fixture_window(kf):
    """One window of at least 130 members in two cell columns, at least 65 of them in the first (rounds of 64 + a rest, then a fresh
    round), non-members in the same cells, and a candidate order that is not the index order -- on the oracle's features_in_area."""
    cl = kf["cluster"]
    og = O.KeyFrameGrid(kf["kps"], kf["grid"])
    order = og.features_in_area(cl["u"], cl["v"], cl["r"]).tolist()
    recs = cl["recs"]
    assert order == [c["i"] for c in recs] and len(order) >= 130
    assert order != sorted(order)
    colA, colB = cl["cols"]
    assert colA != colB and {c["col"] for c in recs} == {colA, colB}
    nA = sum(c["col"] == colA for c in recs)
    assert nA >= 65 and len(recs) - nA >= 32
    assert max(c["rnd"] for c in recs if c["col"] == colA) >= 1
    assert any(c["lane"] != p - c["before"] for p, c in enumerate(recs))       # non-members take lanes: lane != position % 64
    assert {int(kf["kps"]["octave"][c["i"]]) for c in recs} == {0, 1, 2, 3}    # members of every octave hold positions
    pos = cl["pos"]
    lane, rnd, col = (lambda p: recs[p]["lane"]), (lambda p: recs[p]["rnd"]), (lambda p: recs[p]["col"])
    for name in ("a1", "a2", "a3", "a4", "a5", "b1", "b2"):
        assert pos[name][0] < pos[name][1]
    p, q = pos["a1"]; assert (col(p), rnd(p)) == (col(q), rnd(q)) == (colA, 0) and lane(p) != lane(q)
    p, q = pos["a2"]; assert col(p) == col(q) == colA and (rnd(p), rnd(q)) == (0, 1)
    p, q = pos["a3"]; assert (col(p), col(q)) == (colA, colB)
    p, q = pos["a4"]; assert lane(p) == lane(q) and col(p) != col(q)
    p, q = pos["a5"]; assert cl["slotpos"](p) > cl["slotpos"](q)
    assert len({x for v in pos.values() for x in v}) == sum(len(v) for v in pos.values())


def test_kf_fixture_round_edge(kf):
    """The two `edge` key points straddle k + 0.5 of Frame::PosInGrid (src/Frame.cc:384) within one ulp."""
    amx, _, iw, _, _, _ = kf["grid"]
    x_lo, x_hi = kf["round_edge"]
    t = lambda x: F32(F32(x - F32(amx)) * F32(iw))
    assert x_hi == np.nextafter(x_lo, F32(np.inf)) and t(x_lo) < F32(20.5) <= t(x_hi)
    assert abs(float(t(x_lo)) - 20.5) <= float(np.spacing(F32(20.5))) and abs(float(t(x_hi)) - 20.5) <= float(np.spacing(F32(20.5)))
    assert kf["kps"]["x"][kf["idx"]["rlo.edge"]] == x_lo and kf["kps"]["x"][kf["idx"]["rhi.edge"]] == x_hi
    og = O.KeyFrameGrid(kf["kps"], kf["grid"])
    cs = np.ctypeslib.as_array(og.g.cell_start)
    col = lambda tag: int(np.searchsorted(cs, np.nonzero(og.items == kf["idx"][tag])[0][0], side="right") - 1) // 48
    assert col("rlo.edge") == 20 and col("rlo.right") == 21 and col("rhi.edge") == 21 and col("rhi.right") == 21      # roundf: half away from zero
    for name in ("rlo", "rhi"):
        assert kf["idx"][name + ".right"] < kf["idx"][name + ".edge"]


def test_kf_fixture_preconditions(kf, orbx):
    fx = kf
    M = orbx.ORBmatcher
    I4 = np.eye(4, dtype=F32)
    s = fx["small"]
    assert set(HAND) == set(fx["names"])
    assert [n for n, u in zip(fx["names"], fx["use"]) if not u] == ["off", "off2"]
    assert fx["use"][:4].tolist() == [1, 1, 0, 1]                              # unused entries interleaved with used ones
    # host helpers: the planted u, v and level, bit for bit, and ok everywhere
    u, v, iz, d3, ok = M.ProjectPointsKF(I4, WC.KID, WC.WIDE, fx["xw"], fx["normal"], np.zeros(3, F32))
    assert np.array_equal(u.view(np.uint32), fx["u"].view(np.uint32)) and np.array_equal(v.view(np.uint32), fx["v"].view(np.uint32))
    assert (iz == 1).all() and ok.all() and not (d3 < fx["min_inv"]).any() and not (d3 > fx["max_inv"]).any()
    assert np.array_equal(M.PredictScale(fx["mf_max"], d3, WC.LOGSF, WC.NLEV), fx["lv"])
    assert np.array_equal((u - F32(fx["bf"]) * iz).astype(F32), fx["u"] - F32(8))
    T, Ow = M.Sim3Decompose(I4)
    assert np.array_equal(T, I4) and not Ow.any()
    sR12, sR21, t21 = M.Sim3Relative(1.0, np.eye(3, dtype=F32), np.zeros(3, F32))
    assert np.array_equal(sR12, np.eye(3)) and np.array_equal(sR21, np.eye(3)) and not t21.any()
    for xw, mf, pu, pv, lv in ((fx["xw"], fx["mf_max"], fx["u"], fx["v"], fx["lv"]), (s["xw"], s["mf_max"], s["u"], s["v"], s["lv"])):
        u, v, d3, ok = M.ProjectPointsSim3(I4, sR21, t21, WC.KID, WC.WIDE, xw)
        assert np.array_equal(u.view(np.uint32), pu.view(np.uint32)) and np.array_equal(v.view(np.uint32), pv.view(np.uint32)) and ok.all()
        assert np.array_equal(M.PredictScale(mf, d3, WC.LOGSF, WC.NLEV), lv)
    # the gate's geometry is exact: ex == 1, ey == 0 and er == 0 (1 for `ger`), so that e2 * inv is the table entry itself
    kx, ky = fx["kps"]["x"], fx["kps"]["y"]
    for name in ("g599", "g599up", "g78dn", "g78", "ger", "gzero", "h"):
        q, j = fx["names"].index(name), fx["idx"][name + (".first" if name == "h" else ".near")]
        assert fx["u"][q] - kx[j] == 1 and fx["v"][q] - ky[j] == 0
        stereo = name in ("g78dn", "g78", "ger", "gzero")
        assert (fx["ur_kf"][j] >= 0) == stereo
        if stereo: assert (fx["u"][q] - F32(8)) - fx["ur_kf"][j] == (1 if name == "ger" else 0)
    assert fx["ur_kf"][fx["idx"]["gzero.near"]] == 0.0
    t = fx["inv_sigma2"]
    assert float(t[4]) < 5.99 < float(t[3]) and t[3] == np.nextafter(t[4], F32(9)) and float(t[6]) < 7.8 < float(t[7]) and t[6] == np.nextafter(t[7], F32(0))
    assert 2 * float(t[6]) > 7.8 and float(t[6]) > 5.99 and 0.25 * float(t[7]) < 5.99
    # window edges: |dx| == 8 exactly, and the float below
    q = fx["names"].index("ex")
    assert kx[fx["idx"]["ex.at"]] - fx["u"][q] == 8 and 0 < F32(8) - (kx[fx["idx"]["ex.in"]] - fx["u"][q]) < 1e-4
    q = fx["names"].index("ey")
    assert ky[fx["idx"]["ey.at"]] - fx["v"][q] == 8 and 0 < F32(8) - (ky[fx["idx"]["ey.in"]] - fx["v"][q]) < 1e-4
    # distances: the planted ones as planned, everything else beyond FAR
    D = WC.hamming(fx["qdesc"], fx["desc"])
    planted = np.zeros(D.shape, bool)
    for name, tag, d in fx["plants"]:
        assert D[fx["names"].index(name), fx["idx"][tag]] == d
        planted[fx["names"].index(name), fx["idx"][tag]] = True
    assert D[~planted].min() > WC.FAR
    # the reverse direction of SearchBySim3: distance 0 to the key point of the owning query, 128 to every other
    Ds = WC.hamming(s["mp_desc"][s["owner"] >= 0], s["desc"])
    own = s["owner"][s["owner"] >= 0]
    assert (Ds[np.arange(len(own)), own] == 0).all() and (np.sort(Ds, 1)[:, 1] > WC.FAR).all()
    nq1, nq2 = int(fx["use"].sum()), int(s["use"].sum())
    assert nq1 % 2 == 1 and nq2 % 2 == 1 and nq1 != nq2 and 190 <= len(fx["kps"]) <= 210


def test_kf_oracle_gives_the_hand_answers(kf):
    fx = kf
    bi, n = WC.oracle_fuse(fx)
    assert np.array_equal(bi, _want(fx, 0)) and n == int((bi >= 0).sum())
    bi, n = WC.oracle_fuse_sim3(fx)
    assert np.array_equal(bi, _want(fx, 1)) and n == int((bi >= 0).sum())
    m12, n = WC.oracle_sim3(fx, big_first=False)
    assert np.array_equal(m12, _want(fx, 2)) and n == int((m12 >= 0).sum())
    # the roles swapped: the planted search is the 2 -> 1 direction, match12 is indexed by the big frame's key points
    m21, n2 = WC.oracle_sim3(fx, big_first=True)
    want = np.full(len(fx["kps"]), -1, np.int32)
    want[m12[m12 >= 0]] = np.nonzero(m12 >= 0)[0]
    assert np.array_equal(m21, want) and n2 == n
    # subsets: 1, 4 and 5 usable queries (a full and a partial last group of four waves) answer as in the full set
    for k in (1, 4, 5):
        use = WC.kf_subset(fx, k)
        assert int(use.sum()) == k
        for col, fn in ((0, WC.oracle_fuse), (1, WC.oracle_fuse_sim3)):
            bi, n = fn(fx, use)
            assert np.array_equal(bi, np.where(use > 0, _want(fx, col), -1)) and n == int((bi >= 0).sum())
    # n1 = 5: the first five entries of the small frame (one of them unused)
    m5, n5 = WC.oracle_sim3(fx, big_first=False, n_small=5)
    assert np.array_equal(m5, _want(fx, 2)[:5]) and n5 == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# Part 2: the sequential scans
# ---------------------------------------------------------------------------------------------------------------------------------
def _distances_ok(fx):
    D = WC.hamming(fx["qdesc"], fx["desc"])
    for q, t, d in fx["plants"]:
        assert D[fx["names"].index(q), fx["tag"][t]] == d
    assert D[~fx["related"]].min() > WC.FAR
    return lambda q, t: int(D[fx["names"].index(q), fx["tag"][t]])


def _matches(fx, cm):
    inv = {v: k for k, v in fx["tag"].items()}
    return {inv[j]: fx["names"][q] for j, q in enumerate(cm) if q >= 0}


def test_sim3proj_case(orbx):
    """SearchByProjection(KeyFrame*, Scw, ...): :375 `if(vpMatched[idx]) continue`, :387 strict `<`, :394 `<=TH_LOW`, :396 the match
    blocks its slot for every later MapPoint."""
    fx = WC.sim3proj_case()
    d = _distances_ok(fx)
    assert (d("A", "s1"), d("B", "s1"), d("B", "s2"), d("C", "t1"), d("D", "t1"), d("D", "t2")) == (10, 12, 50, 10, 12, 51)
    u, v, iz, d3, ok = orbx.ORBmatcher.ProjectPointsKF(np.eye(4, dtype=F32), WC.KID, WC.WIDE, fx["xw"], fx["normal"], np.zeros(3, F32))
    assert np.array_equal(u, fx["u"]) and np.array_equal(v, fx["v"]) and ok.all()
    assert np.array_equal(orbx.ORBmatcher.PredictScale(fx["mf_max"], d3, WC.LOGSF, WC.NLEV), fx["lv"])
    assert fx["names"].index("A") < fx["names"].index("B") and fx["names"].index("C") < fx["names"].index("D")
    assert fx["tag"]["r0"] < fx["tag"]["r1"] < fx["tag"]["r2"]
    km, n, matched = WC.oracle_sim3proj(fx)
    # A takes s1 (10); B's best slot s1 (12) is taken, its next (50) is accepted; C takes t1, D's next (51) is not; E's best slot
    # p1 (5) was matched before the call, so p2 (20); F: r0 (5) is on octave 2 of a level-0 point, r1 and r2 tie at 15: the first;
    # X is not usable
    assert _matches(fx, km) == {"s1": "A", "s2": "B", "t1": "C", "p2": "E", "r1": "F"} and n == 5
    assert sorted(np.nonzero(matched)[0].tolist()) == sorted(fx["tag"][t] for t in ("s1", "s2", "t1", "p1", "p2", "r1"))


def test_init_case():
    """SearchForInitialization: :422 `if(level1>0) continue`, :444 `if(vMatchedDistance[i2]<=dist) continue`, :459-461 the ratio test,
    :463-467 the stolen match, :482 rotHist keeps i1 of a stolen match, :504 the cull checks `vnMatches12[idx1]>=0`, :513-517."""
    fx = WC.init_case()
    d = _distances_ok(fx)
    assert (d("A", "s"), d("B", "s"), d("C", "s1"), d("D", "s1"), d("D", "s2")) == (20, 15, 20, 20, 21)
    assert fx["nnratio"] == float(F32(0.5)) and fx["kps1"]["octave"][fx["names"].index("E")] == 1
    name = lambda m12: {fx["names"][i]: {v: k for k, v in fx["tag"].items()}[j] for i, j in enumerate(m12) if j >= 0}
    both = {"C": "s1",                 # 20, and nothing else in its window
            "R9": "R9.best",           # 9 < 20 * 0.5; R10: 10 < 10 fails; R11: 11 < 10 fails
            "B": "s",                  # 15 < A's 20: B takes s, A's entry is reset (:465), nmatches-- and ++
            "D": "s2",                 # s1 is skipped at :444 (20 <= 20), so it is neither best nor second: 21 alone passes the ratio test
            "b1_0": "b1_0.only", "b1_1": "b1_1.only", "b2_0": "b2_0.only", "b2_1": "b2_1.only"}
    # bins: 0 holds B, C, D, R9; 1 and 2 two each; 3 holds the stale entry of A (rot 90); 5 holds G.  The three maxima are 0, 1, 2.
    # Culling bin 3 finds vnMatches12[A] == -1 already: no second decrement.  Culling bin 5 drops G.
    m12, n, prev = WC.oracle_init(fx, True)
    assert name(m12) == both and n == 8
    for i, j in enumerate(m12):
        want = (fx["kps"]["x"][j], fx["kps"]["y"][j]) if j >= 0 else tuple(fx["prev"][i])
        assert tuple(prev[i]) == want and (j < 0 or want != tuple(fx["prev"][i]))
    m12, n, prev = WC.oracle_init(fx, False)
    assert name(m12) == dict(both, G="G.only") and n == 9


def test_last_case():
    """SearchByProjection(CurrentFrame, LastFrame, ...): :1385-1390 the three octave windows, :1404 `Observations()>0`, :1407 `>0`,
    :1411 `er>radius`, :1426 `<=TH_HIGH`, :1440 one rotHist entry per assignment, :1463 one decrement per entry."""
    fx = WC.last_case()
    d = _distances_ok(fx)
    assert (d("P", "s"), d("Q", "s"), d("P2", "s2"), d("Q2", "s2"), d("T100", "T100.only"), d("T101", "T101.only")) == (10, 11, 10, 11, 100, 101)
    ur, tag = fx["u_right"], fx["tag"]
    assert F32(500 - 16) - ur[tag["Uk.g"]] == F32(8) and F32(100 - 16) - ur[tag["Ud.g"]] > F32(8) and ur[tag["Uz.g"]] == 0
    for mode, octave in (("neither", 1), ("forward", 4), ("backward", 0)):
        xw, Tcw, Tlw = WC.last_pose(fx, mode)
        zc = np.array([O.lib().oro_gemm_row(O._p(Tcw.reshape(16)), 2, O._p(x)) for x in np.ascontiguousarray(xw)])
        assert (zc == 1).all()
        twc = O.camera_center(Tcw)
        assert {"neither": abs(twc[2]) <= fx["mb"], "forward": twc[2] > fx["mb"], "backward": -twc[2] > fx["mb"]}[mode]
        both = {"blk.x2": "blk",       # x1 (5 bits) holds a point with 2 observations
                "zero.z1": "zero",     # a point with 0 observations is overwritten
                "s": "Q",              # P (mp_obs 0) takes s, cur_obs stays 0, Q takes it again: two assignments
                "Uk.g": "Uk", "Ud.o": "Ud", "Uz.g": "Uz",      # er == radius kept; just above dropped (20 instead of 10); u_right 0 not gated
                "O.o%d" % octave: "O",                         # octaves [1, 3]: 15 on 1; >= 2: 20 on 4; [0, 2]: 10 on 0
                "T100.only": "T100"}
        both.update({"b%d_%d.only" % (b, k): "b%d_%d" % (b, k) for b in (1, 2) for k in range(3)})
        cm, n, cur_obs = WC.oracle_last(fx, mode, True)
        # bins: 0 holds nine entries (s twice), 1 and 2 three each, 5 holds P2 and Q2 on the one slot s2: two decrements
        assert _matches(fx, cm) == both and n == 15 and len(both) == 14
        assert cur_obs[tag["s2"]] == -1 and cur_obs[tag["s"]] == 0 and cur_obs[tag["zero.z1"]] == 3 and cur_obs[tag["blk.x1"]] == 2
        cm, n, cur_obs = WC.oracle_last(fx, mode, False)
        assert _matches(fx, cm) == dict(both, s2="Q2") and n == 17 and cur_obs[tag["s2"]] == 0


def test_map_case():
    """SearchByProjection(F, vpMapPoints, th): :88 `Observations()>0`, :91-94 the u_right gate, :118 `<=TH_HIGH`, :120 the ratio test
    on equal levels only, :133 `viewCos>0.998` against the double literal."""
    fx = WC.map_case()
    _distances_ok(fx)
    vc = fx["vc"][fx["names"].index("Vc")]
    assert float(vc) > 0.998 > float(np.nextafter(vc, F32(0)))           # (float)0.998 lies above 0.998: r = 2.5, its lower neighbour 4.0
    og = O.FrameGrid(fx["kps"], *WC.FRAME_BOUNDS)                        # level 0, th = 1: r = 2.5 * 1 misses the key point 3 px away, 4 * 1 holds it
    assert list(og.features_in_area(300.0, 100.0, 2.5, -1, 0)) == [] and list(og.features_in_area(300.0, 100.0, 4.0, -1, 0)) == [fx["tag"]["Vc.only"]]
    cm, n, cur_obs = WC.oracle_map(fx)
    # Req: 20 > 0.5 * 30 on equal levels: no match; Rdiff: the same distances on levels 1 and 0: matched.  The candidate 3 px away is
    # inside r = 4 (Vlo) and outside r = 2.5 (Vc, Vhi).  T100 in, T101 out.  XRk: er == 4 == r kept; XRd: just above, the 20-bit one wins.
    assert _matches(fx, cm) == {"Rdiff.best": "Rdiff", "Vlo.only": "Vlo", "T100.only": "T100", "XRk.g": "XRk", "XRd.o": "XRd", "Blk.free": "Blk"}
    assert n == 6 and cur_obs[fx["tag"]["Blk.taken"]] == 1
    assert all(cur_obs[j] == fx["mp_obs"][q] for j, q in enumerate(cm) if q >= 0)


def test_kfproj_case(orbx):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): :1528 levels lv - 1 .. lv + 1, :1541 the slot test, :1555
    `<=ORBdist`, :1577-1596 the cull resets the slot to NULL."""
    fx = WC.kfproj_case()
    _distances_ok(fx)
    u, v, iz, d3, inside = orbx.ORBmatcher.ProjectPoints(np.eye(4, dtype=F32), WC.KID, WC.WIDE, fx["xw"])
    assert np.array_equal(u, fx["u"]) and np.array_equal(v, fx["v"]) and inside.all()
    assert np.array_equal(orbx.ORBmatcher.PredictScale(fx["mf_max"], d3, WC.LOGSF, WC.NLEV), fx["lv"])
    both = {"Hblk.free": "Hblk", "T64.only": "T64",      # the 5-bit slot holds a point; 64 in, 65 out
            "Lv.o4": "Lv",             # level 3: octaves 1 (5 bits) and 5 (6 bits) are outside [2, 4]; 15 on 4 beats 20 on 2
            "Lv2.o2": "Lv2",           # octave 1 (5) outside, 20 on octave 2 = lv - 1 accepted
            "b1_0.only": "b1_0", "b1_1.only": "b1_1", "b2_0.only": "b2_0", "b2_1.only": "b2_1"}
    taken = fx["tag"]["Hblk.taken"]
    cm, n, has = WC.oracle_kfproj(fx, True)
    assert _matches(fx, cm) == both and n == 8
    assert sorted(np.nonzero(has)[0].tolist()) == sorted([taken] + [fx["tag"][t] for t in both]) and not has[fx["tag"]["Cull.only"]]
    cm, n, has = WC.oracle_kfproj(fx, False)
    assert _matches(fx, cm) == dict(both, **{"Cull.only": "Cull"}) and n == 9 and has[fx["tag"]["Cull.only"]]
