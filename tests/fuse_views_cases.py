"""Planted one-view fixtures for orbm_fuse_views, with hand-derived answers (tests/test_fuse_views_cpu.py pins the oracles to the
answers, tests/test_fuse_views_gpu.py the library).

Exact projections, as in tests/window_cases.py: under the identity camera (fx = fy = 1, cx = cy = 0, Rcw = I, tcw = 0) the world
point (u, v, 1) has z = 1, invz = 1 and projects to exactly (u, v); ur = u - mbf.  normal = xw / |xw| passes the viewing-angle
test, mfMinDistance = 0 and mfMaxDistance = |xw| * 1.2**(l - 0.5) pass the distance gate and make PredictScale return
ceil(l - 0.5) = l.  The image is 640 x 480 with the grid over it: cells of 10 x 10 pixels, cell index = round(x / 10), so x in
[95, 105) is column 10.  On level l the window radius is 3 * 1.2**l.

Descriptors are window_cases.Book's: a MapPoint's is a Hadamard row (128 bits from any other), a planted feature's is that row with
d chosen bits flipped: its distance to its MapPoint is d and to any other MapPoint more than 120."""
import numpy as np

import fuse_views_oracle as FV
import window_cases as WC

f32 = np.float32
M, S, B, O_, D, A, U, N = FV.MATCH, FV.SKIPPED, FV.BEHIND, FV.OUT_IMAGE, FV.DISTANCE, FV.VIEW_ANGLE, FV.UNDEFINED, FV.NO_MATCH


def identity_view(mbf=0.0, bounds=None, **kw):
    v = FV.make_view(np.eye(3), (0.0, 0.0, 0.0), fx=1.0, fy=1.0, cx=0.0, cy=0.0, mbf=mbf, **kw)
    if bounds is not None:
        v["bounds"] = np.asarray(bounds, f32)              # the image bounds alone: the grid stays over 640 x 480
    return v


class Case:
    """points: (u, v, level, query id of the Book) or a dict with xw / normal / mf_max / mf_min / level overrides; features: (x, y,
    octave, u_right, descriptor bits).  expect: per point (status, best_idx, best_dist)."""

    def __init__(self, view, book, points, features, expect, oro=True, th=3.0):
        self.view, self.th, self.oro = view, th, oro
        n = len(points)
        self.xw, self.normal = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
        self.mf_max, self.mf_min = np.zeros(n, f32), np.zeros(n, f32)
        Q = book.queries()
        self.mp_desc = np.zeros((n, 32), np.uint8)
        for i, p in enumerate(points):
            if not isinstance(p, dict):
                p = dict(u=p[0], v=p[1], level=p[2], q=p[3])
            xw = np.asarray(p.get("xw", (p.get("u", 0.0), p.get("v", 0.0), 1.0)), f32)
            d = np.linalg.norm(xw.astype(np.float64))
            self.xw[i] = xw
            with np.errstate(all="ignore"):
                self.normal[i] = p.get("normal", (xw / d).astype(f32))
            self.mf_max[i] = p.get("mf_max", f32(d * 1.2 ** (p.get("level", 0) - 0.5)))
            self.mf_min[i] = p.get("mf_min", 0.0)
            self.mp_desc[i] = Q[p["q"]]
        self.kps = WC.kp_array([(x, y, o) for x, y, o, _, _ in features]) if features else np.zeros(0, FV.KP_DTYPE)
        self.u_right = np.array([r for _, _, _, r, _ in features], f32)
        self.desc_kf = WC.pack(np.stack([b for *_, b in features])) if features else np.zeros((0, 32), np.uint8)
        self.skip = np.zeros((1, n), np.uint8)
        self.status = np.array([e[0] for e in expect], np.uint8)
        self.best_idx = np.array([e[1] for e in expect], np.int32)
        self.best_dist = np.array([e[2] for e in expect], np.int32)

    def features(self):
        return FV.Features(self.view, self.kps, self.u_right, self.desc_kf)

    def args(self):
        """ORBmatcher.fuse_views' arguments"""
        return (np.array([self.view], FV.VIEW_DTYPE), np.array([0, len(self.kps)], np.int32), self.kps, self.u_right, self.desc_kf, self.skip,
                self.xw, self.normal, self.mf_max, self.mf_min, self.mp_desc)


def _gate_edge(view, x0, u, v, ur, kr, away):
    """The key point (x, v, octave 0, u_right kr) nearest to x0, moving `away` (+1 / -1) from u one float at a time, that is the last
    one inside its chi-square gate, and its neighbour, the first one outside: the gate value is the oracle's float arithmetic."""
    def value(x):
        k = WC.kp_array([(x, v, 0)])
        return FV.gate_value(view, FV.Features(view, k, np.array([kr], f32), np.zeros((1, 32), np.uint8)), 0, u, v, ur)
    x = f32(x0)
    e, lim = value(x)
    while float(e) > lim:
        x = np.nextafter(x, f32(u))
        e, lim = value(x)
    while float(value(np.nextafter(x, f32(u + away * 1e6)))[0]) <= lim:
        x = np.nextafter(x, f32(u + away * 1e6))
    out = np.nextafter(x, f32(u + away * 1e6))
    assert float(value(x)[0]) <= lim < float(value(out)[0])
    return float(x), float(out)


def cases():
    """name -> Case"""
    out = {}
    mono = -1.0

    # ---- ties: two candidates at the same distance; the first in the reference's order wins whatever its index
    b = WC.Book(1)
    q = [b.query() for _ in range(3)]
    feats = [(97.0, 100.0, 0, mono, b.plant(q[0], 20)), (94.0, 100.0, 0, mono, b.plant(q[0], 20)),       # columns 10 and 9: column 9 first
             (300.0, 97.0, 0, mono, b.plant(q[1], 20)), (300.0, 94.0, 0, mono, b.plant(q[1], 20)),       # rows 10 and 9 of column 30: row 9 first
             (500.0, 201.0, 0, mono, b.plant(q[2], 20)), (501.0, 200.0, 0, mono, b.plant(q[2], 20))]     # one cell: push_back order
    out["ties"] = Case(identity_view(), b, [(96.0, 100.0, 0, q[0]), (300.0, 96.0, 0, q[1]), (500.0, 200.0, 0, q[2])], feats,
                       [(M, 1, 20), (M, 3, 20), (M, 4, 20)])

    # ---- TH_LOW: 50 matches, 51 does not (and is still reported as the best distance)
    b = WC.Book(2)
    q = [b.query() for _ in range(2)]
    feats = [(100.0, 100.0, 0, mono, b.plant(q[0], 50)), (300.0, 100.0, 0, mono, b.plant(q[1], 51))]
    out["th_low"] = Case(identity_view(), b, [(100.5, 100.0, 0, q[0]), (300.5, 100.0, 0, q[1])], feats, [(M, 0, 50), (N, -1, 51)])

    # ---- KeyFrame::IsInImage is [min, max): u == mnMaxX and v == mnMaxY are out, u == mnMinX and v == mnMinY are in
    b = WC.Book(3)
    q = [b.query() for _ in range(4)]
    feats = [(1.0, 100.0, 0, mono, b.plant(q[1], 7)), (100.0, 1.0, 0, mono, b.plant(q[3], 9))]
    out["bounds"] = Case(identity_view(), b, [(640.0, 100.0, 0, q[0]), (0.0, 100.0, 0, q[1]), (100.0, 480.0, 0, q[2]), (100.0, 0.0, 0, q[3])],
                         feats, [(O_, -1, 256), (M, 0, 7), (O_, -1, 256), (M, 1, 9)])

    # ---- quirks of :856-:887.  z = +0: not < 0, invz = +inf, u = 0.1 * inf = +inf fails IsInImage.  z = -0 (tcw z = -0 as well, so
    # that the gemm keeps the sign): not < 0 either, invz = -inf, u = -0.1 * -inf = +inf.  A NaN normal: NaN < 0.5*dist is false.
    # mfMaxDistance inf / nan: the distance gate passes (every comparison with 1.2*nan is false, nothing exceeds inf) and log(inf),
    # log(nan) have no int.  mfMaxDistance 0: dist > 0.
    b = WC.Book(4)
    q = [b.query() for _ in range(8)]
    nan, inf = float("nan"), float("inf")
    feats = [(200.0, 100.0, 0, mono, b.plant(q[2], 11))]
    pts = [dict(xw=(0.1, 0.05, 0.0), normal=(0.0, 0.0, 1.0), mf_max=5.0, q=q[0]),
           dict(u=200.0, v=100.0, level=0, q=q[1], xw=(200.0, 100.0, -1.0)),
           dict(u=200.0, v=100.0, level=0, normal=(nan, 0.0, 1.0), q=q[2]),
           dict(u=200.0, v=100.0, level=0, mf_max=inf, q=q[3]),
           dict(u=200.0, v=100.0, level=0, mf_max=nan, q=q[4]),
           dict(u=200.0, v=100.0, level=0, mf_max=0.0, q=q[5]),
           dict(u=200.0, v=100.0, level=0, normal=(-0.89, -0.45, -0.0045), q=q[6]),
           dict(u=200.0, v=100.0, level=0, mf_max=1000.0, mf_min=900.0, q=q[7])]
    out["quirks"] = Case(identity_view(), b, pts, feats,
                         [(O_, -1, 256), (B, -1, 256), (M, 0, 11), (U, -1, 256), (U, -1, 256), (D, -1, 256), (A, -1, 256), (D, -1, 256)])
    b = WC.Book(5)
    q = [b.query()]
    v = identity_view()
    v["tcw"][2] = -0.0
    out["minus_zero"] = Case(v, b, [dict(xw=(-0.1, -0.2, -0.0), normal=(0.0, 0.0, 1.0), mf_max=5.0, q=q[0])], [], [(O_, -1, 256)])

    # ---- the octave window [level - 1, level]: level 0 takes octave 0 (and the -1 no extractor produces), the top level 6 and 7; a
    # quotient far above the pyramid is clamped to the top level.  Radius on level 7: 3 * 1.2**7 = 10.7
    b = WC.Book(6)
    q = [b.query() for _ in range(3)]
    feats = [(100.0, 100.0, 1, mono, b.plant(q[0], 5)), (101.0, 100.0, 0, mono, b.plant(q[0], 30)),
             (300.0, 100.0, 5, mono, b.plant(q[1], 5)), (301.0, 100.0, 6, mono, b.plant(q[1], 30)), (299.0, 100.0, 7, mono, b.plant(q[1], 31)),
             (500.0, 100.0, 7, mono, b.plant(q[2], 12)), (509.0, 100.0, 7, mono, b.plant(q[2], 3)), (511.0, 100.0, 7, mono, b.plant(q[2], 1))]
    pts = [(100.5, 100.0, 0, q[0]), (300.5, 100.0, 7, q[1]), dict(u=500.5, v=100.0, level=12, q=q[2])]
    # point 2: |dx| = 8.5 < 10.7 is in the window and passes the gate (72.25 / 1.2**14 = 5.63 <= 5.99); 10.5 is in the window but
    # 110.25 / 12.84 = 8.6 > 5.99
    out["levels"] = Case(identity_view(), b, pts, feats, [(M, 1, 30), (M, 3, 30), (M, 6, 3)])

    # ---- the chi-square gates, at their float edges: monocular 5.99 on dx alone, stereo 7.8 on the disparity alone (mbf = 40:
    # ur = u - 40).  Per gate one MapPoint whose only candidate is the last float inside, one whose only candidate is the first outside
    b = WC.Book(7)
    q = [b.query() for _ in range(4)]
    v = identity_view(mbf=40.0)
    mi, mo = _gate_edge(v, 100.0 + 2.4474, 100.0, 100.0, 60.0, mono, +1)
    feats = [(mi, 100.0, 0, mono, b.plant(q[0], 10)), (mo, 200.0, 0, mono, b.plant(q[1], 10))]      # the same u for both: the same bits
    # the stereo gate: x and y coincide, the edge is searched on u_right
    kr = f32(260.0 - 2.79285)
    def sval(r):
        k = WC.kp_array([(300.0, 100.0, 0)])
        return FV.gate_value(v, FV.Features(v, k, np.array([r], f32), np.zeros((1, 32), np.uint8)), 0, 300.0, 100.0, 260.0)
    while float(sval(kr)[0]) > 7.8:
        kr = np.nextafter(kr, f32(260.0))
    while float(sval(np.nextafter(kr, f32(0.0)))[0]) <= 7.8:
        kr = np.nextafter(kr, f32(0.0))
    si, so = float(kr), float(np.nextafter(kr, f32(0.0)))
    assert float(sval(f32(si))[0]) <= 7.8 < float(sval(f32(so))[0])
    feats += [(300.0, 100.0, 0, si, b.plant(q[2], 10)), (300.0, 200.0, 0, so, b.plant(q[3], 10))]
    pts = [(100.0, 100.0, 0, q[0]), (100.0, 200.0, 0, q[1]), (300.0, 100.0, 0, q[2]), (300.0, 200.0, 0, q[3])]
    out["gates"] = Case(v, b, pts, feats, [(M, 0, 10), (N, -1, 256), (M, 2, 10), (N, -1, 256)])
    out["gates"].edges = (mi, mo, si, so)

    # ---- a monocular key point next to a stereo one in the same window: the stereo one is nearer in Hamming distance but its
    # disparity is 30 pixels off (900 > 7.8), the monocular one passes 5.99
    b = WC.Book(8)
    q = [b.query()]
    v = identity_view(mbf=40.0)
    feats = [(100.0, 100.0, 0, 90.0, b.plant(q[0], 2)), (101.0, 100.0, 0, mono, b.plant(q[0], 25)), (100.0, 101.0, 0, 60.5, b.plant(q[0], 26))]
    out["mono_stereo"] = Case(v, b, [(100.0, 100.0, 0, q[0])], feats, [(M, 1, 25)])

    # ---- more than 64 items in one column of the window: window_walk takes two rounds, the winner sits in the second
    b = WC.Book(9)
    q = [b.query()]
    feats = [(100.0 + 0.02 * (k % 10), 100.0 + 0.02 * (k // 10), 0, mono, b.plant(q[0], 40)) for k in range(80)]
    feats[71] = feats[71][:4] + (b.plant(q[0], 17),)
    feats[75] = feats[75][:4] + (b.plant(q[0], 17),)       # a tie inside the second round: 71 is first
    out["two_rounds"] = Case(identity_view(), b, [(100.0, 100.0, 0, q[0])], feats, [(M, 71, 17)])

    # ---- a window that misses the grid: the image bounds reach to 1000, the grid to 640; cells 79.. do not exist
    b = WC.Book(10)
    q = [b.query()]
    feats = [(639.0, 100.0, 0, mono, b.plant(q[0], 3))]
    out["off_grid"] = Case(identity_view(bounds=(0.0, 1000.0, 0.0, 480.0)), b, [(800.0, 100.0, 0, q[0])], feats, [(N, -1, 256)])

    # ---- octaves outside the view's levels: 99 is outside every octave window; -1 is inside level 0's and is gated with level 0's
    # sigma (the clamp of include/orbm.h).  The C oracle indexes mvInvLevelSigma2 with the raw octave, so it is left out here.
    b = WC.Book(11)
    q = [b.query()]
    feats = [(100.0, 100.0, 99, mono, b.plant(q[0], 1)), (101.0, 100.0, -1, mono, b.plant(q[0], 8)), (100.0, 101.0, 0, mono, b.plant(q[0], 9))]
    out["octave_clamp"] = Case(identity_view(), b, [(100.0, 100.0, 0, q[0])], feats, [(M, 1, 8)], oro=False)
    return out
