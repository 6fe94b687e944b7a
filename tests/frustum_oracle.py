"""Restatement in numpy of Frame::isInFrustum (src/Frame.cc:269-325 of WChen09/My-SLAM) with MapPoint::GetMin / MaxDistanceInvariance
and MapPoint::PredictScale (src/MapPoint.cc:373-383, :402-417), vectorised over the local MapPoints of Tracking::SearchLocalPoints
(src/Tracking.cc:1174-1187): the oracle of orbm_frustum (include/orbm.h).  Test infrastructure only.

float32 where the reference is float, float64 where OpenCV 3.1.0 works in double: mRcw*P+mtcw as cv::gemm's
small-matrix path, cv::norm and Mat::dot accumulated in double, double constants compared in double.  The logf of PredictScale is
the correctly rounded float function (x87 long double, rounded once).

Also here: frustum_f64, the same test written down naively in float64 with its margins to every gate, and the synthetic scenes
(camera, local map, current frame) the tests, the sweep and the bench tool feed to both sides."""
import numpy as np

f32, f64, ld = np.float32, np.float64, np.longdouble
MAX_LEVELS = 16

IN_VIEW, SKIPPED, BEHIND, OUT_X, OUT_Y, DISTANCE, VIEW_COS, UNDEFINED = range(8)
STATUS_NAMES = ["in_view", "skipped", "behind", "out_x", "out_y", "distance", "view_cos", "undefined"]

VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("mbf", "<f4"), ("bounds", "<f4", (4,)), ("log_scale_factor", "<f4"), ("nlevels", "<i4"),
                       ("scale_factors", "<f4", (MAX_LEVELS,))])
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])


def make_view(R, t, fx, fy, cx, cy, mbf, bounds, scale_factor=1.2, nlevels=8, Ow=None, log_scale_factor=None):
    """One orbm_frame_view block.  Ow = -Rcw^T tcw as Frame::UpdatePoseMatrices computes it (src/Frame.cc:266: cv::gemm's
    small-matrix path with alpha = -1); mfLogScaleFactor = log(mfScaleFactor) in float, mvScaleFactors as the extractor's
    constructor fills them."""
    v = np.zeros((), VIEW_DTYPE)
    R = np.asarray(R, f32).reshape(3, 3)
    t = np.asarray(t, f32).reshape(3)
    v["Rcw"] = R.reshape(9)
    v["tcw"] = t
    if Ow is None:
        with np.errstate(all="ignore"):
            Ow = [f32(f64((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) * -1.0 + 0.0) for k in range(3)]
    v["Ow"] = np.asarray(Ow, f32)
    v["fx"], v["fy"], v["cx"], v["cy"], v["mbf"] = f32(fx), f32(fy), f32(cx), f32(cy), f32(mbf)
    v["bounds"] = np.asarray(bounds, f32)
    v["log_scale_factor"] = f32(np.log(ld(f32(scale_factor)))) if log_scale_factor is None else f32(log_scale_factor)
    v["nlevels"] = nlevels
    sf = np.ones(MAX_LEVELS, f32)
    for i in range(1, min(nlevels, MAX_LEVELS)):
        sf[i] = sf[i - 1] * f32(scale_factor)
    v["scale_factors"] = sf
    return v


# ---- the arithmetic conventions

def _gemm_row(R, t, P):
    """cv::gemm's small-matrix path for one row of mRcw*P+mtcw: the float sum left to right, then (float)(t0*1 + c*1) in double"""
    t0 = (R[0] * P[:, 0] + R[1] * P[:, 1]) + R[2] * P[:, 2]
    return (t0.astype(f64) + f64(t)).astype(f32)


def _dot3(a, b):
    """Mat::dot / the squares of cv::norm: products and sum in double"""
    a, b = a.astype(f64), b.astype(f64)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def logf_cr(x):
    """the correctly rounded float logarithm of a float: long double, rounded once"""
    with np.errstate(all="ignore"):
        return np.log(np.asarray(x, f32).astype(ld)).astype(f32)


def predict_quotient(mf_max, dist, log_scale_factor):
    """log(ratio)/pF->mfLogScaleFactor of src/MapPoint.cc:407-410 before the ceil, in float"""
    with np.errstate(all="ignore"):
        ratio = np.asarray(mf_max, f32) / np.asarray(dist, f32)                     # :407
        return logf_cr(ratio) / f32(log_scale_factor)                              # :410


def predict_scale(mf_max, dist, log_scale_factor, nlevels):
    """MapPoint::PredictScale(dist, Frame*) -> (level, undefined): undefined where the int conversion of :410 is (the ceil is not
    finite or outside int); level is meaningless there"""
    with np.errstate(all="ignore"):
        c = np.ceil(predict_quotient(mf_max, dist, log_scale_factor))
        undefined = ~((c >= f32(-2147483648.0)) & (c < f32(2147483648.0)))
        level = np.where(undefined, 0, c).astype(np.int64)
    level = np.where(level < 0, 0, np.where(level >= nlevels, nlevels - 1, level))  # :411-414
    return level.astype(np.int32), undefined


def frustum(view, skip, xw, normal, mf_max, mf_min, viewing_cos_limit):
    """-> (status uint8, proj_x, proj_y, proj_xr float32, pred_level int32, view_cos float32, n_to_match): orbm_frustum's outputs"""
    V = view
    skip = np.asarray(skip, np.uint8)
    P = np.ascontiguousarray(xw, f32).reshape(-1, 3)
    Pn = np.ascontiguousarray(normal, f32).reshape(-1, 3)
    mf_max, mf_min = np.asarray(mf_max, f32), np.asarray(mf_min, f32)
    n = len(P)
    R, t, Ow, b = V["Rcw"], V["tcw"], V["Ow"], V["bounds"]
    with np.errstate(all="ignore"):
        PcX, PcY, PcZ = _gemm_row(R[0:3], t[0], P), _gemm_row(R[3:6], t[1], P), _gemm_row(R[6:9], t[2], P)     # :277
        behind = PcZ < f32(0)                                                       # :283
        invz = f32(1) / PcZ                                                         # :287
        u = V["fx"] * PcX * invz + V["cx"]                                          # :288
        v = V["fy"] * PcY * invz + V["cy"]                                          # :289
        out_x = (u < b[0]) | (u > b[1])                                             # :291
        out_y = (v < b[2]) | (v > b[3])                                             # :293
        max_d = f32(1.2) * mf_max                                                   # src/MapPoint.cc:382
        min_d = f32(0.8) * mf_min                                                   # src/MapPoint.cc:376
        PO = P - Ow[None, :]                                                        # :299
        dist = np.sqrt(_dot3(PO, PO)).astype(f32)                                   # :300
        bad_dist = (dist < min_d) | (dist > max_d)                                  # :302
        vc = (_dot3(PO, Pn) / dist.astype(f64)).astype(f32)                         # :308
        bad_cos = vc < f32(viewing_cos_limit)                                       # :310
        level, undefined = predict_scale(mf_max, dist, V["log_scale_factor"], int(V["nlevels"]))   # :314
        ur = u - V["mbf"] * invz                                                    # :319
    status = np.full(n, IN_VIEW, np.uint8)
    for gate, code in ((undefined, UNDEFINED), (bad_cos, VIEW_COS), (bad_dist, DISTANCE), (out_y, OUT_Y), (out_x, OUT_X), (behind, BEHIND),
                       (skip != 0, SKIPPED)):
        status[gate] = code                                                         # the earliest line wins: assigned last
    ok = status == IN_VIEW
    z = f32(0)
    return (status, np.where(ok, u, z).astype(f32), np.where(ok, v, z).astype(f32), np.where(ok, ur, z).astype(f32),
            np.where(ok, level, 0).astype(np.int32), np.where(ok, vc, z).astype(f32), int(ok.sum()))


def frustum_f64(view, skip, xw, normal, mf_max, mf_min, viewing_cos_limit):
    """The same test in plain float64 -> (status, u, v, ur, level, view_cos, margin): margin[i] is the smallest relative distance
    of point i to any gate (depth sign, the four bounds, the two distances, the cosine limit, the next integer of the level
    quotient); nan where something is not finite.  Skipped points have margin inf."""
    V = view
    P, Pn = np.asarray(xw, f64).reshape(-1, 3), np.asarray(normal, f64).reshape(-1, 3)
    mf_max, mf_min = np.asarray(mf_max, f64), np.asarray(mf_min, f64)
    R, t, Ow, b = V["Rcw"].astype(f64).reshape(3, 3), V["tcw"].astype(f64), V["Ow"].astype(f64), V["bounds"].astype(f64)
    with np.errstate(all="ignore"):
        Pc = P @ R.T + t
        u = f64(V["fx"]) * Pc[:, 0] / Pc[:, 2] + f64(V["cx"])
        v = f64(V["fy"]) * Pc[:, 1] / Pc[:, 2] + f64(V["cy"])
        PO = P - Ow
        dist = np.linalg.norm(PO, axis=1)
        max_d, min_d = 1.2 * mf_max, 0.8 * mf_min
        vc = (PO * Pn).sum(1) / dist
        q = np.log(mf_max / dist) / f64(V["log_scale_factor"])
        level = np.clip(np.ceil(q), 0, int(V["nlevels"]) - 1)
        ur = u - f64(V["mbf"]) / Pc[:, 2]
        wdt, hgt = b[1] - b[0], b[3] - b[2]
        margin = np.min(np.stack([np.abs(Pc[:, 2]) / dist, np.abs(u - b[0]) / wdt, np.abs(u - b[1]) / wdt, np.abs(v - b[2]) / hgt,
                                  np.abs(v - b[3]) / hgt, np.abs(dist - min_d) / dist, np.abs(dist - max_d) / dist,
                                  np.abs(vc - f64(f32(viewing_cos_limit))), np.abs(q - np.rint(q)) / np.maximum(1.0, np.abs(q))]), 0)
    status = np.full(len(P), IN_VIEW, np.uint8)
    for gate, code in ((vc < f64(f32(viewing_cos_limit)), VIEW_COS), ((dist < min_d) | (dist > max_d), DISTANCE), ((v < b[2]) | (v > b[3]), OUT_Y),
                       ((u < b[0]) | (u > b[1]), OUT_X), (Pc[:, 2] < 0, BEHIND), (np.asarray(skip) != 0, SKIPPED)):
        status[gate] = code
    margin = np.where(np.asarray(skip) != 0, np.inf, margin)
    return status, u, v, ur, level, vc, margin


# ---- synthetic scenes

class Scene:
    """A frame's view block and its local map: what Tracking::SearchLocalPoints hands to the loop."""

    def __init__(self, view, skip, xw, normal, mf_max, mf_min):
        self.view = view
        self.skip = np.ascontiguousarray(skip, np.uint8)
        self.xw = np.ascontiguousarray(xw, f32).reshape(-1, 3)
        self.normal = np.ascontiguousarray(normal, f32).reshape(-1, 3)
        self.mf_max, self.mf_min = np.ascontiguousarray(mf_max, f32), np.ascontiguousarray(mf_min, f32)

    def __len__(self):
        return len(self.skip)

    def args(self):
        return self.view, self.skip, self.xw, self.normal, self.mf_max, self.mf_min

    def head(self, n):
        return Scene(self.view, self.skip[:n], self.xw[:n], self.normal[:n], self.mf_max[:n], self.mf_min[:n])


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(rng, n, W=1241, H=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, stereo=True, scale_factor=1.2, nlevels=8,
               skip_share=0.1, wild_share=0.2, degenerate_share=0.02, turn=0.0, log_scale_factor=None):
    """A camera near the origin (turned by `turn` radians about its y axis on top of a small random rotation) and n local MapPoints
    1 to 80 m from the origin over one and a half times its field of view, a few behind it.  Normal and mfMax / mfMinDistance of
    a point are what MapPoint::UpdateNormalAndDepth leaves after one observation from a reference camera (src/MapPoint.cc:359-369):
    normal = the unit ray from the reference camera, mfMaxDistance = dist * scaleFactor^octave, mfMinDistance = mfMaxDistance /
    scaleFactor^(nlevels - 1).  The reference camera is near the current one, or (wild_share) anywhere around the point.
    degenerate_share of the points carry an mfMaxDistance of inf, nan, 0 or a negative number."""
    Rcw = _rodrigues(rng.normal(0, 0.05, 3)) @ _rodrigues(np.array([0.0, turn, 0.0]))
    C = rng.normal(0, 0.5, 3)
    view = make_view(Rcw, -Rcw @ C, fx, fy, cx, cy, 0.54 * fx if stereo else 0.0, (0.0, W, 0.0, H), scale_factor, nlevels,
                     log_scale_factor=log_scale_factor)
    z = np.exp(rng.uniform(np.log(1.0), np.log(80.0), n))
    z = np.where(rng.random(n) < 0.06, -z, z)
    hx, hy = np.arctan(0.5 * W / fx), np.arctan(0.5 * H / fy)
    P = np.stack([np.abs(z) * np.tan(rng.uniform(-1.5 * hx, 1.5 * hx, n)), np.abs(z) * np.tan(rng.uniform(-1.6 * hy, 1.6 * hy, n)), z], 1)
    near = C + rng.normal(0, 1.5, (n, 3))
    d = rng.normal(0, 1, (n, 3))
    around = P - d / np.linalg.norm(d, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(1.0), np.log(80.0), (n, 1)))
    Oref = np.where(rng.random((n, 1)) < wild_share, around, near)
    P32 = P.astype(f32)
    PC = P32 - Oref.astype(f32)
    dist_ref = np.sqrt((PC.astype(f64) ** 2).sum(1)).astype(f32)
    normal = (PC / dist_ref[:, None]).astype(f32)
    sf = view["scale_factors"]
    mf_max = dist_ref * sf[rng.integers(0, nlevels, n)]
    mf_min = mf_max / sf[nlevels - 1]
    deg = rng.random(n) < degenerate_share
    with np.errstate(all="ignore"):
        mf_max = np.where(deg, rng.choice(np.array([np.inf, np.nan, 0.0, -3.0], f32), n), mf_max).astype(f32)
        mf_min = np.where(deg, f32(0), mf_min).astype(f32)
    return Scene(view, rng.random(n) < skip_share, P32, normal, mf_max, mf_min)


# the scenes of the test suite: (seed, n, keyword arguments of make_scene)
SUITE = [
    (1, 5000, dict()),                                              # stereo, the usual frame
    (2, 5000, dict(stereo=False)),                                  # monocular: mbf = 0
    (3, 3000, dict(turn=2.6)),                                      # looking away: most points behind or outside
    (4, 3000, dict(W=640, H=480, fx=517.3, fy=516.5, cx=318.6, cy=255.3, scale_factor=1.1, nlevels=12, wild_share=0.5)),
    (5, 2000, dict(scale_factor=1.0, nlevels=1)),                   # mfLogScaleFactor = 0: every level quotient is inf or nan
    (6, 2000, dict(scale_factor=2.0, nlevels=4, skip_share=0.4, degenerate_share=0.1)),
]


def suite_scene(k):
    seed, n, kw = SUITE[k]
    return make_scene(np.random.default_rng(seed), n, **kw)


class FrameSide:
    """The current frame as ORBmatcher::SearchByProjection reads it: mvKeysUn, mDescriptors, mvuRight, and per slot the
    Observations() of the MapPoint it already holds (-1: none); plus the local map's descriptors and Observations()."""

    def __init__(self, kps, desc, u_right, cur_obs, mp_desc, mp_obs):
        self.kps, self.desc, self.u_right, self.cur_obs, self.mp_desc, self.mp_obs = kps, desc, u_right, cur_obs, mp_desc, mp_obs


def make_frame(rng, sc, n_clutter=600, occupied_share=0.15, keep_share=0.8):
    """Key points where the scene's MapPoints project (float64 is good enough to place them), a pixel or so off, on the predicted
    level or the one below, with the MapPoint's descriptor and a few flipped bits; clutter in between; some slots taken.  u_right
    follows the projection for most stereo points, contradicts it for some and is -1 (monocular) for the rest."""
    st, u, v, ur, level, _, _ = frustum_f64(*sc.args(), 0.5)
    n = len(sc)
    mp_desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    mp_obs = rng.integers(1, 6, n).astype(np.int32)
    b = sc.view["bounds"]
    vis = np.flatnonzero((st == IN_VIEW) & np.isfinite(u) & np.isfinite(v) & (rng.random(n) < keep_share))
    m = len(vis) + n_clutter
    kps = np.zeros(m, KP_DTYPE)
    kps["x"] = np.concatenate([u[vis] + rng.normal(0, 0.8, len(vis)), rng.uniform(b[0], b[1], n_clutter)])
    kps["y"] = np.concatenate([v[vis] + rng.normal(0, 0.8, len(vis)), rng.uniform(b[2], b[3], n_clutter)])
    nl = int(sc.view["nlevels"])
    kps["octave"] = np.concatenate([np.clip(np.nan_to_num(level[vis]) - rng.integers(0, 2, len(vis)), 0, nl - 1), rng.integers(0, nl, n_clutter)])
    kps["angle"] = rng.uniform(0, 360, m)
    desc = np.concatenate([mp_desc[vis], rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
    flips = rng.random((m, 256)) < 0.06
    desc = desc ^ np.packbits(flips, axis=1)
    u_right = np.full(m, -1, f32)
    if sc.view["mbf"] > 0:
        u_right[:len(vis)] = ur[vis]
        u_right[:len(vis)][rng.random(len(vis)) < 0.1] += 40.0
        u_right[rng.random(m) < 0.2] = -1.0
    order = rng.permutation(m)
    cur_obs = np.where(rng.random(m) < occupied_share, rng.integers(0, 3, m), -1).astype(np.int32)
    return FrameSide(np.ascontiguousarray(kps[order]), np.ascontiguousarray(desc[order]), np.ascontiguousarray(u_right[order]), cur_obs, mp_desc, mp_obs)


def distance(view, xw):
    """cv::norm(P - mOw) of src/Frame.cc:299-300 in float"""
    PO = np.ascontiguousarray(xw, f32).reshape(-1, 3) - view["Ow"][None, :]
    with np.errstate(all="ignore"):
        return np.sqrt(_dot3(PO, PO)).astype(f32)


# ---- hand-made inputs

def _rig(fx=500.0, fy=500.0, t=(0.0, 0.0, 0.0), **kw):
    """camera at the origin looking down z, fx = fy = 500, principal point (320, 240), a 640 x 480 image, mbf = 40"""
    return make_view(np.eye(3), t, fx, fy, 320.0, 240.0, 40.0, (0.0, 640.0, 0.0, 480.0), **kw)


def _points(view, P, normal=None, mf_max=5.0, mf_min=1.0):
    P = np.asarray(P, f32).reshape(-1, 3)
    n = len(P)
    if normal is None:
        with np.errstate(all="ignore"):
            normal = P / np.linalg.norm(P.astype(f64), axis=1, keepdims=True)
    return Scene(view, np.zeros(n, np.uint8), P, np.broadcast_to(np.asarray(normal, f32), (n, 3)), np.broadcast_to(f32(mf_max), n),
                 np.broadcast_to(f32(mf_min), n))


def quirk_cases():
    """name -> (scene, viewingCosLimit, expected statuses).  The base point (0.2, 0.1, 4) projects to (345, 252.5), is 4.006 m away
    with mfMaxDistance = 5 and mfMinDistance = 1 (range 0.8 .. 6), is seen along its normal (viewCos = 1) and lands on level
    ceil(log(5 / 4.006) / log(1.2)) = ceil(1.215) = 2."""
    base = [0.2, 0.1, 4.0]
    nan = float("nan")
    return {
        "base point is in view": (_points(_rig(), base), 0.5, [IN_VIEW]),
        # PcZ = +0 is not < 0: invz = +inf, u = 500 * 0.1 * inf + 320 = +inf > mnMaxX
        "+0 depth passes :283": (_points(_rig(), [0.1, 0.05, 0.0]), 0.5, [OUT_X]),
        # 0 * -0.1 = -0, -0 + -0 = -0, and -0 + (double)-0 = -0: PcZ = -0 is not < 0 either; invz = -inf, u = 500 * -0.1 * -inf = +inf
        "-0 depth passes :283": (_points(_rig(t=(0.0, 0.0, -0.0)), [-0.1, -0.2, -0.0]), 0.5, [OUT_X]),
        # on the camera's y axis: u = 500 * 0 * inf + 320 = NaN passes :291, v = +inf is caught by :293
        "NaN u passes :291": (_points(_rig(), [0.0, 0.05, 0.0]), 0.5, [OUT_Y]),
        # a NaN focal length makes u (or v) NaN and nothing else: both bounds tests pass and the point is in view with a NaN projection
        "NaN u passes to the end": (_points(_rig(fx=nan), base), 0.5, [IN_VIEW]),
        "NaN v passes :293": (_points(_rig(fy=nan), base), 0.5, [IN_VIEW]),
        # a NaN normal: viewCos = NaN is not < 0.5
        "NaN viewCos passes :310": (_points(_rig(), base, normal=[nan, 0.0, 1.0]), 0.5, [IN_VIEW]),
        # looking along -normal: viewCos = -1 < 0.5
        "seen from behind": (_points(_rig(), base, normal=[-0.05, -0.025, -1.0]), 0.5, [VIEW_COS]),
        # mfMaxDistance = inf: ratio = inf, log = inf; nan: every comparison of :302 is false, log(nan) = nan
        "level of an infinite mfMaxDistance": (_points(_rig(), base, mf_max=np.inf), 0.5, [UNDEFINED]),
        "level of a NaN mfMaxDistance": (_points(_rig(), base, mf_max=nan), 0.5, [UNDEFINED]),
        # mfLogScaleFactor = 0: 0.2216 / 0 = inf;  1e-12: 2.2e11 is beyond int
        "level with mfLogScaleFactor = 0": (_points(_rig(log_scale_factor=0.0), base), 0.5, [UNDEFINED]),
        "level quotient beyond int": (_points(_rig(log_scale_factor=1e-12), base), 0.5, [UNDEFINED]),
        # -1e-12: -2.2e11 is beyond int on the other side
        "level quotient below int": (_points(_rig(log_scale_factor=-1e-12), base), 0.5, [UNDEFINED]),
        # mfMaxDistance = 0 never reaches PredictScale: dist > 1.2 * 0
        "mfMaxDistance = 0": (_points(_rig(), base, mf_max=0.0, mf_min=0.0), 0.5, [DISTANCE]),
        "behind": (_points(_rig(), [0.2, 0.1, -4.0]), 0.5, [BEHIND]),
    }


def ceil_boundary_scenes():
    """Per (scale factor, levels): the point (0, 0, 1) seen from the origin, dist = 1 exactly, so ratio = mfMaxDistance exactly;
    mfMaxDistance = mvScaleFactors[k] and its two float neighbours for every k -- the inputs on which ceil(log(ratio) /
    mfLogScaleFactor) sits on an integer.  -> [(scene, k of every point)]"""
    out = []
    for scale_factor, nlevels in ((1.2, 8), (1.1, 12), (2.0, 4), (1.5, 6), (1.2, 16), (1.44, 8)):
        view = _rig(scale_factor=scale_factor, nlevels=nlevels)
        sf = view["scale_factors"][:nlevels]
        mf = np.stack([np.nextafter(sf, f32(0)), sf, np.nextafter(sf, f32(np.inf))], 1).reshape(-1)
        sc = _points(view, np.tile([0.0, 0.0, 1.0], (len(mf), 1)), normal=[0.0, 0.0, 1.0])
        sc.mf_max, sc.mf_min = np.ascontiguousarray(mf, f32), np.full(len(mf), 0.1, f32)
        out.append((sc, np.repeat(np.arange(nlevels), 3)))
    return out
