"""Oracles, scenes and an object-graph model for orbm_fuse_views (include/orbm.h): ORBmatcher::Fuse(pKF, vpMapPoints, th)
(src/ORBmatcher.cc:825-975 of WChen09/My-SLAM) for every target key frame of LocalMapping::SearchInNeighbors
(src/LocalMapping.cc:456-536) in one call.  Test infrastructure only.

  project()      :852-890 in numpy, on frustum_oracle's arithmetic (cv::gemm's small-matrix path, double dot products, the
                 correctly rounded logf): status, u, v, ur, predicted level of every (view, MapPoint) slot
  select()       :892-949 for one slot, the window from the C oracle's key-frame grid (oracle_lib.KeyFrameGrid)
  oro_fuse       the whole of :852-952 per view on the C oracle (oracle_lib.fuse): the independent statement of the search
  MapPoint, KeyFrame, bookkeeping()   the part of the object graph the loop writes (:954-970; MapPoint::Replace with the
                 descriptor update of src/MapPoint.cc:177-215, :242-307)
  sequential()   the reference's loop: one Fuse per view, every point searched with its live descriptor
  snapshot(), replay()   what the batch call returns on the state before the loop, and the adapter's replay of it
                 (host/ORBmatcher.h), with and without the re-selection rule
"""
import numpy as np

import frustum_oracle as F
import mappoint_oracle as MO
import oracle_lib as O

f32, f64 = np.float32, np.float64
MAX_LEVELS = 16
TH_LOW = 50
MATCH, SKIPPED, BEHIND, OUT_IMAGE, DISTANCE, VIEW_ANGLE, UNDEFINED, NO_MATCH = range(8)
STATUS_NAMES = ["match", "skipped", "behind", "out_image", "distance", "view_angle", "undefined", "no_match"]
KP_DTYPE = F.KP_DTYPE
GRID_DTYPE = np.dtype([("assign_min_x", "<f4"), ("assign_min_y", "<f4"), ("inv_w", "<f4"), ("inv_h", "<f4"), ("query_min_x", "<f4"),
                       ("query_min_y", "<f4")])
VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("mbf", "<f4"), ("bounds", "<f4", (4,)), ("log_scale_factor", "<f4"), ("nlevels", "<i4"),
                       ("scale_factors", "<f4", (MAX_LEVELS,)), ("inv_level_sigma2", "<f4", (MAX_LEVELS,)), ("grid", GRID_DTYPE)])

W, H, FX, FY, CX, CY, MBF = 640, 480, 500.0, 500.0, 320.0, 240.0, 40.0


def make_view(R=np.eye(3), t=(0.0, 0.0, 0.0), fx=FX, fy=FY, cx=CX, cy=CY, mbf=MBF, width=W, height=H, scale_factor=1.2, nlevels=8,
              min_x=0.0, min_y=0.0, log_scale_factor=None):
    """One orbm_fuse_view: frustum_oracle.make_view's pose, calibration and pyramid, mvInvLevelSigma2 as the extractor's
    constructor fills it (1.0f / (sf*sf)), and the key frame's grid over [min, min + size) (64 x 48 cells)."""
    fv = F.make_view(R, t, fx, fy, cx, cy, mbf, (min_x, min_x + width, min_y, min_y + height), scale_factor, nlevels,
                     log_scale_factor=log_scale_factor)
    v = np.zeros((), VIEW_DTYPE)
    for k in fv.dtype.names:
        v[k] = fv[k]
    sf = v["scale_factors"]
    inv = np.zeros(MAX_LEVELS, f32)
    inv[:nlevels] = f32(1.0) / (sf[:nlevels] * sf[:nlevels])
    v["inv_level_sigma2"] = inv
    v["grid"]["assign_min_x"], v["grid"]["assign_min_y"] = f32(min_x), f32(min_y)
    v["grid"]["inv_w"], v["grid"]["inv_h"] = f32(64.0) / f32(width), f32(48.0) / f32(height)
    v["grid"]["query_min_x"], v["grid"]["query_min_y"] = f32(min_x), f32(min_y)
    return v


def grid_tuple(view):
    g = view["grid"]
    return tuple(float(g[k]) for k in GRID_DTYPE.names)


# ---- :852-890

def project(V, skip, xw, normal, mf_max, mf_min):
    """-> (status uint8, u, v, ur float32, level int32, dist float32) for the MapPoints against one view.  status is NO_MATCH for a
    point that reached :887 (the search decides between that and MATCH); u, v, ur, level are zeros for every other point."""
    skip = np.asarray(skip, np.uint8)
    P = np.ascontiguousarray(xw, f32).reshape(-1, 3)
    Pn = np.ascontiguousarray(normal, f32).reshape(-1, 3)
    mf_max, mf_min = np.asarray(mf_max, f32), np.asarray(mf_min, f32)
    R, t, Ow, b = V["Rcw"], V["tcw"], V["Ow"], V["bounds"]
    with np.errstate(all="ignore"):
        PcX, PcY, PcZ = F._gemm_row(R[0:3], t[0], P), F._gemm_row(R[3:6], t[1], P), F._gemm_row(R[6:9], t[2], P)   # :853
        behind = PcZ < f32(0)                                                       # :856
        invz = f32(1) / PcZ                                                         # :859
        x, y = PcX * invz, PcY * invz                                               # :860-861
        u = V["fx"] * x + V["cx"]                                                   # :863
        v = V["fy"] * y + V["cy"]                                                   # :864
        out = ~((u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3]))                # :867 KeyFrame::IsInImage; NaN fails
        ur = u - V["mbf"] * invz                                                    # :870
        max_d, min_d = f32(1.2) * mf_max, f32(0.8) * mf_min                         # src/MapPoint.cc:382, :376
        PO = P - Ow[None, :]                                                        # :874
        dist = np.sqrt(F._dot3(PO, PO)).astype(f32)                                 # :875
        bad_dist = (dist < min_d) | (dist > max_d)                                  # :878
        bad_angle = F._dot3(PO, Pn) < 0.5 * dist.astype(f64)                        # :884, both sides double
        level, undefined = F.predict_scale(mf_max, dist, V["log_scale_factor"], int(V["nlevels"]))   # :887
    status = np.full(len(P), NO_MATCH, np.uint8)
    for gate, code in ((undefined, UNDEFINED), (bad_angle, VIEW_ANGLE), (bad_dist, DISTANCE), (out, OUT_IMAGE), (behind, BEHIND),
                       (skip != 0, SKIPPED)):
        status[gate] = code                                                         # the earliest line wins: assigned last
    ok = status == NO_MATCH
    z = f32(0)
    return (status, np.where(ok, u, z).astype(f32), np.where(ok, v, z).astype(f32), np.where(ok, ur, z).astype(f32),
            np.where(ok, level, 0).astype(np.int32), dist)


# ---- the key frames' features and :892-949

class Features:
    """mvKeysUn, mvuRight, mDescriptors of one key frame, and its grid on the C oracle"""

    def __init__(self, view, kps, u_right, desc):
        self.view = view
        self.kps = np.ascontiguousarray(kps, KP_DTYPE)
        self.u_right = np.ascontiguousarray(u_right, f32)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.grid = O.KeyFrameGrid(self.kps, grid_tuple(view))

    def __len__(self):
        return len(self.kps)


def radius(view, level, th):
    return f32(th) * view["scale_factors"][level]                                   # :890


def gate_value(view, feat, idx, u, v, ur):
    """-> (e2 * mvInvLevelSigma2[kpLevel] in float, the limit it is compared with in double): :914-937"""
    kp = feat.kps[idx]
    inv = view["inv_level_sigma2"][min(max(int(kp["octave"]), 0), MAX_LEVELS - 1)]
    ex, ey = f32(u) - kp["x"], f32(v) - kp["y"]
    if feat.u_right[idx] >= 0:
        er = f32(ur) - feat.u_right[idx]
        return (ex * ex + ey * ey + er * er) * inv, 7.8
    return (ex * ex + ey * ey) * inv, 5.99


def select(view, feat, u, v, ur, level, desc, th):
    """:892-949 for one MapPoint -> (bestIdx, bestDist); (-1, 256) when no candidate survives"""
    level = int(level)
    idxs = feat.grid.features_in_area(float(u), float(v), float(radius(view, level, th))) if len(feat) else []
    best, bidx = 256, -1
    for idx in idxs:
        oct_ = int(feat.kps["octave"][idx])
        if oct_ < level - 1 or oct_ > level:                                        # :911
            continue
        e, lim = gate_value(view, feat, idx, u, v, ur)
        if float(e) > lim:                                                          # :925 / :936: a float against a double
            continue
        d = MO.descriptor_distance(desc, feat.desc[idx])
        if d < best:                                                                # :944
            best, bidx = d, int(idx)
    return bidx, best


def oro_fuse(view, feat, usable, xw, normal, mf_max, mf_min, mp_desc, th):
    """:852-952 for the MapPoints against one view on the C oracle -> best_idx int32 (-1: not fused)"""
    n = len(usable)
    if n == 0 or len(feat) == 0:
        return np.full(n, -1, np.int32)
    T = np.eye(4, dtype=f32)
    T[:3, :3] = view["Rcw"].reshape(3, 3)
    T[:3, 3] = view["tcw"]
    nl = int(view["nlevels"])
    mf_max, mf_min = np.asarray(mf_max, f32), np.asarray(mf_min, f32)
    with np.errstate(all="ignore"):
        mn, mx = f32(0.8) * mf_min, f32(1.2) * mf_max
    bi, _ = O.fuse(usable, xw, normal, mn, mx, mf_max, mp_desc, T, view["Ow"], (float(view["fx"]), float(view["fy"]), float(view["cx"]), float(view["cy"])),
                   float(view["mbf"]), view["bounds"], view["scale_factors"][:nl], view["inv_level_sigma2"][:nl], float(view["log_scale_factor"]),
                   feat.grid, feat.u_right, feat.desc, float(th))
    return bi


# ---- the object graph

class KeyFrame:
    def __init__(self, kid, u_right, desc):
        self.id, self.u_right, self.desc = kid, u_right, desc
        self.slots = [None] * len(desc)                                             # mvpMapPoints


class MapPoint:
    def __init__(self, mid, desc):
        self.id, self.desc = mid, np.array(desc, np.uint8)
        self.bad, self.replaced, self.obs, self.nobs = False, None, {}, 0           # mObservations: key frame -> idx

    def is_in_keyframe(self, kf):
        return kf in self.obs

    def add_observation(self, kf, idx):                                             # src/MapPoint.cc:98-109
        if kf in self.obs:
            return
        self.obs[kf] = idx
        self.nobs += 2 if kf.u_right[idx] >= 0 else 1

    def _ordered(self):                                                             # std::map order: by key frame (its id here)
        return sorted(self.obs.items(), key=lambda e: e[0].id)

    def compute_distinctive_descriptors(self):                                      # :242-307
        if self.bad or not self.obs:
            return
        D = np.stack([kf.desc[idx] for kf, idx in self._ordered()])
        best, _ = MO.distinctive_descriptor(D)
        self.desc = D[best].copy()

    def replace(self, other):                                                       # :177-215
        if other.id == self.id:
            return
        obs = self._ordered()
        self.obs, self.bad, self.replaced = {}, True, other
        for kf, idx in obs:
            if not other.is_in_keyframe(kf):
                kf.slots[idx] = other                                               # ReplaceMapPointMatch
                other.add_observation(kf, idx)
            else:
                kf.slots[idx] = None                                                # EraseMapPointMatch
        other.compute_distinctive_descriptors()


def bookkeeping(kf, mp, best_idx):
    """:954-970"""
    in_kf = kf.slots[best_idx]
    if in_kf is not None:
        if not in_kf.bad:
            if in_kf.nobs > mp.nobs:
                mp.replace(in_kf)
            else:
                in_kf.replace(mp)
    else:
        mp.add_observation(kf, best_idx)
        kf.slots[best_idx] = mp


class State:
    """a live copy of a scene's graph: kfs = every key frame (the views first), vp = vpMapPoints (None: a NULL entry)"""

    def __init__(self, kfs, mps, vp):
        self.kfs, self.mps, self.vp = kfs, mps, vp

    def graph(self):
        """everything the loop can write, comparable with =="""
        return ([(m.bad, m.replaced.id if m.replaced else -1, [(kf.id, idx) for kf, idx in m._ordered()], m.nobs, m.desc.tobytes()) for m in self.mps],
                [[s.id if s else -1 for s in kf.slots] for kf in self.kfs])


class Scene:
    """views[v] (VIEW_DTYPE) with feats[v] (Features); the MapPoint list's geometry (xw, normal, mf_max, mf_min: one row per entry of
    vpMapPoints, zeros for a NULL entry); and the graph before the loop: home[h] = (u_right, desc) of the key frames outside the
    loop, points[k] = (descriptor, bad, [(key frame, idx)]) with key frames numbered views first, vp[i] = index into points or -1."""

    def __init__(self, views, feats, xw, normal, mf_max, mf_min, home, points, vp, th=3.0):
        self.views, self.feats, self.th = views, feats, th
        self.xw, self.normal = np.ascontiguousarray(xw, f32).reshape(-1, 3), np.ascontiguousarray(normal, f32).reshape(-1, 3)
        self.mf_max, self.mf_min = np.ascontiguousarray(mf_max, f32), np.ascontiguousarray(mf_min, f32)
        self.home, self.points, self.vp = home, points, list(vp)
        self._proj = None

    nviews = property(lambda s: len(s.views))
    n_mp = property(lambda s: len(s.vp))

    def state(self):
        kfs = [KeyFrame(v, f.u_right, f.desc) for v, f in enumerate(self.feats)]
        kfs += [KeyFrame(self.nviews + h, ur, d) for h, (ur, d) in enumerate(self.home)]
        mps = []
        for k, (desc, bad, obs) in enumerate(self.points):
            m = MapPoint(k, desc)
            m.bad = bad
            for kf, idx in obs:
                assert kfs[kf].slots[idx] is None
                kfs[kf].slots[idx] = m
                m.add_observation(kfs[kf], idx)
            mps.append(m)
        return State(kfs, mps, [mps[k] if k >= 0 else None for k in self.vp])

    def inputs(self, st=None):
        """the batch call's arguments on the state st (default: before the loop), in ORBmatcher.fuse_views' order"""
        st = st or self.state()
        skip = np.array([[1 if (m is None or m.bad or m.is_in_keyframe(st.kfs[v])) else 0 for m in st.vp] for v in range(self.nviews)], np.uint8)
        skip = skip.reshape(self.nviews, self.n_mp)
        mp_desc = np.stack([m.desc if m is not None else np.zeros(32, np.uint8) for m in st.vp]) if self.n_mp else np.zeros((0, 32), np.uint8)
        off = np.zeros(self.nviews + 1, np.int32)
        off[1:] = np.cumsum([len(f) for f in self.feats])
        cat = lambda arrs, dt, tail=(): np.concatenate(arrs) if arrs else np.zeros((0,) + tail, dt)
        return (np.array(self.views, VIEW_DTYPE), off, cat([f.kps for f in self.feats], KP_DTYPE), cat([f.u_right for f in self.feats], f32),
                cat([f.desc for f in self.feats], np.uint8, (32,)), skip, self.xw, self.normal, self.mf_max, self.mf_min, mp_desc)

    def projection(self):
        """project() of every point against every view with nothing skipped (the geometry does not change during the loop)"""
        if self._proj is None:
            none = np.zeros(self.n_mp, np.uint8)
            self._proj = [project(V, none, self.xw, self.normal, self.mf_max, self.mf_min) for V in self.views]
        return self._proj


def snapshot(sc):
    """orbm_fuse_views on the state before the loop, from the oracles -> (status, best_idx, best_dist, u, v, ur, level [nviews, n_mp],
    nfused [nviews], mp_desc).  best_idx / the MATCH status come from the C oracle's Fuse, best_dist from select()."""
    views, off, kps, ur_kf, dk, skip, xw, normal, mf_max, mf_min, mp_desc = sc.inputs()
    nv, n = sc.nviews, sc.n_mp
    status, bi, bd = np.zeros((nv, n), np.uint8), np.full((nv, n), -1, np.int32), np.full((nv, n), 256, np.int32)
    u, v, ur = np.zeros((nv, n), f32), np.zeros((nv, n), f32), np.zeros((nv, n), f32)
    lv = np.zeros((nv, n), np.int32)
    for k in range(nv):
        status[k], u[k], v[k], ur[k], lv[k], _ = project(views[k], skip[k], xw, normal, mf_max, mf_min)
        reached = (status[k] == NO_MATCH).astype(np.uint8)
        bi[k] = oro_fuse(views[k], sc.feats[k], reached, xw, normal, mf_max, mf_min, mp_desc, sc.th)
        status[k][bi[k] >= 0] = MATCH
        for i in np.flatnonzero(reached):
            bd[k, i] = select(views[k], sc.feats[k], u[k, i], v[k, i], ur[k, i], lv[k, i], mp_desc[i], sc.th)[1]
    return status, bi, bd, u, v, ur, lv, (status == MATCH).sum(1).astype(np.int32), mp_desc


def sequential(sc):
    """The reference's loop (src/LocalMapping.cc:487-492 around src/ORBmatcher.cc:842-972): view after view, point after point,
    :849 and the descriptor read on the live objects, the search on the C oracle.  -> (state, per-view counts)"""
    st = sc.state()
    proj = sc.projection()
    counts = []
    for k in range(sc.nviews):
        kf, n_fused = st.kfs[k], 0
        reached = proj[k][0] == NO_MATCH
        for i, mp in enumerate(st.vp):
            if mp is None or mp.bad or mp.is_in_keyframe(kf) or not reached[i]:
                continue
            best = int(oro_fuse(sc.views[k], sc.feats[k], np.ones(1, np.uint8), sc.xw[i:i + 1], sc.normal[i:i + 1], sc.mf_max[i:i + 1],
                                sc.mf_min[i:i + 1], mp.desc[None, :], sc.th)[0])
            if best < 0:
                continue
            bookkeeping(kf, mp, best)
            n_fused += 1
        counts.append(n_fused)
    return st, counts


def replay(sc, dense, reselect=True):
    """The adapter's replay of the batch result (host/ORBmatcher.h) -> (state, per-view counts, slots re-selected).  reselect=False
    leaves the rule out: every slot keeps the snapshot's selection."""
    status, bi, _, u, v, ur, lv, _, snap_desc = dense
    st = sc.state()
    counts, nres = [], 0
    for k in range(sc.nviews):
        kf, n_fused = st.kfs[k], 0
        for i, mp in enumerate(st.vp):
            if mp is None:
                continue
            if mp.bad or mp.is_in_keyframe(kf):                                     # :849 on the live objects
                continue
            if status[k, i] not in (MATCH, NO_MATCH):
                continue
            if not reselect or mp.desc.tobytes() == snap_desc[i].tobytes():
                if status[k, i] != MATCH:
                    continue
                best = int(bi[k, i])
            else:
                nres += 1
                best, d = select(sc.views[k], sc.feats[k], u[k, i], v[k, i], ur[k, i], lv[k, i], mp.desc, sc.th)
                if d > TH_LOW:
                    continue
            bookkeeping(kf, mp, best)
            n_fused += 1
        counts.append(n_fused)
    return st, counts, nres


# ---- scenes

def _flip(rng, desc, nbits):
    """desc with nbits random bits flipped"""
    d = np.unpackbits(np.asarray(desc, np.uint8))
    d[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(d)


def make_scene(seed, nviews, n_mp, nfeat, all_skipped_view=None, nhome=6, th=3.0):
    """Cameras near the origin, n_mp MapPoints 2 to 30 m in front of them (a few behind, outside, out of their distance range, seen
    from the side, or with a degenerate mfMaxDistance), and per view nfeat[v] features: key points where points project (a pixel
    off, on the predicted level or the one below, the point's descriptor with some bits flipped, stereo or monocular) and clutter.
    Slots of the views hold the list's own points (those are skipped there), foreign MapPoints with fewer or more observations
    (Replace in both directions) or nothing (AddObservation); every MapPoint has observations in the `nhome` key frames outside the
    loop, whose descriptors feed the median rule.  all_skipped_view: every point of the list is already in that view."""
    rng = np.random.default_rng(seed)
    nl, sfac = 8, 1.2
    views = []
    for _ in range(nviews):
        R = F._rodrigues(rng.normal(0, 0.03, 3))
        C = rng.normal(0, 0.3, 3)
        views.append(make_view(R, -R @ C, scale_factor=sfac, nlevels=nl))
    sf = views[0]["scale_factors"] if nviews else make_view()["scale_factors"]
    z = np.exp(rng.uniform(np.log(2.0), np.log(30.0), n_mp))
    z = np.where(rng.random(n_mp) < 0.05, -z, z)
    hx, hy = np.arctan(0.5 * W / FX), np.arctan(0.5 * H / FY)
    P = np.stack([np.abs(z) * np.tan(rng.uniform(-1.25 * hx, 1.25 * hx, n_mp)), np.abs(z) * np.tan(rng.uniform(-1.25 * hy, 1.25 * hy, n_mp)), z], 1).astype(f32)
    d = rng.normal(0, 1, (n_mp, 3))
    around = P - d / np.linalg.norm(d, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(2.0), np.log(30.0), (n_mp, 1)))
    Oref = np.where(rng.random((n_mp, 1)) < 0.12, around, rng.normal(0, 0.4, (n_mp, 3))).astype(f32)
    PC = P - Oref
    dref = np.sqrt((PC.astype(f64) ** 2).sum(1)).astype(f32)
    normal = (PC / dref[:, None]).astype(f32)
    mf_max = dref * sf[rng.integers(0, 4, n_mp)]
    mf_max = np.where(rng.random(n_mp) < 0.08, mf_max * f32(0.3), mf_max).astype(f32)            # out of the distance range
    mf_min = (mf_max / sf[nl - 1]).astype(f32)
    deg = rng.random(n_mp) < 0.04
    with np.errstate(all="ignore"):
        mf_max = np.where(deg, rng.choice(np.array([np.inf, np.nan, 0.0], f32), n_mp), mf_max).astype(f32)
        mf_min = np.where(deg, f32(0), mf_min).astype(f32)

    base = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    home = [([], []) for _ in range(nhome)]                                         # u_right, desc rows

    def home_obs(desc, k):
        """k observations of a descriptor in distinct home key frames -> [(key frame, idx)]"""
        out = []
        for h in rng.choice(nhome, k, replace=False):
            home[h][0].append(f32(rng.uniform(0, W)) if rng.random() < 0.5 else f32(-1))
            home[h][1].append(_flip(rng, desc, int(rng.integers(0, 9))))
            out.append((nviews + int(h), len(home[h][1]) - 1))
        return out

    is_null = rng.random(n_mp) < 0.05
    is_bad = ~is_null & (rng.random(n_mp) < 0.04)
    points, vp = [], []
    for i in range(n_mp):
        if is_null[i]:
            vp.append(-1)
            continue
        points.append([base[i], bool(is_bad[i]), [] if is_bad[i] else home_obs(base[i], int(rng.integers(2, 5)))])
        vp.append(len(points) - 1)

    none = np.zeros(n_mp, np.uint8)
    feats = []
    for k in range(nviews):
        V = views[k]
        st, u, v, ur, lv, _ = project(V, none, P, normal, mf_max, mf_min)
        cand = np.flatnonzero((st == NO_MATCH) & ~is_null)
        want = int(nfeat[k])
        seen = rng.permutation(cand)[:min(len(cand), (want * 3 + 4) // 5)]
        rows = []                                                                   # (x, y, octave, u_right, desc, holder)
        for i in seen:
            octave = max(int(lv[i]) - int(rng.integers(0, 2)), 0)
            r = rng.random()
            kr = f32(-1) if r < 0.4 else f32(ur[i] + rng.normal(0, 0.5) + (30.0 if r > 0.93 else 0.0))
            desc = _flip(rng, base[i], int(rng.integers(0, 30)))
            r = rng.random()
            holder = ("own", i) if r < 0.2 and not is_bad[i] else ("foreign", int(rng.integers(0, 6))) if r < 0.6 else None
            rows.append((u[i] + rng.normal(0, 0.6), v[i] + rng.normal(0, 0.6), octave, kr, desc, holder))
        while len(rows) < want:
            holder = ("foreign", int(rng.integers(0, 6))) if rng.random() < 0.3 else None
            rows.append((rng.uniform(0, W), rng.uniform(0, H), int(rng.integers(0, nl)), f32(rng.uniform(0, W)) if rng.random() < 0.5 else f32(-1),
                         rng.integers(0, 256, 32, dtype=np.uint8), holder))
        if all_skipped_view == k:
            for i in range(n_mp):
                if not is_null[i] and not is_bad[i]:
                    rows.append((rng.uniform(0, W), rng.uniform(0, H), int(rng.integers(0, nl)), f32(-1), _flip(rng, base[i], 3), ("own", i)))
        rows = [rows[j] for j in rng.permutation(len(rows))]
        kps = np.zeros(len(rows), KP_DTYPE)
        own = set()
        for j, (x, y, octave, kr, desc, holder) in enumerate(rows):
            kps[j]["x"], kps[j]["y"], kps[j]["octave"], kps[j]["angle"] = x, y, octave, rng.uniform(0, 360)
            if holder is None:
                continue
            if holder[0] == "own":
                if holder[1] not in own:                                            # a MapPoint is in a key frame once
                    own.add(holder[1])
                    points[vp[holder[1]]][2].append((k, j))
            else:
                points.append([desc.copy(), False, [(k, j)] + home_obs(desc, holder[1])])
        feats.append(Features(V, kps, np.array([r[3] for r in rows], f32), np.array([r[4] for r in rows], np.uint8).reshape(-1, 32)))
    home = [(np.array(ur_, f32), np.array(dd, np.uint8).reshape(-1, 32)) for ur_, dd in home]
    return Scene(views, feats, P, normal, mf_max, mf_min, home, [tuple(p) for p in points], vp, th)


def reselect_scene():
    """The scene that needs the re-selection rule.  One MapPoint P in front of two views, descriptor X, with two stereo
    observations (X and X) in key frames outside the loop.  View 0 holds, where P projects, a foreign MapPoint Q with two
    monocular observations in two other key frames; all of Q's descriptors are Y = X with 40 bits flipped.  P matches Q's slot
    (distance 40 <= TH_LOW) and, having no fewer observations (4 against 3), absorbs Q (pMPinKF->Replace(pMP)): P's rows are now
    Y (view 0), X, X, Y, Y, whose median distance to the rest is 0 for Y and 40 for X, so P's descriptor becomes Y.  View 1 has two
    free features where P projects: c1 with X (0 from X, 40 from Y) and after it c2 = Y with 10 more bits flipped (50 from X, 10
    from Y).  The reference fuses P with c2 in view 1; the snapshot's selection says c1."""
    rng = np.random.default_rng(5)
    views = [make_view(), make_view(t=(0.1, 0.0, 0.0))]
    P = np.array([[0.3, 0.2, 5.0]], f32)
    dref = np.sqrt((P.astype(f64) ** 2).sum(1)).astype(f32)
    normal = (P / dref[:, None]).astype(f32)
    mf_max = dref * views[0]["scale_factors"][1]
    mf_min = mf_max / views[0]["scale_factors"][7]
    X = rng.integers(0, 256, 32, dtype=np.uint8)
    xb = np.unpackbits(X)
    order = rng.permutation(256)
    yb = xb.copy(); yb[order[:40]] ^= 1
    cb = yb.copy(); cb[order[40:50]] ^= 1
    Y, C2 = np.packbits(yb), np.packbits(cb)
    none = np.zeros(1, np.uint8)
    feats = []
    for k, descs in enumerate(([Y], [X, C2])):
        st, u, v, ur, lv, _ = project(views[k], none, P, normal, mf_max, mf_min)
        assert st[0] == NO_MATCH
        kps = np.zeros(len(descs), KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = u[0] + f32(0.25), v[0] + np.arange(len(descs), dtype=f32) * f32(0.5), lv[0]
        feats.append(Features(views[k], kps, np.full(len(descs), -1, f32), np.array(descs, np.uint8)))
    stereo, mono = np.full(1, 100.0, f32), np.full(1, -1, f32)
    home = [(stereo, np.array([X], np.uint8)), (stereo, np.array([X], np.uint8)), (mono, np.array([Y], np.uint8)), (mono, np.array([Y], np.uint8))]
    points = [(X, False, [(2, 0), (3, 0)]),                   # P: two stereo observations at home, Observations() == 4
              (Y, False, [(0, 0), (4, 0), (5, 0)])]           # Q: view 0's slot and two monocular ones at home, Observations() == 3
    return Scene(views, feats, P, normal, mf_max, mf_min, home, points, [0], 3.0)


SUITE = {
    "mix-5": dict(seed=11, nviews=5, n_mp=200, nfeat=[400, 70, 0, 1, 400]),           # the one bulk scene: every kind of view
    "skipview-3": dict(seed=12, nviews=3, n_mp=63, nfeat=[70, 8, 70], all_skipped_view=1),
    "single-65": dict(seed=13, nviews=1, n_mp=65, nfeat=[400]),
    "one-point": dict(seed=16, nviews=2, n_mp=1, nfeat=[70, 1]),                       # the point is fused in both views
    "n64-4": dict(seed=15, nviews=4, n_mp=64, nfeat=[70, 400, 1, 0]),
    "reselect": None,
}


def suite_scene(name):
    return reselect_scene() if SUITE[name] is None else make_scene(**SUITE[name])
