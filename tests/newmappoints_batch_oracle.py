"""Scenes and reference procedures for orbm_create_new_map_points (include/orbm.h): LocalMapping::CreateNewMapPoints
(src/LocalMapping.cc:209-454 of WChen09/My-SLAM) for all neighbours of a key frame in one call.  Test infrastructure only.

A scene is key frame 1 and K second views of one set of world points.  The expected values come from what the project already
has: oracle_lib.search_for_triangulation (the C oracle of SearchForTriangulation) per view, and triangulation_oracle.triangulate
on that view's pairs.  Two procedures use them:
  procedure A  the reference's order: for each view in turn, search with the current has_mp1, triangulate the pairs, set has_mp1 of
               the accepted ones (:436-451 gives the feature a MapPoint, and :699-703 skips it from then on)
  procedure B  what the feature does: search and triangulate every view on the initial snapshot, then, in view order, keep the
               pairs whose feature of key frame 1 has no MapPoint at that moment (the adapter's live filter)
tests/test_newmappoints_batch_cpu.py asserts A == B; the GPU tests compare the batch call with B's snapshot."""
import numpy as np

import oracle_lib as O
import triangulation_oracle as T

f32 = np.float32
NO_MATCH = 255


class Scene:
    """cam1 / kf1 / desc1 / has1 / fv1: key frame 1.  cams2 / kfs2 / descs2 / has2 / fvs2 / F12: one entry per second view.
    A FeatureVector is (node, off, idx): ascending node ids, CSR offsets, feature indices in ascending order inside a node."""

    def __init__(self, cam1, kf1, desc1, has1, fv1, cams2, kfs2, descs2, has2, fvs2, F12, only_stereo=False):
        self.cam1, self.kf1, self.desc1, self.has1, self.fv1 = cam1, kf1, np.ascontiguousarray(desc1, np.uint8), np.asarray(has1, np.uint8), fv1
        self.cams2, self.kfs2, self.descs2, self.has2, self.fvs2 = list(cams2), list(kfs2), [np.ascontiguousarray(d, np.uint8) for d in descs2], \
            [np.asarray(h, np.uint8) for h in has2], list(fvs2)
        self.F12 = np.ascontiguousarray(F12, f32).reshape(-1, 3, 3)
        self.only_stereo = bool(only_stereo)

    @property
    def nviews(self):
        return len(self.cams2)

    def batch_args(self, has1=None):
        """the arguments of ORBmatcher.create_new_map_points, in order"""
        if self.nviews:
            off2, kf2 = T.concat_keyframes(self.kfs2)
            desc2, has2 = np.concatenate(self.descs2), np.concatenate(self.has2)
            cams2 = np.array(self.cams2, T.CAM_DTYPE)
        else:
            off2, kf2 = np.zeros(1, np.int32), T.KeyFrame(np.zeros(0, T.KP_DTYPE), np.zeros((0, 2), f32), np.zeros(0, f32), np.zeros(0, f32))
            desc2, has2, cams2 = np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), np.zeros(0, T.CAM_DTYPE)
        fvo = np.zeros(self.nviews + 1, np.int32)
        fvo[1:] = np.cumsum([len(fv[0]) for fv in self.fvs2])
        node = np.concatenate([fv[0] for fv in self.fvs2] + [np.zeros(0, np.int32)]).astype(np.int32)
        idx = np.concatenate([fv[2] for fv in self.fvs2] + [np.zeros(0, np.int32)]).astype(np.int32)
        off, base = [np.zeros(1, np.int32)], 0
        for fv in self.fvs2:
            off.append(np.asarray(fv[1][1:], np.int32) + base)
            base += int(fv[1][-1])
        off = np.concatenate(off).astype(np.int32)
        return (self.cam1, self.kf1.kps_un, self.kf1.keys_xy, self.kf1.u_right, self.kf1.depth, self.desc1,
                self.has1 if has1 is None else has1, self.fv1, cams2, self.F12, off2, kf2.kps_un, kf2.keys_xy, kf2.u_right, kf2.depth, desc2,
                has2, fvo, (node, off, idx), self.only_stereo)

    def search_args(self, v):
        """Cw, T2w, K2, F12, sf2, sigma2 of the per-view entry points (orbm_search_for_triangulation and its oracle)"""
        c2 = self.cams2[v]
        T2w = np.eye(4, dtype=f32)
        T2w[:3, :3] = c2["Rcw"].reshape(3, 3)
        T2w[:3, 3] = c2["tcw"]
        nl = int(c2["nlevels"])
        return (self.cam1["Ow"], T2w, (float(c2["fx"]), float(c2["fy"]), float(c2["cx"]), float(c2["cy"])), self.F12[v],
                c2["scale_factors"][:nl], c2["level_sigma2"][:nl])


def feature_vector(nodes):
    """the CSR form of a FeatureVector from each feature's node id (-1: the feature is in no node)"""
    nodes = np.asarray(nodes, np.int64)
    ids = np.unique(nodes[nodes >= 0])
    off, idx = [0], []
    for n in ids:
        members = np.nonzero(nodes == n)[0]
        idx.extend(members.tolist())
        off.append(len(idx))
    return ids.astype(np.int32), np.asarray(off, np.int32), np.asarray(idx, np.int32)


def compute_f12(cam1, cam2):
    """LocalMapping::ComputeF12 (src/LocalMapping.cc:538-555): K1^-T [t12]x R12 K2^-1 with R12 = R1w R2w^T, t12 = -R12 t2w + t1w"""
    R1, t1 = cam1["Rcw"].reshape(3, 3).astype(np.float64), cam1["tcw"].astype(np.float64)
    R2, t2 = cam2["Rcw"].reshape(3, 3).astype(np.float64), cam2["tcw"].astype(np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K1 = np.array([[cam1["fx"], 0, cam1["cx"]], [0, cam1["fy"], cam1["cy"]], [0, 0, 1]], np.float64)
    K2 = np.array([[cam2["fx"], 0, cam2["cx"]], [0, cam2["fy"], cam2["cy"]], [0, 0, 1]], np.float64)
    return (np.linalg.inv(K1.T) @ tx @ R12 @ np.linalg.inv(K2)).astype(f32)


def _flip(rng, desc, nbits):
    """copies of 256-bit descriptors with up to nbits bits flipped: far inside TH_LOW = 50"""
    bits = np.unpackbits(desc, axis=1)
    for row in bits:
        row[rng.integers(0, 256, rng.integers(0, nbits + 1))] ^= 1
    return np.packbits(bits, axis=1)


def make_scene(seed, nviews, npts=260, stereo1=0.5, stereo2=0.5, node_size=6, has_mp=0.15, outliers=0.1, seen=0.85,
               baselines=(0.03, 3.0), only_stereo=False, noise=0.7, bad_depth=0.03, nlevels2=None, calib2=None, mbf2=None, duplicates=False,
               sigma2=None):
    """nviews second views of npts world points in front of key frame 1.  Every key frame lists its features in an order of its
    own; a view sees a share `seen` of the points.  A world point has a random descriptor and each observation flips a few bits;
    the `outliers` share of a view's features carries unrelated descriptors.  Node ids belong to world points (point // node_size),
    so a FeatureVector needs no vocabulary: node_size 1 is one feature per node, node_size >= npts one node for everything.
    A share has_mp of the features of every key frame already has a MapPoint.  The baselines grow from the first view to the
    last, so that pairs rejected for parallax in an early view come back in a later one.
    duplicates: the points of a node share one descriptor and no bit is flipped, so every candidate of a node ties and the last
    one wins; with sigma2 (every level's mvLevelSigma2 of the second views) large enough to pass any epipolar distance, that pairs
    features of different world points, which is where the depth-sign rejections come from."""
    rng = np.random.default_rng(seed)
    calib = T.KITTI
    R1 = T.rotation(*rng.normal(0, 0.05, 3))
    O1 = rng.normal(0, 20.0, 3)
    cam1 = T.make_camera(R1, -R1 @ O1, **calib)
    z = rng.uniform(2.0, 40.0, npts)
    xc = np.stack([(rng.uniform(0, 1240, npts) - calib["cx"]) / calib["fx"] * z, (rng.uniform(0, 370, npts) - calib["cy"]) / calib["fy"] * z, z], 1)
    Xw = (xc - (-R1 @ O1)) @ R1
    base_desc = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    octave = rng.integers(0, 8, npts)
    if duplicates:
        base_desc = base_desc[(np.arange(npts) // node_size) * node_size]

    def observe(cam, share_stereo, pts):
        kf = T._observe(rng, cam, Xw[pts], share_stereo, noise, bad_depth)
        nl = int(cam["nlevels"])
        consistent = rng.random(len(pts)) < 0.8
        kf.kps_un["octave"] = np.where(consistent, np.minimum(octave[pts], nl - 1), kf.kps_un["octave"])
        desc = base_desc[pts].copy() if duplicates else _flip(rng, base_desc[pts], 6)
        return kf, desc

    pts1 = rng.permutation(npts)
    kf1, desc1 = observe(cam1, stereo1, pts1)
    fv1 = feature_vector(pts1 // node_size)
    has1 = rng.random(npts) < has_mp
    cams2, kfs2, descs2, has2, fvs2, F12 = [], [], [], [], [], []
    for v in range(nviews):
        R2 = T.rotation(*rng.normal(0, 0.03, 3)) @ R1
        direction = rng.normal(0, 1, 3) * np.array([1.0, 0.2, 1.0])
        b = baselines[0] * (baselines[1] / baselines[0]) ** (v / max(nviews - 1, 1)) if nviews > 1 else baselines[1]
        O2 = O1 + b * direction / np.linalg.norm(direction)
        c2 = dict(calib if calib2 is None else calib2[v % len(calib2)])
        if mbf2 is not None:
            c2["mbf"] = mbf2
        nl = 8 if nlevels2 is None else nlevels2[v % len(nlevels2)]
        cam2 = T.make_camera(R2, -R2 @ O2, nlevels=nl, level_sigma2=None if sigma2 is None else np.full(T.MAX_LEVELS, sigma2), **c2)
        pts2 = rng.permutation(npts)[:max(int(seen * npts), 1)]
        st2 = stereo2[v % len(stereo2)] if isinstance(stereo2, (tuple, list)) else stereo2
        kf2, desc2 = observe(cam2, st2, pts2)
        wrong = rng.random(len(pts2)) < outliers
        desc2[wrong] = rng.integers(0, 256, (int(wrong.sum()), 32), dtype=np.uint8)
        cams2.append(cam2); kfs2.append(kf2); descs2.append(desc2); has2.append(rng.random(len(pts2)) < has_mp)
        fvs2.append(feature_vector(pts2 // node_size)); F12.append(compute_f12(cam1, cam2))
    return Scene(cam1, kf1, desc1, has1, fv1, cams2, kfs2, descs2, has2, fvs2, F12, only_stereo)


def degenerate_scene():
    """The two statuses no real pose pair reaches (triangulation_oracle.zero_distance_cases / w_zero_cases) as two views of one key
    frame 1: both cases put camera 1 at the origin with the same calibration.  Pair i of a case shares a descriptor and a node of
    its own; F12 maps every feature of key frame 1 to the line x = 320, on which all features of both views lie."""
    cam1, z1, camz, z2, _ = T.zero_distance_cases()
    _, w1, camw, w2, _ = T.w_zero_cases()
    n = len(z1)
    kf1 = T.KeyFrame(np.concatenate([z1.kps_un, w1.kps_un]), np.concatenate([z1.keys_xy, w1.keys_xy]),
                     np.concatenate([z1.u_right, w1.u_right]), np.concatenate([z1.depth, w1.depth]))
    rng = np.random.default_rng(5)
    desc1 = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
    F = np.zeros((3, 3), f32)
    F[2, 0], F[2, 2] = 1, -320
    fv1 = feature_vector(np.arange(2 * n))
    return Scene(cam1, kf1, desc1, np.zeros(2 * n, np.uint8), fv1, [camz, camw], [z2, w2], [desc1[:n], desc1[n:]],
                 [np.zeros(n, np.uint8), np.zeros(n, np.uint8)], [feature_vector(np.arange(n)), feature_vector(np.arange(n) + n)], [F, F])


# ---- the two per-view reference steps

def search_view(sc, v, has1):
    """matches12 of view v alone (int32 [n1], -1 = none) by the C oracle, check_orientation off"""
    kf2 = sc.kfs2[v]
    if len(sc.kf1) == 0 or len(kf2) == 0:
        return np.full(len(sc.kf1), -1, np.int32)
    m12, _ = O.search_for_triangulation(sc.kf1.kps_un, sc.desc1, has1, sc.kf1.u_right, sc.fv1, kf2.kps_un, sc.descs2[v], sc.has2[v], kf2.u_right,
                                        sc.fvs2[v], *sc.search_args(v), sc.only_stereo, False)
    return m12


def triangulate_view(sc, v, m12):
    """(pairs int32 [k, 2] in ascending idx1, status uint8 [k], x3d float32 [k, 3]) of view v's pair list"""
    i1 = np.nonzero(m12 >= 0)[0]
    pairs = np.stack([i1, m12[i1]], 1).astype(np.int32).reshape(-1, 2)
    matches = np.concatenate([pairs, np.zeros((len(pairs), 1), np.int32)], 1)
    status, x3d = T.triangulate(sc.cam1, sc.kf1, [sc.cams2[v]], [0, len(sc.kfs2[v])], sc.kfs2[v], matches)
    return pairs, status, x3d


def snapshot(sc):
    """Every view searched and triangulated on the initial snapshot: the dense outputs of the batch call
    (matches12 [nviews, n1], status, x3d [nviews, n1, 3], nmatches)."""
    n1 = len(sc.kf1)
    m12 = np.full((sc.nviews, n1), -1, np.int32)
    status = np.full((sc.nviews, n1), NO_MATCH, np.uint8)
    x3d = np.zeros((sc.nviews, n1, 3), f32)
    for v in range(sc.nviews):
        m12[v] = search_view(sc, v, sc.has1)
        pairs, st, x = triangulate_view(sc, v, m12[v])
        status[v, pairs[:, 0]] = st
        x3d[v, pairs[:, 0]] = x
    return m12, status, x3d, (m12 >= 0).sum(1).astype(np.int32)


def procedure_a(sc):
    """the reference's order; one (pairs, status, x3d) per view"""
    has1 = sc.has1.copy()
    out = []
    for v in range(sc.nviews):
        pairs, st, x = triangulate_view(sc, v, search_view(sc, v, has1))
        has1[pairs[st <= T.STEREO2, 0]] = 1                      # :446 mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
        out.append((pairs, st, x))
    return out


def replay(sc, dense):
    """procedure B's second half, the adapter's live filter over dense outputs (the oracle's snapshot() or the library's)"""
    m12, status, x3d = dense[:3]
    has1 = sc.has1.copy()
    out = []
    for v in range(sc.nviews):
        i1 = np.nonzero((m12[v] >= 0) & (has1 == 0))[0]
        pairs = np.stack([i1, m12[v, i1]], 1).astype(np.int32).reshape(-1, 2)
        st, x = status[v, i1], x3d[v, i1]
        has1[i1[st <= T.STEREO2]] = 1
        out.append((pairs, st, x))
    return out


def procedure_b(sc):
    return replay(sc, snapshot(sc))


def same_lists(a, b):
    """pair lists, statuses and x3D bit patterns of every view"""
    if len(a) != len(b):
        return False
    for (pa, sa, xa), (pb, sb, xb) in zip(a, b):
        if not (np.array_equal(pa, pb) and np.array_equal(sa, sb) and np.array_equal(xa.view(np.uint32), xb.view(np.uint32))):
            return False
    return True


# the scenes of the suite: name -> make_scene arguments
SUITE = {
    "mono-1": dict(seed=101, nviews=1, stereo1=0, stereo2=0, node_size=4),
    "mono-5": dict(seed=102, nviews=5, stereo1=0, stereo2=0, node_size=6, baselines=(0.3, 4.0)),
    "stereo-2": dict(seed=103, nviews=2, stereo1=1, stereo2=1, node_size=1, baselines=(0.04, 4.0)),
    "stereo-only-5": dict(seed=104, nviews=5, stereo1=0.6, stereo2=0.6, node_size=3, only_stereo=True),
    "mixed-8": dict(seed=105, nviews=8, stereo1=0.5, stereo2=(0.0, 1.0, 0.5), node_size=10 ** 6, npts=200),
    "mixed-5-calib": dict(seed=106, nviews=5, node_size=8, nlevels2=(8, 5, 12), mbf2=200.0,
                          calib2=(T.KITTI, dict(fx=520.9, fy=521.0, cx=325.1, cy=249.7, mbf=40.0))),
    "mixed-2-one-node": dict(seed=107, nviews=2, node_size=10 ** 6, outliers=0.3, npts=320),
    "duplicates-3": dict(seed=109, nviews=3, stereo1=0.3, stereo2=0.3, node_size=5, duplicates=True, sigma2=1e12, baselines=(1.0, 4.0), outliers=0.0),
    "mono-stereo-8": dict(seed=108, nviews=8, stereo1=0, stereo2=1, node_size=2, baselines=(0.02, 2.0), npts=200),
}


def suite_scene(name):
    return make_scene(**SUITE[name])
