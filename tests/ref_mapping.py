"""Client of oracle/_ref/ref_mapping: the reference's own src/MapPoint.cc, compiled unmodified behind the stand-ins of
oracle/ref/mapping_standin.h, and on real MapPoint objects from it the reference's own Frame::isInFrustum, KeyFrame::UnprojectStereo /
ComputeSceneMedianDepth and LocalMapping::CreateNewMapPoints / ComputeF12, sliced out of the reference at build time.  The request
and response formats are at the top of oracle/ref/ref_mapping.cc and in oracle/ref/ref_solver_io.h.  This module has the request
builders, the pinned cases of tests/test_reference_pin_mapping_cpu.py and _gpu.py with their plants, the recorded fixtures under
tests/golden/mapping/, and the one tolerance.

Every plant is proved from the inputs (exact float arithmetic, or a margin worked out in float64 that is orders of magnitude above
any rounding) or from the reference's own records, never from the library or its restatements.

The tolerance.  Only x3D from the 4x4 SVD of src/LocalMapping.cc:331 is compared by value: its last bits are
OpenCV's algorithm, not the reference's text.  The measurement is the largest deviation between the reference's own arithmetic variants
C (the pin) and B over the pinned pairs that both accept through the SVD, relative to max(1, |value|); the tolerance is 4 x that and is
recorded in tests/golden/mapping/tolerance.json.  The library's own deviation never enters.  Pairs on which C and B decide differently
are not pinned: tri_pinned() leaves them out, and record_fixtures() asserts that none is left."""
import json
import os
import subprocess
import tempfile

import numpy as np

import frustum_oracle as fo
import mappoint_oracle as mo
import triangulation_oracle as to
from ref_solvers import MAX_PROCS, Records, pack_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mapping")
KINDS = ("mappoint", "frustum", "newpoints")
TIMEOUT = 120          # seconds; no run of a reference program goes without one
FACTOR = 4
f32, f64 = np.float32, np.float64


def exe(variant=""):
    return os.path.join(REF_OUT, "ref_mapping" + variant)


def ensure(allow_build=True, variants=("", "_ubsan")):
    """True when the driver (and the named variants of it) exists, building them when they are missing and the reference exists"""
    need = [exe(v) for v in variants]
    if all(os.path.exists(p) for p in need):
        return True
    if not allow_build:
        return False
    import ref_pin
    if os.path.exists(os.path.join(ref_pin.reference_dir(), "src", "MapPoint.cc")):
        targets = ["mapping"] + (["measure"] if set(variants) - {"", "_ubsan"} else [])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")] + targets)
        return all(os.path.exists(p) for p in need)
    return False


def run(request, variant=""):
    """-> (exit status, response bytes, stderr text) of one driver run on the request bytes"""
    with tempfile.TemporaryDirectory() as d:
        rq, rs = os.path.join(d, "req"), os.path.join(d, "rsp")
        with open(rq, "wb") as f:
            f.write(request)
        p = subprocess.run([exe(variant), rq, rs], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
        data = b""
        if p.returncode == 0:
            with open(rs, "rb") as f:
                data = f.read()
        return p.returncode, data, p.stderr.decode(errors="replace")


def run_many(jobs):
    """jobs: [(request, variant)] -> results of run() in order, at most MAX_PROCS at a time"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(MAX_PROCS, max(1, len(jobs)))) as ex:
        return list(ex.map(lambda j: run(*j), jobs))


def run_ok(request, variant=""):
    rc, data, err = run(request, variant)
    assert rc == 0, err
    return Records(data)


def bits(a):
    """float32 values as bit patterns, every NaN as one pattern"""
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# ================================================================== MapPoint::ComputeDistinctiveDescriptors

DD_SIZES = (1, 2, 3, 16, 17, 64, 65, 256, 257, 513, 700)


def _pop(a, b):
    return mo._POP[np.bitwise_xor(a, b)].sum(axis=-1)


def _distances(D):
    return np.stack([_pop(D, D[i]) for i in range(len(D))])


def medians_by_index(D):
    """-> (lower, upper): per row the sorted distances' element (N-1)//2 and N//2, straight from the definition"""
    S = np.sort(_distances(D), axis=1)
    n = len(D)
    return S[:, (n - 1) // 2], S[:, n // 2]


def _distinct_rows(rng, n, base=None, weight=(18, 40), keep_clear=0):
    """n distinct descriptors: a base with a random set of `weight` bits flipped, none among the first keep_clear bits"""
    base = rng.integers(0, 256, 32, dtype=np.uint8) if base is None else base
    seen, rows = set(), []
    while len(rows) < n:
        flip = np.zeros(256, np.uint8)
        flip[keep_clear + rng.choice(256 - keep_clear, int(rng.integers(*weight)), replace=False)] = 1
        r = base ^ np.packbits(flip, bitorder="little")
        if r.tobytes() not in seen:
            seen.add(r.tobytes())
            rows.append(r)
    return np.stack(rows)


def _tie_point(rng, n, at):
    """n distinct rows; the rows `at` are the base with ONE of its first bits flipped, the others the base with 18..39 of the remaining
    bits flipped.  Every tie row is at distance 2 of the other tie rows and at w + 1 of a row of weight w, so the tie rows' distance
    rows are permutations of one another: equal medians.  dd_points() asserts from the distance matrix that no other row's is as small."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    rows = _distinct_rows(rng, n, base, keep_clear=8)
    for k, i in enumerate(at):
        rows[i] = base
        rows[i, 0] ^= np.uint8(1 << k)
    return rows


def dd_points():
    """[(name, rows uint8 [N, 32], kfbad uint8 [N], mpbad, expected winner among the rows that are not bad or None)]: the observations
    of one MapPoint each, in map order"""
    rng = np.random.default_rng(20240607)
    pts = []
    for n in (1, 2, 3):                                                         # the other sizes of DD_SIZES carry a plant each, below
        rows = _distinct_rows(rng, n, weight=(2, 30))
        pts.append(("n%d" % n, rows, np.zeros(n, np.uint8), 0, None))
    # a tie of the smallest median between the first and the last row: the first wins
    for n in (3, 16, 17, 65, 257):
        pts.append(("tie_first_last_n%d" % n, _tie_point(rng, n, (0, n - 1)), np.zeros(n, np.uint8), 0, 0))
    # a tie between rows of different 256-row blocks (and not the first row of the run)
    pts.append(("tie_blocks_n513", _tie_point(rng, 513, (5, 300, 512)), np.zeros(513, np.uint8), 0, 5))
    pts.append(("tie_blocks_n700", _tie_point(rng, 700, (255, 256, 699)), np.zeros(700, np.uint8), 0, 255))
    # even N on which the lower middle (the reference's 0.5*(N-1)) and the upper middle (N/2) elect different rows
    for n in (4, 16, 64, 256):
        for _ in range(4000):
            off, rows = mo.batch_from_lengths(rng, [n], flips=8)
            if len({r.tobytes() for r in rows}) != n:
                continue
            lo, up = medians_by_index(rows)
            if int(np.argmin(lo)) != int(np.argmin(up)):           # argmin: the first smallest, as :296's strict `<` elects
                pts.append(("even_n%d" % n, rows, np.zeros(n, np.uint8), 0, int(np.argmin(lo))))
                break
        else:
            raise AssertionError("no even-N plant found for N = %d" % n)
    # bad key frames interleaved with good ones; the tie rows stay good
    for n, good in ((40, 17), (90, 65)):
        kfbad = np.ones(n, np.uint8)
        keep = np.sort(rng.choice(np.arange(2, n - 1), good - 2, replace=False))
        kfbad[keep] = 0
        kfbad[0] = kfbad[n - 1] = 0
        kfbad[1] = 1
        rows = _distinct_rows(rng, n, weight=(18, 40))
        rows[kfbad == 0] = _tie_point(rng, good, (0, good - 1))
        pts.append(("bad_interleaved_n%d" % n, rows, kfbad, 0, 0))
    # nothing to choose from: the descriptor stays what it was
    rows = _distinct_rows(rng, 5)
    pts.append(("all_keyframes_bad", rows, np.ones(5, np.uint8), 0, None))
    pts.append(("point_bad", rows, np.zeros(5, np.uint8), 1, None))
    pts.append(("no_observations", rows[:0], np.zeros(0, np.uint8), 0, None))
    # all rows equal (any index is the same descriptor), and a distance of 256
    pts.append(("all_equal_n17", np.repeat(rows[:1], 17, axis=0), np.zeros(17, np.uint8), 0, None))
    a = rows[0]
    pts.append(("distance_256", np.stack([a, ~a]), np.zeros(2, np.uint8), 0, 0))
    pts.append(("distance_256_n3", np.stack([~a, a, a ^ np.uint8(1)]), np.zeros(3, np.uint8), 0, 1))
    for name, rows, kfbad, mpbad, want in pts:                                  # the proofs, from the distance matrix alone
        good = rows[kfbad == 0]
        if want is not None:
            lo, _ = medians_by_index(good)
            assert lo[want] == lo.min() and not (lo[:want] == lo.min()).any(), name
            assert (good == good[want]).all(1).sum() == 1, name
        if name.startswith(("tie", "bad_interleaved")):
            assert (lo == lo.min()).sum() >= 2, name
        if name.startswith(("tie_first_last", "bad_interleaved")):
            assert lo[len(good) - 1] == lo.min(), name
    assert _pop(pts[-2][1][0], pts[-2][1][1]) == 256
    assert set(DD_SIZES) <= {int((p[2] == 0).sum()) for p in pts}
    return pts


DD_INIT = np.arange(32, dtype=np.uint8) * 7 + 3          # mDescriptor before the call: no row of any point


def dd_request(points):
    off = np.zeros(len(points) + 1, np.int32)
    off[1:] = np.cumsum([len(p[1]) for p in points])
    desc = np.concatenate([p[1] for p in points]).reshape(-1, 32) if points else np.zeros((0, 32), np.uint8)
    kfbad = np.concatenate([p[2] for p in points]).astype(np.uint8) if points else np.zeros(0, np.uint8)
    return pack_records([("mode", np.array([1], np.int32)), ("off", off), ("desc", desc.astype(np.uint8)), ("kfbad", kfbad),
                         ("mpbad", np.array([p[3] for p in points], np.uint8)), ("init", np.tile(DD_INIT, (len(points), 1)))])


def dd_library_input(req):
    """The batch as the library takes it: per point the rows vDescriptors holds after :261-267 (bad key frames left out, nothing for a
    bad point).  -> (off int32 [n+1], desc uint8 [rows, 32])"""
    off, desc, kfbad, mpbad = req.one("off").reshape(-1), req.one("desc").reshape(-1, 32), req.one("kfbad").reshape(-1), req.one("mpbad").reshape(-1)
    runs = []
    for p in range(len(off) - 1):
        rows = desc[off[p]:off[p + 1]][kfbad[off[p]:off[p + 1]] == 0]
        runs.append(rows[:0] if mpbad[p] else rows)
    lib_off = np.zeros(len(runs) + 1, np.int32)
    lib_off[1:] = np.cumsum([len(r) for r in runs])
    return lib_off, np.concatenate(runs).reshape(-1, 32)


def dd_check(req, rsp, best):
    """the reference's mDescriptor must be row best[p] of the point's run; best[p] == -1 exactly where the run is empty, and there the
    descriptor is the one the point had"""
    off, desc = dd_library_input(req)
    out = rsp.one("desc").reshape(-1, 32)
    init = req.one("init").reshape(-1, 32)
    best = np.asarray(best)
    assert len(best) == len(off) - 1
    for p in range(len(best)):
        if off[p + 1] == off[p]:
            assert best[p] == -1 and (out[p] == init[p]).all(), p
        else:
            assert 0 <= best[p] < off[p + 1] - off[p], (p, best[p])
            assert (out[p] == desc[off[p] + best[p]]).all(), (p, int(best[p]))


# ================================================================== Frame::isInFrustum

def _exact_rig(bounds, **kw):
    """camera at the origin looking down z with fx = fy = 512 and the principal point at 0: for a point at depth 1 u = 512 * x exactly
    for every float x, because 0*y and 0*z are zeros, the sums with them and with tcw = 0 are exact, invz = 1 and 512 is a power of two"""
    return fo.make_view(np.eye(3), (0.0, 0.0, 0.0), 512.0, 512.0, 0.0, 0.0, 40.0, bounds, **kw)


def _scene(view, P, normal=(0.0, 0.0, 1.0), mf_max=5.0, mf_min=0.01):
    P = np.asarray(P, f32).reshape(-1, 3)
    n = len(P)
    return fo.Scene(view, np.zeros(n, np.uint8), P, np.broadcast_to(np.asarray(normal, f32), (n, 3)).copy(),
                    np.broadcast_to(np.asarray(mf_max, f32), n).copy(), np.broadcast_to(np.asarray(mf_min, f32), n).copy())


def _around(x):
    x = f32(x)
    return [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]


def frustum_cases():
    """name -> (scene, viewingCosLimit, expected flags or None).  Expected flags are worked out from the inputs in exact arithmetic (see
    each plant); tests/test_reference_pin_mapping_cpu.py holds the reference's records to them."""
    cases = {}
    for name, (sc, limit, _) in fo.quirk_cases().items():
        cases["quirk: " + name] = (sc, limit, None)
    # PcZ at -0, +0 and the smallest values of both signs, off the y axis and on it (PcX == 0: u = 0 * inf = NaN).  tcw's z is -0 and x, y
    # are <= 0 where PcZ shall be -0 (0 * -x = -0 and -0 + -0 = -0).  None is in view: PcZ < 0 at -tiny (:283); elsewhere invz is an
    # infinity and u or v is an infinity beyond the bounds -- or NaN, which passes :291, and then v is the infinity
    tiny = f32(1.4e-45)
    view = fo.make_view(np.eye(3), (0.0, 0.0, -0.0), 500.0, 500.0, 320.0, 240.0, 40.0, (0.0, 640.0, 0.0, 480.0))
    P = [[-0.1, -0.2, -0.0], [-0.0, -0.2, -0.0], [-0.1, -0.2, -tiny], [-0.0, -0.2, -tiny]]
    cases["depth: minus zero and minus tiny"] = (_scene(view, P, mf_max=1.0), 0.5, [0, 0, 0, 0])
    P = [[0.1, 0.05, 0.0], [0.0, 0.05, 0.0], [0.1, 0.05, tiny], [0.0, 0.05, tiny]]
    cases["depth: plus zero and plus tiny"] = (_scene(fo._rig(), P, mf_max=1.0), 0.5, [0, 0, 0, 0])
    # u at mnMinX / mnMaxX and one ulp to either side; the same for v.  u = 512 * x exactly (see _exact_rig), v = 512 * y
    b = (16.0, 624.0, 8.0, 472.0)
    us = _around(b[0]) + _around(b[1])
    vs = _around(b[2]) + _around(b[3])
    P = [[u / f32(512), f32(100) / f32(512), 1.0] for u in us] + [[f32(100) / f32(512), v / f32(512), 1.0] for v in vs]
    cases["bounds: u and v on the bounds"] = (_scene(_exact_rig(b), P), 0.5, [0, 1, 1, 1, 1, 0] * 2)
    # dist at 0.8f*mfMinDistance and 1.2f*mfMaxDistance and one ulp to either side: the point (0, 0, z) is z from the origin exactly
    # (sqrt of z*z in double), in an image whose bounds hold u = v = 0
    wide = (-64.0, 64.0, -64.0, 64.0)
    mn, mx = f32(3.7), f32(2.9)
    lo, hi = _around(f32(0.8) * mn), _around(f32(1.2) * mx)
    sc = _scene(_exact_rig(wide), [[0, 0, z] for z in lo + hi], mf_max=[1e3] * 3 + [mx] * 3, mf_min=[mn] * 3 + [1e-3] * 3)
    cases["distance: dist on the two limits"] = (sc, 0.5, [0, 1, 1, 1, 1, 0])
    # viewCos at the limit and one ulp below it: PO = (0, 0, 1), dist = 1, normal (0, 0, c): viewCos = c exactly
    for limit in (0.5, 0.9):
        c = _around(f32(limit))[:2]
        sc = _scene(_exact_rig(wide), [[0, 0, 1]] * 2, mf_max=1.0)
        sc.normal[:, 2] = c
        cases["viewcos: at the limit %.1f" % limit] = (sc, limit, [0, 1])
    # mfMaxDistance / dist at mvScaleFactors[k] and its float neighbours, every k of each pyramid, one of them with a single level
    for i, (sc, _) in enumerate(fo.ceil_boundary_scenes()):
        cases["ceil: pyramid %d" % i] = (sc, 0.5, None)
    view = fo._rig(scale_factor=1.2, nlevels=1)
    sc = fo._points(view, np.tile([0.0, 0.0, 1.0], (5, 1)), normal=[0.0, 0.0, 1.0])
    sc.mf_max, sc.mf_min = np.array(_around(1.0)[1:] + _around(1.2), f32), np.full(5, 0.1, f32)
    cases["ceil: one level"] = (sc, 0.5, [1] * 5)
    # predicted levels below 0 and at or above nlevels: dist = 1, so ratio = mfMaxDistance.  With 12 levels of 1.1, log(0.85) / log(1.1) =
    # -1.7 (1.2 * 0.84 is still >= 1 and passes :302); 1.1^11 = 2.85 is the top level's factor, 4 and 40 lie above it
    view = fo._rig(scale_factor=1.1, nlevels=12)
    sc = fo._points(view, np.tile([0.0, 0.0, 1.0], (4, 1)), normal=[0.0, 0.0, 1.0])
    sc.mf_max, sc.mf_min = np.array([0.85, 0.84, 4.0, 40.0], f32), np.full(4, 0.1, f32)
    cases["level: below 0 and above the top"] = (sc, 0.5, [1] * 4)
    # scenes: n = 0, 1, 63, 64, 65 stereo and monocular, and gates cases of 130 points at both limits
    for k, tag in ((0, "stereo"), (1, "mono")):
        full = fo.suite_scene(k)
        for n in (0, 1, 63, 64, 65):
            cases["scene: %s n=%d" % (tag, n)] = (_noskip(full.head(100 + n)).tail(n) if n else _noskip(full.head(0)), 0.5, None)
    cases["gates: stereo 12 levels, limit 0.9"] = (_noskip(fo.suite_scene(3).head(130)), 0.9, None)
    cases["gates: looking away, limit 0.5"] = (_noskip(fo.suite_scene(2).head(130)), 0.5, None)
    cases["gates: mono, limit 0.9"] = (_noskip(fo.suite_scene(1).head(330)).tail(130), 0.9, None)
    cases["gates: degenerate distances"] = (_noskip(fo.suite_scene(5).head(130)), 0.5, None)
    cases["gates: mfLogScaleFactor = 0"] = (_noskip(fo.suite_scene(4).head(40)), 0.5, None)
    return cases


class _Scene(fo.Scene):
    def tail(self, n):
        return _Scene(self.view, self.skip[len(self) - n:], self.xw[len(self) - n:], self.normal[len(self) - n:], self.mf_max[len(self) - n:],
                      self.mf_min[len(self) - n:])

    def take(self, idx):
        return _Scene(self.view, self.skip[idx], self.xw[idx], self.normal[idx], self.mf_max[idx], self.mf_min[idx])


def _noskip(sc):
    return _Scene(sc.view, np.zeros(len(sc), np.uint8), sc.xw, sc.normal, sc.mf_max, sc.mf_min)


def frustum_request(sc, limit):
    return pack_records([("mode", np.array([2], np.int32)), ("view", np.frombuffer(np.asarray(sc.view, fo.VIEW_DTYPE).tobytes(), np.uint8)),
                         ("limit", np.array([limit], f32)), ("xw", sc.xw.reshape(-1, 3)), ("normal", sc.normal.reshape(-1, 3)),
                         ("mfmax", sc.mf_max), ("mfmin", sc.mf_min)])


def frustum_scene(req):
    """the scene and limit a frustum request holds"""
    view = np.frombuffer(req.one("view").tobytes(), fo.VIEW_DTYPE)[0]
    n = req.one("xw").shape[0]
    return _Scene(view, np.zeros(n, np.uint8), req.one("xw"), req.one("normal"), req.one("mfmax").reshape(-1), req.one("mfmin").reshape(-1)), \
        float(req.scalar("limit"))


def maybe_undefined(sc):
    """Points whose level quotient log(mfMaxDistance / dist) / mfLogScaleFactor (src/MapPoint.cc:410) is not certain from the inputs to
    convert to int: elsewhere mfMaxDistance is finite and positive, dist is positive and finite (a point that reaches :314 has passed
    :302), so |log| < 104, and |mfLogScaleFactor| >= 1e-3 keeps the quotient under 2^17.  The UBSan copy decides about the others."""
    lsf = float(sc.view["log_scale_factor"])
    if not np.isfinite(lsf) or abs(lsf) < 1e-3:
        return np.ones(len(sc), bool)
    with np.errstate(all="ignore"):
        d = fo.distance(sc.view, sc.xw)
        return ~(np.isfinite(sc.mf_max) & (sc.mf_max > 0) & np.isfinite(d) & (d > 0))


CONVERSION = "is outside the range of representable values of type 'int'"


def split_undefined(sc, limit):
    """-> bool [n]: the points on which the reference's UBSan copy reports the int conversion of :410, each asked alone (UBSan reports
    one source line once per process)"""
    cand = np.flatnonzero(maybe_undefined(sc))
    res = run_many([(frustum_request(sc.take([i]), limit), "_ubsan") for i in cand])
    und = np.zeros(len(sc), bool)
    for i, (rc, _, err) in zip(cand, res):
        assert rc == 0, err
        if "runtime error" in err:
            assert CONVERSION in err and "MapPoint.cc:410" in err, err
            und[i] = True
    return und


def frustum_check(fx, got, what):
    """got: orbm_frustum's tuple for the full scene of a fixture; the reference's record holds the defined points"""
    req, rsp, und = Records(fx["req"]), Records(fx["rsp"]), fx["undef"]
    status = np.asarray(got[0])
    assert ((status == fo.UNDEFINED) == und).all(), (what, "undefined", np.flatnonzero((status == fo.UNDEFINED) != und))
    d = ~und
    flag = rsp.one("flag").reshape(-1)
    assert ((status[d] == fo.IN_VIEW) == (flag == 1)).all(), (what, "in view", np.flatnonzero((status[d] == fo.IN_VIEW) != (flag == 1)))
    assert (np.asarray(got[4])[d] == rsp.one("level").reshape(-1)).all(), (what, "level")
    for k, tag in ((1, "projx"), (2, "projy"), (3, "projxr"), (5, "viewcos")):
        bad = np.flatnonzero(bits(np.asarray(got[k])[d]) != bits(rsp.one(tag).reshape(-1)))
        assert len(bad) == 0, (what, tag, bad[:5])
    assert got[6] == int(flag.sum()), (what, "nToMatch")


# ================================================================== CreateNewMapPoints, pairs given

CALIB2 = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, mbf=to.KITTI["mbf"])      # the rig's mbf (:408 reads the current key frame's), another mb


def make_pair2(rng, n, stereo1, stereo2, baseline=0.6, depth=(2.0, 40.0), noise=0.7, outliers=0.12, bad_depth=0.03):
    """triangulation_oracle.make_pair with two different cameras: the current key frame is KITTI's with 8 levels of 1.2, the neighbour a
    640 x 480 camera with 12 levels of 1.1 and another mb.  Octaves are random in each pyramid."""
    R1 = to.rotation(*rng.normal(0, 0.05, 3))
    O1 = rng.normal(0, 20.0, 3)
    R2 = to.rotation(*rng.normal(0, 0.03, 3)) @ R1
    direction = rng.normal(0, 1, 3) * np.array([1.0, 0.2, 1.0])
    O2 = O1 + baseline * direction / np.linalg.norm(direction)
    cam1 = to.make_camera(R1, -R1 @ O1, **to.KITTI)
    cam2 = to.make_camera(R2, -R2 @ O2, scale_factor=1.1, nlevels=12, **CALIB2)
    z = rng.uniform(depth[0], depth[1], n)
    xc = np.stack([(rng.uniform(300, 900, n) - to.KITTI["cx"]) / to.KITTI["fx"] * z, (rng.uniform(40, 330, n) - to.KITTI["cy"]) / to.KITTI["fy"] * z, z], 1)
    Xw = (xc - (-R1 @ O1)) @ R1
    kf1 = to._observe(rng, cam1, Xw, stereo1, noise, bad_depth)
    kf2 = to._observe(rng, cam2, Xw, stereo2, noise, bad_depth)
    kf1.kps_un["octave"] = np.minimum(kf1.kps_un["octave"], 3)
    kf2.kps_un["octave"] = np.minimum(kf2.kps_un["octave"], 5)
    idx2 = np.arange(n)
    swap = np.nonzero(rng.random(n) < outliers)[0]
    idx2[swap] = rng.integers(0, n, len(swap))
    order = rng.permutation(n)
    return cam1, kf1, cam2, kf2, np.stack([order, idx2[order], np.zeros(n, np.int64)], 1).astype(np.int32)


def _feature(cam, X, stereo, depth=None, mbf=None):
    """the exact (float64, rounded once) feature of world point X in cam, on octave 0: (x, y, u_right, depth)"""
    R = cam["Rcw"].reshape(3, 3).astype(f64)
    Xc = R @ np.asarray(X, f64) + cam["tcw"].astype(f64)
    u = float(cam["fx"]) * Xc[0] / Xc[2] + float(cam["cx"])
    v = float(cam["fy"]) * Xc[1] / Xc[2] + float(cam["cy"])
    if not stereo:
        return u, v, -1.0, -1.0
    return u, v, u - float(cam["mbf"] if mbf is None else mbf) / Xc[2], Xc[2] if depth is None else depth


def _keyframe(feats):
    kps = np.zeros(len(feats), to.KP_DTYPE)
    kps["x"], kps["y"] = [f[0] for f in feats], [f[1] for f in feats]
    return to.KeyFrame(kps, np.stack([kps["x"], kps["y"]], 1), [f[2] for f in feats], [f[3] for f in feats])


QUIRK_POINTS = [(0.3, 0.2, 10.0), (-0.5, 0.1, 9.0), (0.8, -0.3, 11.0), (0.1, 0.4, 12.0), (-0.9, -0.2, 10.5), (0.6, 0.3, 9.5)]


def quirk315_case():
    """src/LocalMapping.cc:315 has `else if(bStereo2)`: with both features stereo only the first key frame's depth enters
    cosParallaxStereo.  Cameras one metre apart on x looking down z, fx = 500, mbf = 250 (mb = 0.5); points 9..12 m away seen exactly
    by both.  The first feature carries the true depth: cosParallaxStereo1 = cos(2 atan(0.25 / 10)) = 0.9988.  The rays' parallax is
    about 0.1 rad: cosParallaxRays = 0.995 < 0.9988, so the reference triangulates (:321) and accepts a point that reprojects
    exactly.  The second feature carries a depth of 2 m with a right coordinate that fits the true point: read as a plain `if`,
    cosParallaxStereo2 = cos(2 atan(0.25 / 2)) = 0.969 becomes the minimum, 0.995 < 0.969 fails, :346 unprojects the second feature to a
    fifth of the distance, and that point reprojects about 200 px off in the first key frame: refused at :387.  The margins are asserted."""
    cam1 = to.make_camera(np.eye(3), [0, 0, 0], 500, 500, 320, 240, 250)
    cam2 = to.make_camera(np.eye(3), [-1, 0, 0], 500, 500, 320, 240, 250)
    f1 = [_feature(cam1, X, True) for X in QUIRK_POINTS]
    f2 = [_feature(cam2, X, True, depth=2.0) for X in QUIRK_POINTS]
    for X in QUIRK_POINTS:
        X = np.asarray(X)
        r2 = X - [1, 0, 0]
        cos_rays = X @ r2 / np.linalg.norm(X) / np.linalg.norm(r2)
        cos1, cos2 = np.cos(2 * np.arctan2(0.25, X[2])), np.cos(2 * np.arctan2(0.25, 2.0))
        assert 0 < cos_rays < cos1 - 1e-3 and cos2 < cos_rays - 1e-2            # `else if`: triangulated; `if`: not, and :346 is taken
        near = np.array([1, 0, 0]) + r2 * (2.0 / r2[2])
        assert abs(500 * near[0] / near[2] - 500 * X[0] / X[2]) > 100           # ... to a point 100 px off in key frame 1: 1e4 > 7.8
    n = len(QUIRK_POINTS)
    return cam1, _keyframe(f1), cam2, _keyframe(f2), np.stack([np.arange(n), np.arange(n), np.zeros(n, int)], 1).astype(np.int32)


def quirk408_case():
    """src/LocalMapping.cc:408 subtracts mpCurrentKeyFrame->mbf, not pKF2->mbf, from u2.  Cameras three metres apart, the current one
    with mbf = 250, the neighbour with mbf = 500 (mb = 1); the first feature monocular, the second stereo with the true depth and a
    right coordinate u2 - 250 / z: the reference's errX2_r is 0 and the triangulated point (cosParallaxRays = 0.95 < cosParallaxStereo2 =
    cos(2 atan(0.5 / 10)) = 0.995) is accepted.  Read with pKF2->mbf, u2_r = u2 - 500 / z is 250 / z > 20 px off: 400 > 7.8 * 1, refused."""
    cam1 = to.make_camera(np.eye(3), [0, 0, 0], 500, 500, 320, 240, 250)
    cam2 = to.make_camera(np.eye(3), [-3, 0, 0], 500, 500, 320, 240, 500)
    f1 = [_feature(cam1, X, False) for X in QUIRK_POINTS]
    f2 = [_feature(cam2, X, True, mbf=250.0) for X in QUIRK_POINTS]
    for X in QUIRK_POINTS:
        X = np.asarray(X)
        r2 = X - [3, 0, 0]
        cos_rays = X @ r2 / np.linalg.norm(X) / np.linalg.norm(r2)
        assert 0 < cos_rays < np.cos(2 * np.arctan2(0.5, X[2])) - 1e-2 and (250.0 / X[2]) ** 2 > 50 * 7.8
    n = len(QUIRK_POINTS)
    return cam1, _keyframe(f1), cam2, _keyframe(f2), np.stack([np.arange(n), np.arange(n), np.zeros(n, int)], 1).astype(np.int32)


def two_view_case():
    """two neighbours with different cameras behind one current key frame, the pairs of both interleaved"""
    rng = np.random.default_rng(77)
    cam1, kf1, cam2a, kf2a, ma = to.make_pair(rng, 40, stereo1=0.5, stereo2=0.5, baseline=0.7)
    R2 = to.rotation(0.01, -0.02, 0.015) @ cam1["Rcw"].reshape(3, 3).astype(f64)
    O2 = cam1["Ow"].astype(f64) + np.array([0.5, 0.05, -0.4])
    cam2b = to.make_camera(R2, -R2 @ O2, scale_factor=1.1, nlevels=12, **CALIB2)
    R1 = cam1["Rcw"].reshape(3, 3).astype(f64)
    z = rng.uniform(3, 30, 40)
    xc = np.stack([(kf1.kps_un["x"] - to.KITTI["cx"]) / to.KITTI["fx"] * z, (kf1.kps_un["y"] - to.KITTI["cy"]) / to.KITTI["fy"] * z, z], 1)
    kf2b = to._observe(rng, cam2b, (xc - cam1["tcw"].astype(f64)) @ R1, 0.5, 0.7, 0.03)
    kf2b.kps_un["octave"] = np.minimum(kf1.kps_un["octave"], 7)
    mb = np.stack([np.arange(40), np.arange(40), np.ones(40, int)], 1).astype(np.int32)
    pairs = np.empty((80, 3), np.int32)
    pairs[0::2], pairs[1::2] = ma, mb
    off2, kf2 = to.concat_keyframes([kf2a, kf2b])
    return cam1, kf1, np.stack([cam2a, cam2b]), off2, kf2, pairs


def _neighbour(rng, cam1, kf1, offset, nlevels=8, scale_factor=1.2, calib=None):
    """a neighbour `offset` metres from the current key frame's centre, turned a little, observing points 3 to 30 m down kf1's rays"""
    R1 = cam1["Rcw"].reshape(3, 3).astype(f64)
    R2 = to.rotation(*rng.normal(0, 0.01, 3)) @ R1
    O2 = cam1["Ow"].astype(f64) + np.asarray(offset, f64)
    cam2 = to.make_camera(R2, -R2 @ O2, scale_factor=scale_factor, nlevels=nlevels, **(calib or to.KITTI))
    z = rng.uniform(3, 30, len(kf1))
    xc = np.stack([(kf1.kps_un["x"] - cam1["cx"]) / cam1["fx"] * z, (kf1.kps_un["y"] - cam1["cy"]) / cam1["fy"] * z, z], 1)
    kf2 = to._observe(rng, cam2, (xc - cam1["tcw"].astype(f64)) @ R1, 0.5, 0.5, 0.0)
    kf2.kps_un["octave"] = np.minimum(kf1.kps_un["octave"], nlevels - 1)
    return cam2, kf2


GATE_BASELINES = (0.3, 0.7, 0.54)           # metres; KITTI's mb = mbf / fx = 0.53716
GATE_DEPTHS = (200.0, 10.0, 50.0)           # the neighbour's one MapPoint, in baselines down its optical axis
EXPECTED_GATES = {"gate_baseline": [0, 1, 1], "gate_median_depth": [0, 1, 1]}


def gate_case(stereo):
    """Three neighbours of one current key frame, 12 pairs each, interleaved.  stereo: the request says !mbMonocular and the
    neighbours are 0.3, 0.7 and 0.54 m away: :253 `baseline<pKF2->mb` (0.53716) removes the first and only the first, by margins of
    3e-3 and more.  Otherwise the request says mbMonocular, the neighbours are all 0.7 m away and their one MapPoint lies 200, 10 and 50
    baselines down the optical axis: ratioBaselineDepth = 0.005, 0.1, 0.02 against :261's 0.01 removes the first and only the first."""
    rng = np.random.default_rng(31 if stereo else 32)
    cam1, kf1, _, _, _ = to.make_pair(rng, 12, stereo1=0.5, stereo2=0.5, bad_depth=0.0)
    d = np.array([1.0, 0.1, -0.6])
    d /= np.linalg.norm(d)
    nb = [_neighbour(rng, cam1, kf1, d * (b if stereo else 0.7)) for b in GATE_BASELINES]
    mb = float(cam1["mb"])
    assert all(float(c["mb"]) == mb for c, _ in nb) and GATE_BASELINES[0] < mb - 3e-3 and min(GATE_BASELINES[1:]) > mb + 2e-3
    assert GATE_DEPTHS[0] > 2 / 0.01 - 1 and max(GATE_DEPTHS[1:]) < 0.6 / 0.01
    off2, kf2 = to.concat_keyframes([k for _, k in nb])
    pairs = np.stack([np.tile(np.arange(12), 3), np.tile(np.arange(12), 3), np.repeat(np.arange(3), 12)], 1).reshape(3, 12, 3)
    pairs = pairs.transpose(1, 0, 2).reshape(-1, 3).astype(np.int32)
    return cam1, kf1, np.stack([c for c, _ in nb]), off2, kf2, pairs, 0 if stereo else 1, None if stereo else GATE_DEPTHS


def tri_cases():
    """name -> (cam1, kf1, cams2 [nv], off2, kf2 concatenated, pairs [n, 3]) before the pairs on which the reference's variants decide
    differently are taken out"""
    cases = {}
    rng = np.random.default_rng(4242)
    for s1, s2, tag in ((0.0, 0.0, "mono_mono"), (1.0, 0.0, "stereo_mono"), (0.0, 1.0, "mono_stereo"), (1.0, 1.0, "stereo_stereo")):
        cam1, kf1, cam2, kf2, m = make_pair2(rng, 75, s1, s2)
        cases[tag] = (cam1, kf1, np.stack([cam2]), np.array([0, len(kf2)], np.int32), kf2, m)
    cam1, kf1, cam2, kf2, m = to.make_pair(rng, 75, stereo1=0.5, stereo2=0.5, baseline=0.25, mbf2=200.0)
    cases["mixed_short_baseline"] = (cam1, kf1, np.stack([cam2]), np.array([0, len(kf2)], np.int32), kf2, m)
    cam1, kf1, cam2, kf2, m = to.make_pair(rng, 75, stereo1=0.3, stereo2=0.3, baseline=0.02, noise=0.2)
    cases["low_parallax"] = (cam1, kf1, np.stack([cam2]), np.array([0, len(kf2)], np.int32), kf2, m)
    for name, c in (("zero_distance", to.zero_distance_cases(8)), ("w_zero", to.w_zero_cases(8)), ("quirk315", quirk315_case()),
                    ("quirk408", quirk408_case())):
        cam1, kf1, cam2, kf2, m = c
        cases[name] = (cam1, kf1, np.stack([cam2]), np.array([0, len(kf2)], np.int32), kf2, m)
    cases["two_views"] = two_view_case()
    cases["gate_baseline"] = gate_case(True)
    cases["gate_median_depth"] = gate_case(False)
    return cases


TRI_COUNTS = {"mono_mono": 65, "stereo_mono": 64, "mono_stereo": 63, "stereo_stereo": 65, "mixed_short_baseline": 65, "low_parallax": 64}


def _scene_points(cam1, cams2, depths=None):
    """One MapPoint per neighbour for ComputeSceneMedianDepth (src/KeyFrame.cc:633), ten baselines down the
    neighbour's optical axis: baseline / depth = 0.1 or less, and the request says monocular so that :258-262 is the gate that runs
    and lets every neighbour through as long as baseline / depth >= 0.01"""
    out = []
    for v, c in enumerate(cams2):
        base = np.linalg.norm(c["Ow"].astype(f64) - cam1["Ow"].astype(f64))
        out.append(c["Ow"].astype(f64) + c["Rcw"][6:9].astype(f64) * ((depths[v] if depths else 10) * base if base > 0 else 1.0))
    return np.asarray(out, f32)


def tri_request(cam1, kf1, cams2, off2, kf2, pairs, mono=1, depths=None):
    """depths: per neighbour, how many baselines down its optical axis its one MapPoint lies (10 where None)"""
    raw = lambda a, dt: np.frombuffer(np.ascontiguousarray(a, dt).tobytes(), np.uint8).reshape(-1, dt.itemsize)
    cams2 = np.atleast_1d(np.asarray(cams2, to.CAM_DTYPE))
    return pack_records([
        ("mode", np.array([3], np.int32)), ("mono", np.array([mono], np.int32)), ("cam1", raw(cam1, to.CAM_DTYPE).reshape(-1)),
        ("kps1", raw(kf1.kps_un, to.KP_DTYPE)), ("xy1", kf1.keys_xy), ("ur1", kf1.u_right), ("dep1", kf1.depth),
        ("cams2", raw(cams2, to.CAM_DTYPE)), ("off2", np.asarray(off2, np.int32)), ("kps2", raw(kf2.kps_un, to.KP_DTYPE)),
        ("xy2", kf2.keys_xy), ("ur2", kf2.u_right), ("dep2", kf2.depth), ("scene", _scene_points(cam1, cams2, depths)),
        ("scnidx", np.zeros(len(cams2), np.int32)), ("pairs", np.asarray(pairs, np.int32).reshape(-1, 3))])


def tri_inputs(req):
    """what a newpoints request holds, as triangulation_oracle.triangulate and the library's triangulate_matches take it"""
    cam1 = np.frombuffer(req.one("cam1").tobytes(), to.CAM_DTYPE)[0]
    cams2 = np.frombuffer(req.one("cams2").tobytes(), to.CAM_DTYPE)
    kf = lambda s: to.KeyFrame(np.frombuffer(req.one("kps" + s).tobytes(), to.KP_DTYPE), req.one("xy" + s).reshape(-1, 2), req.one("ur" + s).reshape(-1),
                               req.one("dep" + s).reshape(-1))
    return cam1, kf("1"), cams2, req.one("off2").reshape(-1), kf("2"), req.one("pairs").reshape(-1, 3)


def tri_check(rsp, status, x3d, tol, views=None):
    """the library's (or a restatement's) status and x3d against the reference's record of the same pairs: accepted or not and the
    feature-without-depth status exactly (views: the pairs' view indices; pairs of neighbours the gates removed are left out), unprojected points as bit patterns, triangulated points within tol relative to max(1, |value|).
    -> the largest such deviation"""
    acc, path, ref = rsp.one("acc").reshape(-1), rsp.one("path").reshape(-1), rsp.one("x3d").reshape(-1, 3)
    status, x3d = np.asarray(status), np.asarray(x3d, f32).reshape(-1, 3)
    if views is not None:                                   # pairs of a neighbour that :251-263 removed never reach the per-pair loop: the
        live = rsp.one("gate").reshape(-1)[np.asarray(views)] == 1      # caller hands the library only the neighbours that passed
        assert (acc[~live] == 0).all() and (path[~live] == 0).all(), "a pair of a removed neighbour was processed"
        acc, path, ref, status, x3d = acc[live], path[live], ref[live], status[live], x3d[live]
    ok = status <= to.STEREO2
    assert (ok == (acc == 1)).all(), ("accepted", np.flatnonzero(ok != (acc == 1)), status[ok != (acc == 1)])
    assert ((status == to.UNDEFINED) == (acc == 2)).all(), ("undefined", np.flatnonzero((status == to.UNDEFINED) != (acc == 2)))
    un = ok & (path != 0)
    assert (status[un] == np.where(path[un] == 1, to.STEREO1, to.STEREO2)).all()
    assert (status[ok & (path == 0)] == to.SVD).all()
    assert (bits(x3d[un]) == bits(ref[un])).all(), "UnprojectStereo points differ in bits"
    sv = ok & (path == 0)
    dev = float((np.abs(x3d[sv].astype(f64) - ref[sv]) / np.maximum(1.0, np.abs(ref[sv].astype(f64)))).max()) if sv.any() else 0.0
    assert dev <= tol, (dev, tol)
    return dev


# ================================================================== the pinned requests, the fixtures, the tolerance

def fixture_path(kind):
    return os.path.join(GOLDEN, kind + ".npz")


def load_fixtures():
    """{(kind, name): {"req": request bytes, "rsp": response bytes}} from tests/golden/mapping/; a frustum case also has "full", the
    request of all its points, and "undef", the bool mask of the points on which the reference's int conversion is undefined: "req"
    holds the others"""
    out = {}
    for kind in KINDS:
        if os.path.exists(fixture_path(kind)):
            with np.load(fixture_path(kind)) as z:
                for k in z.files:
                    name, what = k.rsplit("/", 1)
                    out.setdefault((kind, name), {})[what] = z[k].tobytes() if what in ("req", "rsp", "full") else z[k]
    for (kind, name), fx in out.items():
        if kind == "frustum":                               # the file holds "full" and "undef"; "req" follows from them
            sc, limit = frustum_scene(Records(fx["full"]))
            fx["req"] = frustum_request(sc.take(np.flatnonzero(~fx["undef"])), limit)
    return out


def load_tolerance():
    with open(os.path.join(GOLDEN, "tolerance.json")) as f:
        return json.load(f)


def frustum_pinned(cases=None):
    """[(name, full scene, limit, undefined mask, request of the defined points)]; needs the UBSan copy"""
    out = []
    for name, (sc, limit, want) in (cases or frustum_cases()).items():
        sc = _noskip(sc)
        und = split_undefined(sc, limit)
        out.append((name, sc, limit, und, frustum_request(sc.take(np.flatnonzero(~und)), limit)))
    return out


DROPPED = {}            # case -> pairs of it that tri_pinned() last left out because the variants decide them differently


def tri_pinned(variants=("", "_b")):
    """[(name, request)] of the pairs on which the named variants of the reference decide alike, cut to TRI_COUNTS, and the pair counts
    0 and 1 of the first case"""
    out = []
    for name, c in tri_cases().items():
        pairs, extra = c[5], tuple(c[6:])
        res = [run_ok(tri_request(*c), v) for v in variants]
        same = np.ones(len(pairs), bool)
        for r in res[1:]:
            same &= (r.one("acc") == res[0].one("acc")).reshape(-1) & (r.one("path") == res[0].one("path")).reshape(-1)
        keep = pairs[same][:TRI_COUNTS.get(name, len(pairs))]
        assert len(keep) == TRI_COUNTS.get(name, len(keep)), (name, len(keep))
        DROPPED[name] = int((~same).sum())
        out.append((name, tri_request(*c[:5], keep, *extra)))
        if name == "mono_mono":
            out.append((name + "_n0", tri_request(*c[:5], keep[:0])))
            out.append((name + "_n1", tri_request(*c[:5], keep[:1])))
    return out


F12_SPREAD = [0.0]      # measure_tri()'s second measurement: F12 between C and B, relative to the matrix's largest element


def f12_check(rsp, cam1, cams2, f12_of, tol):
    """F12 of every neighbour that passed the gates against the reference's record, relative to the matrix's largest element; zeros where
    the neighbour was removed (ComputeF12 never ran).  f12_of(cam1, cam2) is the function under test.  -> the largest deviation"""
    dev = 0.0
    for v, (g, F) in enumerate(zip(rsp.one("gate").reshape(-1), rsp.one("F12"))):
        if not g:
            assert not F.any()
        if not F.any():                                     # removed, or a degenerate pose whose F12 is all zeros
            continue
        dev = max(dev, float(np.abs(np.asarray(f12_of(cam1, cams2[v]), f64).reshape(-1) - F).max() / np.abs(F).max()))
    assert dev <= tol, (dev, tol)
    return dev


def measure_tri(reqs):
    """-> (spread, disagreements): the largest deviation of x3D between the reference's variants C and B over the pairs both accept through
    the SVD, relative to max(1, |value|), and the pairs on which they decide differently"""
    spread, bad, n = 0.0, [], 0
    F12_SPREAD[0] = 0.0
    for name, req in reqs:
        c, b = run_ok(req, ""), run_ok(req, "_b")
        if not ((c.one("acc") == b.one("acc")).all() and (c.one("path") == b.one("path")).all() and (c.one("gate") == b.one("gate")).all()):
            bad.append(name)
            continue
        for fc, fb in zip(c.one("F12"), b.one("F12")):
            if np.abs(fc).max() > 0:
                F12_SPREAD[0] = max(F12_SPREAD[0], float(np.abs(fc.astype(f64) - fb).max() / np.abs(fc).max()))
        sv = ((c.one("acc") == 1) & (c.one("path") == 0)).reshape(-1)
        if sv.any():
            xc, xb = c.one("x3d")[sv].astype(f64), b.one("x3d")[sv].astype(f64)
            spread = max(spread, float((np.abs(xc - xb) / np.maximum(1.0, np.abs(xc))).max()))
            n += int(sv.sum())
    return spread, bad, n


def record_fixtures():
    """Writes tests/golden/mapping/: the requests, the responses of variant C, the undefined masks, tolerance.json"""
    assert ensure(variants=("", "_ubsan", "_b"))
    os.makedirs(GOLDEN, exist_ok=True)
    pts = dd_points()
    req = dd_request(pts)
    np.savez_compressed(fixture_path("mappoint"), **{"batch/req": np.frombuffer(req, np.uint8), "batch/rsp": np.frombuffer(run_ok(req).data, np.uint8)})
    arrays = {}
    for name, sc, limit, und, req in frustum_pinned():
        arrays[name + "/rsp"] = np.frombuffer(run_ok(req).data, np.uint8)
        arrays[name + "/full"] = np.frombuffer(frustum_request(sc, limit), np.uint8)
        arrays[name + "/undef"] = und
    np.savez_compressed(fixture_path("frustum"), **arrays)
    reqs = tri_pinned()
    spread, bad, n = measure_tri(reqs)
    assert not bad, bad                                     # the allowed share of pairs on which C and B decide differently is zero
    arrays = {}
    for name, req in reqs:
        arrays[name + "/req"] = np.frombuffer(req, np.uint8)
        arrays[name + "/rsp"] = np.frombuffer(run_ok(req).data, np.uint8)
    np.savez_compressed(fixture_path("newpoints"), **arrays)
    tol = dict(quantity="x3D of the 4x4 SVD (src/LocalMapping.cc:331), relative to max(1, |value|)", pairs=n, spread_c_b=spread,
               factor=FACTOR, tolerance=FACTOR * spread,
               f12_quantity="F12 (src/LocalMapping.cc:538-555), relative to the matrix's largest element", f12_spread_c_b=F12_SPREAD[0],
               f12_tolerance=FACTOR * F12_SPREAD[0], pairs_dropped_because_c_and_b_decide_differently=dict(DROPPED))
    with open(os.path.join(GOLDEN, "tolerance.json"), "w") as f:
        json.dump(tol, f, indent=1)
        f.write("\n")
    return tol


# ================================================================== CreateNewMapPoints, the whole loop

LOOP_KINDS = ("loop",)
# name -> (make_scene arguments, mbMonocular, depths of the neighbours' MapPoints in baselines or None)
LOOP_CASES = {
    "mono-1": (dict(seed=201, nviews=1, stereo1=0, stereo2=0, node_size=4, baselines=(0.5, 1.5)), 1, None),
    "stereo-2": (dict(seed=202, nviews=2, stereo1=1, stereo2=1, node_size=3, baselines=(0.8, 3.0)), 0, None),
    "mono-3": (dict(seed=203, nviews=3, stereo1=0, stereo2=0, node_size=6, baselines=(0.2, 3.0)), 1, None),
    "stereo-5": (dict(seed=204, nviews=5, stereo1=0.7, stereo2=0.7, node_size=5, baselines=(0.3, 4.0)), 0, None),     # 0.3 m < mb: :253
    "mono-5": (dict(seed=205, nviews=5, stereo1=0, stereo2=0, node_size=8, baselines=(0.2, 4.0)), 1, (10, 10, 200, 10, 10)),   # :261
}
LOOP_REMOVED = {"stereo-5": [0], "mono-5": [2]}


def loop_scene(name):
    import newmappoints_batch_oracle as nb
    kw, mono, depths = LOOP_CASES[name]
    return nb.make_scene(npts=120, bad_depth=0.0, **kw), mono, depths


def loop_requests(sc, mono, depths):
    """-> (the whole-loop request of ref_newpoints, the request without pairs whose answer by ref_mapping holds the gates and F12)"""
    a = sc.batch_args()
    cam1, cams2, off2 = a[0], a[8], a[10]
    kf1 = to.KeyFrame(a[1], a[2], a[3], a[4])
    kf2 = to.KeyFrame(a[11], a[12], a[13], a[14])
    gate_req = tri_request(cam1, kf1, cams2, off2, kf2, np.zeros((0, 3), np.int32), mono, depths)
    base = [r for r in Records(gate_req).order if r not in ("mode", "pairs", "scnidx")]
    G = Records(gate_req)
    i32 = lambda x: np.ascontiguousarray(x, np.int32).reshape(-1)
    recs = [("mode", np.array([4], np.int32))] + [(t, G.one(t)) for t in base] + [
        ("desc1", a[5]), ("desc2", a[15]), ("has1", np.asarray(a[6], np.uint8)), ("has2", np.asarray(a[16], np.uint8)),
        ("fv1n", i32(a[7][0])), ("fv1o", i32(a[7][1])), ("fv1i", i32(a[7][2])),
        ("fv2v", i32(a[17])), ("fv2n", i32(a[18][0])), ("fv2o", i32(a[18][1])), ("fv2i", i32(a[18][2]))]
    return pack_records(recs), gate_req


def run_loop(request, variant=""):
    with tempfile.TemporaryDirectory() as d:
        rq, rs = os.path.join(d, "req"), os.path.join(d, "rsp")
        with open(rq, "wb") as f:
            f.write(request)
        p = subprocess.run([os.path.join(REF_OUT, "ref_newpoints" + variant), rq, rs], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert p.returncode == 0 and b"runtime error" not in p.stderr, p.stderr.decode(errors="replace")
        with open(rs, "rb") as f:
            return f.read()


def ensure_loop(allow_build=True, variants=("", "_ubsan")):
    need = [os.path.join(REF_OUT, "ref_newpoints" + v) for v in variants]
    if all(os.path.exists(p) for p in need):
        return True
    return ensure(allow_build, variants) and all(os.path.exists(p) for p in need)


def surviving_scene(sc, gate_rsp):
    """the scene of the neighbours that passed :251-263, with the F12 the reference computed, as the caller hands it to the library;
    -> (scene, index of every surviving neighbour in the request)"""
    import newmappoints_batch_oracle as nb
    gate = gate_rsp.one("gate").reshape(-1)
    live = [v for v in range(sc.nviews) if gate[v]]
    pick = lambda xs: [xs[v] for v in live]
    F12 = gate_rsp.one("F12").reshape(-1, 3, 3)[live]
    return nb.Scene(sc.cam1, sc.kf1, sc.desc1, sc.has1, sc.fv1, pick(sc.cams2), pick(sc.kfs2), pick(sc.descs2), pick(sc.has2), pick(sc.fvs2), F12,
                    sc.only_stereo), live


def loop_check(rsp, live, lists, tol):
    """lists: per surviving neighbour (pairs [k, 2], status, x3d) in the loop's order, from the numpy loop or from the replay rule applied to
    the library's dense output.  The accepted ones must be the reference's new MapPoints in the reference's order: neighbour, idx1 and
    idx2 exactly, the position as bits where the status says UnprojectStereo and within tol otherwise.  -> the largest deviation"""
    acc, ref = rsp.one("acc").reshape(-1, 3), rsp.one("x3d").reshape(-1, 3)
    got, gx, gs = [], [], []
    for w, (pairs, st, x) in enumerate(lists):
        ok = st <= to.STEREO2
        got.append(np.concatenate([np.full((int(ok.sum()), 1), live[w], np.int32), pairs[ok]], 1))
        gx.append(np.asarray(x, f32).reshape(-1, 3)[ok])
        gs.append(st[ok])
    got, gx, gs = np.concatenate(got).reshape(-1, 3), np.concatenate(gx).reshape(-1, 3), np.concatenate(gs)
    assert got.shape == acc.shape and (got == acc).all(), ("the accepted list or its order", got.shape, acc.shape)
    un = gs != to.SVD
    assert (bits(gx[un]) == bits(ref[un])).all(), "UnprojectStereo points differ in bits"
    dev = float((np.abs(gx[~un].astype(f64) - ref[~un]) / np.maximum(1.0, np.abs(ref[~un].astype(f64)))).max()) if (~un).any() else 0.0
    assert dev <= tol, (dev, tol)
    return dev


def record_loop_fixtures():
    """tests/golden/mapping/loop.npz; asserts that variants C and B of the reference make the same list on every case"""
    assert ensure_loop(variants=("", "_ubsan", "_b")) and ensure(variants=("", "_b"))
    arrays = {}
    for name in LOOP_CASES:
        sc, mono, depths = loop_scene(name)
        req, gate_req = loop_requests(sc, mono, depths)
        rsp, gate_rsp = run_loop(req), run_ok(gate_req).data
        assert (Records(run_loop(req, "_b")).one("acc") == Records(rsp).one("acc")).all(), name
        assert (run_ok(gate_req, "_b").one("gate") == Records(gate_rsp).one("gate")).all(), name
        assert run_loop(req, "_ubsan") == rsp, name
        for k, v in (("req", req), ("rsp", rsp), ("gate_rsp", gate_rsp)):          # the gate request is the same data without pairs
            arrays[name + "/" + k] = np.frombuffer(v, np.uint8)
    np.savez_compressed(fixture_path("loop"), **arrays)


def load_loop_fixtures():
    out = {}
    with np.load(fixture_path("loop")) as z:
        for k in z.files:
            name, what = k.rsplit("/", 1)
            out.setdefault(name, {})[what] = z[k].tobytes()
    return out
