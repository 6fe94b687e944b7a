"""Client of oracle/_ref/ref_sim3, ref_pnp and ref_init: the reference's own src/Sim3Solver.cc, src/PnPsolver.cc and
src/Initializer.cc, compiled unmodified behind the stand-ins of oracle/ref/solver_standin.h on the OpenCV shim's linear-algebra
layer (oracle/ref/cv_shim/cv_linalg.hpp).  Request and response formats are at the top of each driver (oracle/ref/ref_*.cc) and in
oracle/ref/ref_solver_io.h.  This module has the record reader / writer, the request builders, the pinned case list of
tests/test_reference_pin_solvers_cpu.py and _gpu.py, the recorded fixtures under tests/golden/solvers/, and the tolerances.

Tolerances.  OpenCV's SVD, eigen, inverse and small-product internals are not part of the reference's text; the
shim decides them, in two variants (A, the pin: double decompositions, float products summed in float; B: long double and double).
For every quantity compared by value the measurement is the largest deviation between the two REFERENCE variants over the pinned
cases, relative to max(1, |value|); the tolerance is 4 x that.  The library's own deviation never enters.  tools/measure_ref_solvers.py
re-measures (after `make -C oracle/ref measure`) and prints the table; record_fixtures() asserts that A and B agree on every exactly
compared field of every pinned case."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import initializer_cases as ic
import pnp_cases as pc
import sim3_cases as sc
import sim3_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "solvers")
KINDS = ("sim3", "pnp", "init")
TIMEOUT = 120          # seconds; no run of a reference program goes without one
MAX_PROCS = 16
DTYPES = (np.uint8, np.int32, np.float32, np.float64)

# ---- measured spreads between reference variants A and B over the pinned cases (tools/measure_ref_solvers.py), and the tolerances
SIM3_SRT_SPREAD = 5.2e-5        # 5.126e-05: ms12i, mR12i, mt12i, the returned T12 and GetEstimated*
PNP_RT_SPREAD = 3.9e-4          # 3.819e-04: mRi, mti of single hypotheses (samples without a wrong match)
PNP_TCW_SPREAD = 3.9e-4         # 3.819e-04: the Tcw that iterate returns (Refine over the inliers, or the best hypothesis)
INIT_MATRIX_SPREAD = 2.5e-5     # 2.425e-05: H21i / F21i, unit Frobenius norm, sign aligned
INIT_SCORE_SPREAD = 2.9e-4      # 2.889e-04: CheckHomography / CheckFundamental scores
INIT_MOTION_SPREAD = 6.5e-5     # 6.424e-05: the candidate motions of ReconstructH / ReconstructF (as a set), R21 and t21
INIT_P3D_SPREAD = 2.2e-5        # 2.145e-05: vP3D of CheckRT and of Initialize, at the points flagged good / triangulated
INIT_PARALLAX_SPREAD = 1.8e-7   # 1.779e-07: CheckRT's parallax, compared as its cosine
SPREADS = {"sim3_srt": SIM3_SRT_SPREAD, "pnp_rt": PNP_RT_SPREAD, "pnp_tcw": PNP_TCW_SPREAD, "init_matrix": INIT_MATRIX_SPREAD,
           "init_score": INIT_SCORE_SPREAD, "init_motion": INIT_MOTION_SPREAD, "init_p3d": INIT_P3D_SPREAD,
           "init_parallax": INIT_PARALLAX_SPREAD}
FACTOR = 4


def tol(name):
    return FACTOR * SPREADS[name]


def exe(kind, variant=""):
    return os.path.join(REF_OUT, "ref_%s%s" % (kind, variant))


def ensure(allow_build=True, variants=("", "_ubsan")):
    """True when every driver (and the named variants of it) exists, building them when they are missing and the reference exists"""
    need = [exe(k, v) for k in KINDS for v in variants]
    if all(os.path.exists(p) for p in need):
        return True
    if not allow_build:
        return False
    import ref_pin
    if os.path.exists(os.path.join(ref_pin.reference_dir(), "src", "Sim3Solver.cc")):
        targets = ["solvers"] + (["measure"] if "_b" in variants else [])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")] + targets)
        return all(os.path.exists(p) for p in need)
    return False


# ---- records

def pack_records(recs):
    out = []
    for tag, a in recs:
        a = np.asarray(a)
        if a.dtype not in DTYPES:
            raise ValueError("record %s has dtype %s" % (tag, a.dtype))
        a2 = a.reshape(1, a.size) if a.ndim < 2 else a.reshape(a.shape[0], int(np.prod(a.shape[1:])))
        out.append(struct.pack("<8siii", tag.encode(), DTYPES.index(a.dtype), a2.shape[0], a2.shape[1]) + np.ascontiguousarray(a2).tobytes())
    return b"".join(out)


class Records:
    """An ordered record file: r[tag] is the list of that tag's arrays (the k-th belongs to the k-th group), r.one(tag) the only one"""

    def __init__(self, data):
        self.data = bytes(data)
        self.by = {}
        self.order = []
        off = 0
        while off < len(self.data):
            tag, dt, rows, cols = struct.unpack_from("<8siii", self.data, off)
            off += 20
            n = rows * cols * np.dtype(DTYPES[dt]).itemsize
            a = np.frombuffer(self.data, DTYPES[dt], rows * cols, off).reshape(rows, cols)
            off += n
            tag = tag.rstrip(b"\0").decode()
            self.by.setdefault(tag, []).append(a)
            self.order.append(tag)
        assert off == len(self.data)

    def __getitem__(self, tag):
        return self.by[tag]

    def __contains__(self, tag):
        return tag in self.by

    def one(self, tag):
        v = self.by[tag]
        assert len(v) == 1, tag
        return v[0]

    def scalar(self, tag, k=None):
        v = self.by[tag]
        if k is None:
            assert len(v) == 1, tag
            k = 0
        return v[k].reshape(-1)[0]


def run(kind, request, variant=""):
    """-> (exit status, response bytes, stderr text) of one driver run on the request bytes"""
    with tempfile.TemporaryDirectory() as d:
        rq, rs = os.path.join(d, "req"), os.path.join(d, "rsp")
        with open(rq, "wb") as f:
            f.write(request)
        p = subprocess.run([exe(kind, variant), rq, rs], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
        data = b""
        if p.returncode == 0:
            with open(rs, "rb") as f:
                data = f.read()
        return p.returncode, data, p.stderr.decode(errors="replace")


def run_many(jobs):
    """jobs: [(kind, request, variant)] -> results of run() in order, at most MAX_PROCS at a time"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(MAX_PROCS, max(1, len(jobs)))) as ex:
        return list(ex.map(lambda j: run(*j), jobs))


# ---- requests

def sim3_request(case, step, min_inliers=sc.MIN_INLIERS, max_its=sc.MAX_ITERATIONS, max_calls=400, prob=sc.PROBABILITY):
    return pack_records([
        ("x1", case["x1"].astype(np.float32)), ("x2", case["x2"].astype(np.float32)),
        ("sig1", case["sigma2_1"].astype(np.float32)), ("sig2", case["sigma2_2"].astype(np.float32)),
        ("K1", np.asarray(case["K1"], np.float32)), ("K2", np.asarray(case["K2"], np.float32)),
        ("prob", np.array([prob], np.float64)),
        ("ipar", np.array([int(case["fix"]), case["seed"], min_inliers, max_its, step, max_calls], np.int32))])


def pnp_request(case, mode, params, step=1, max_calls=9):
    prob, min_inliers, max_its, min_set, eps, th2 = params
    return pack_records([
        ("p2d", case["p2d"].astype(np.float32)), ("sig2", case["sigma2"].astype(np.float32)), ("p3d", case["p3d"].astype(np.float32)),
        ("K", np.asarray(case["K"], np.float32)), ("prob", np.array([prob], np.float64)), ("fpar", np.array([eps, th2], np.float32)),
        ("ipar", np.array([case["seed"], min_inliers, max_its, min_set, mode, step, max_calls], np.int32))])


def init_request(case, iterations=ic.ITERATIONS, n_per_set=0):
    return pack_records([
        ("keys1", case["keys1"].astype(np.float32)), ("keys2", case["keys2"].astype(np.float32)),
        ("m12", case["matches12"].astype(np.int32)), ("K", np.asarray(ic.K, np.float32)), ("sigma", np.array([ic.SIGMA], np.float32)),
        ("ipar", np.array([case["seed"], iterations, n_per_set], np.int32))])


# ---- the pinned cases

def _threshold_case():
    """test_sim3_cpu.py's hand-derived scene for the integer-truncated thresholds: sigma2 = 1.44 gives 9.210 * 1.44 = 13.26 -> 13, so a
    reprojection error of 13.1 is an outlier and 12.9 an inlier; sigma2 = 1 gives 9 and 9.1 is an outlier.  Three more exact points so
    that three draws exist besides the planted ones."""
    rng = np.random.default_rng(11)
    scale, R, t = 1.3, so.rodrigues(np.array([0.1, -0.2, 0.15])), np.array([0.2, -0.1, 0.05])
    x2 = np.stack([rng.uniform(-2, 2, 9), rng.uniform(-1, 1, 9), rng.uniform(4, 8, 9)], 1)
    x1 = scale * (x2 @ R.T) + t
    for k, e in enumerate((13.1, 12.9, 9.1)):
        x1[3 + k, 0] += np.sqrt(e) / float(sc.K1[0]) * x1[3 + k, 2]
    s144 = np.float32(1.2) * np.float32(1.2)
    sig1 = np.array([1, 1, 1, s144, s144, 1, 1, 1, 1], np.float32)
    return dict(name="thresholds", N=9, seed=7, fix=False, x1=x1.astype(np.float32), x2=x2.astype(np.float32), sigma2_1=sig1,
                sigma2_2=np.full(9, np.float32(1.2) ** 14, np.float32), K1=sc.K1, K2=sc.K2, planted_errors=(13.1, 12.9, 9.1))


SIM3_THRESHOLDS = _threshold_case()
SIM3_HYP_ITS = 24          # hypotheses recorded per case: one iterate(1) call each


# PnP scenes for the pin: points at 4-20 m (the conditioning of pnp_cases.ORACLE), exact projections, a tenth of the matches wrong
# from N = 63 on.  The seeds are the first from 3000 (4000 for four-point samples) for which the recorded samples hold no wrong match
# and the two reference variants agree on every flag: a sample with a wrong match has no pose to find, EPnP's Gauss-Newton ends
# wherever the SVD's basis starts it, and the variants part on about one such sample in five.
# FOUR-POINT SAMPLES: M^T M of four points has a four-dimensional null space and EPnP's answer depends on the basis the SVD returns for
# it; on about half of all four-point samples of the N = 63 / 129 scenes the two variants end in different local solutions (DESIGN.md
# section 2, findings).  The four-point cases here are those on which both variants agree: N = 4, the all-coplanar N = 8, and three
# samples of an N = 129 scene; no N = 63 scene with three agreeing, converging four-point samples was found in 3000 seeds.
PNP_CASES = {c["name"]: c for c in [
    pc.make_case("p4_s4", 4, 4, 2004, zmax=20.0), pc.make_case("p5_s5", 5, 5, 2005, zmax=20.0), pc.make_case("p8_s6", 8, 6, 2006, zmax=20.0),
    pc.make_case("p8_s8", 8, 8, 2008, zmax=20.0), pc.make_case("p63_s8", 63, 8, 3014, wrong=6, zmax=20.0),
    pc.make_case("p64_s5", 64, 5, 3014, wrong=6, zmax=20.0), pc.make_case("p65_s6", 65, 6, 3014, wrong=6, zmax=20.0),
    pc.make_case("p129_s8", 129, 8, 3014, wrong=12, zmax=20.0), pc.make_case("p129_s4", 129, 4, 4019, wrong=12, zmax=20.0),
    pc.make_case("p8_s4_coplanar", 8, 4, 77, planar_first=8, zmin=20.0, zmax=40.0)]}
PNP_HYP_CALLS = {"p4_s4": 9, "p5_s5": 9, "p8_s6": 9, "p8_s8": 9, "p8_s4_coplanar": 9, "p129_s4": 3}    # hypotheses recorded per case (default 5)
PNP_RUNS = ("p4_s4", "p8_s8", "p64_s5", "p65_s6", "p129_s8")
assert (PNP_CASES["p8_s4_coplanar"]["p3d"][:, 2] == 0).all()


def pnp_params(case, reloc=False):
    """SetRansacParameters' arguments: Relocalization's (Tracking.cc:1393) for the transcripts where N allows, else the solver's minimum"""
    if reloc and case["N"] >= 20:
        return (0.99, 10, 300, case["set_size"], 0.5, 5.991)
    return (0.99, case["set_size"], 300, case["set_size"], 0.5, 5.991)


INIT_NAMES = ("plane8", "general8", "plane63", "general63", "plane64", "general64", "plane65", "general65", "plane129", "general129",
              "rotation129", "few63")
INIT_PER_SET = 12          # sets recorded one by one per case


def pinned_requests():
    """[(kind, name, request bytes)] of every pinned case, in a fixed order"""
    out = []
    for name, mi in (("n3_free", 3), ("n3_fix", 3), ("n63_free", 20), ("n64_fix", 20), ("n65_free", 20), ("n129_fix", 20), ("n129_free", 20)):
        out.append(("sim3", "hyp_" + name, sim3_request(sc.BY_NAME[name], 1, mi, SIM3_HYP_ITS, SIM3_HYP_ITS + 1)))
    out.append(("sim3", "hyp_thresholds", sim3_request(SIM3_THRESHOLDS, 1, 3, SIM3_HYP_ITS, SIM3_HYP_ITS + 1)))
    for name, mi in (("n3_fix", 3), ("n20_free", 20), ("n21_fix", 20), ("n63_free", 20), ("n64_fix", 20), ("n65_free", 20), ("n129_free", 20)):
        out.append(("sim3", "run_" + name, sim3_request(sc.BY_NAME[name], 5, mi)))
    c = sc.BY_NAME["n64_fix"]
    k0 = next(k for k, tri in enumerate(c["triples"]) if not c["outlier"][tri].any())
    out.append(("sim3", "run_n64_fix_last", sim3_request(c, 5, 20, k0 + 1)))          # the last allowed iteration returns the pose
    for name, c in PNP_CASES.items():
        out.append(("pnp", "hyp_" + name, pnp_request(c, 1, pnp_params(c), 1, PNP_HYP_CALLS.get(name, 5))))
    for name in PNP_RUNS:
        c = PNP_CASES[name]
        out.append(("pnp", "run_" + name, pnp_request(c, 2, pnp_params(c, True), 5, 80)))
    for name in INIT_NAMES:
        out.append(("init", name, init_request(ic.BY_NAME[name], ic.ITERATIONS, INIT_PER_SET)))
    return out


def fixture_path(kind):
    return os.path.join(GOLDEN, "%s.npz" % kind)


def load_fixtures():
    """{(kind, name): (request bytes, response bytes)} from tests/golden/solvers/"""
    out = {}
    for kind in KINDS:
        z = np.load(fixture_path(kind))
        for key in z.files:
            if key.endswith("/req"):
                name = key[:-4]
                out[(kind, name)] = (z[key].tobytes(), z[name + "/rsp"].tobytes())
    return out


def pinned_cases():
    """{(kind, name): Records of the reference's variant-A response}, from the binaries; None when they are absent"""
    if not ensure():
        return None
    reqs = pinned_requests()
    res = run_many([(k, r, "") for k, _, r in reqs])
    out = {}
    for (kind, name, _), (rc, data, err) in zip(reqs, res):
        assert rc == 0, (kind, name, rc, err)
        out[(kind, name)] = Records(data)
    return out


# ---- which fields are exact, and how values are compared

EXACT = {
    "sim3": ("maxits", "mininl", "err1", "err2", "got", "nomore", "rn", "rinl", "iters", "best", "ran", "tri", "ninl", "inl"),
    "pnp": ("maxits", "mininl", "minset", "eps", "maxerr", "got", "nomore", "rn", "rinl", "iters", "best", "sample", "ninl", "inl", "direct"),
    "init": ("ok", "vbTri", "sets", "m1st", "m2nd", "nrand", "nsrand", "pn1", "T1", "pn2", "T2", "Hinl", "Finl", "fHinl", "fHwin", "fFinl", "fFwin",
             "Hret", "Fret", "Hgood", "Fgood", "Hvb", "Fvb"),
}
# Fields of the tables below that only the reference's two variants are compared on, because the library has no call that returns them:
# PnP "best" (mnBestInliers is not in orbp_pnp_get_ransac_state); Initializer "Hret" / "Fret" and "HR21" / "Ht21" / "FR21" / "Ft21"
# (ReconstructH / ReconstructF are not exposed apart from Initialize, whose "ok", "R21", "t21" are compared) and "nsrand" (the
# library never calls srand when it is given a source).  compare() compares the tags the library view supplies; REQUIRED says which must be there.
REFERENCE_ONLY = {"pnp": ("best",), "init": ("Hret", "Fret", "HR21", "Ht21", "FR21", "Ft21", "nsrand")}
VALUES = {
    "sim3": {"s": "sim3_srt", "R": "sim3_srt", "t": "sim3_srt", "T": "sim3_srt", "es": "sim3_srt", "eR": "sim3_srt", "et": "sim3_srt"},
    "pnp": {"R": "pnp_rt", "t": "pnp_rt", "T": "pnp_tcw"},
    "init": {"Hs": "init_matrix", "Fs": "init_matrix", "fH": "init_matrix", "fF": "init_matrix", "Hsc": "init_score", "Fsc": "init_score",
             "fHsc": "init_score", "fFsc": "init_score", "Hmot": "init_motion", "Fmot": "init_motion", "R21": "init_motion", "t21": "init_motion",
             "HR21": "init_motion", "Ht21": "init_motion", "FR21": "init_motion", "Ft21": "init_motion", "vP3D": "init_p3d", "Hp3d": "init_p3d",
             "Fp3d": "init_p3d", "Hpar": "init_parallax", "Fpar": "init_parallax"},
}


def deviation(a, b):
    """max |a - b| / max(1, |b|)"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def unit(M, like=None):
    """each 3x3 of M (rows of 9) scaled to unit Frobenius norm, its sign chosen to agree with `like`"""
    M = np.asarray(M, np.float64).reshape(-1, 9)
    n = np.linalg.norm(M, axis=1, keepdims=True)
    M = M / np.where(n > 0, n, 1)
    if like is not None:
        sgn = np.sign((M * unit(like)).sum(1, keepdims=True))
        M = M * np.where(sgn == 0, 1, sgn)
    return M


def value_deviation(quantity, a, b):
    if quantity == "init_matrix":
        return deviation(unit(a, b), unit(b))
    if quantity == "init_parallax":
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max()) if a.size else 0.0
    return deviation(a, b)


def _match_motions(a, b):
    """the permutation p with a[k] ~ b[p[k]]: the order of the candidate motions follows the signs the SVD gives its singular vectors,
    which OpenCV's internals decide, so motions are compared as a set"""
    a, b = np.asarray(a, np.float64).reshape(-1, 12), np.asarray(b, np.float64).reshape(-1, 12)
    if len(a) != len(b):
        return None
    perm = [int(np.argmin(np.abs(b - m).max(1))) for m in a]
    return perm if sorted(perm) == list(range(len(a))) else None


def _cos_parallax(p):
    """CheckRT's parallax back in cosine space, where it is computed: acos is singular at 1 (and the reference's own acos gives NaN above it)"""
    c = np.cos(np.deg2rad(np.asarray(p, np.float64)))
    return np.where(np.isnan(c), 1.0, c)


def _compare_init_groups(got, ref, devs, bad):
    # Only the model whose route Initialize takes (RH > 0.40, src/Initializer.cc:112-118) is compared motion by motion: the other one is
    # degenerate by the construction of the scenes (an F fitted to a plane, an H to a volume), and initializer_cases.py keeps its
    # margins on the route alone.
    sh, sf = float(ref["fHsc"][0].reshape(-1)[0]), float(ref["fFsc"][0].reshape(-1)[0])
    route = "H" if np.float32(sh) / (np.float32(sh) + np.float32(sf)) > 0.40 else "F"
    for px in (route,):
        if px + "mot" not in got:
            continue
        g, r = got[px + "mot"][0], ref[px + "mot"][0]
        perm = _match_motions(g, r)
        if perm is None:
            bad.append(px + "mot: not the same set of motions")
            continue
        if not len(perm):
            continue
        devs["init_motion"] = max(devs.get("init_motion", 0.0), deviation(g, r[perm]))
        gg, rg = got[px + "good"][0].reshape(-1), ref[px + "good"][0].reshape(-1)[perm]
        gv, rv = got[px + "vb"][0].astype(bool), ref[px + "vb"][0].astype(bool)[perm]
        if not np.array_equal(gg, rg):
            bad.append("%sgood %s != %s" % (px, gg, rg))
        if not np.array_equal(gv, rv):
            bad.append(px + "vb")
            continue
        n1 = gv.shape[1]
        gp, rp = got[px + "p3d"][0].reshape(len(perm), n1, 3), ref[px + "p3d"][0].reshape(len(perm), n1, 3)[perm]
        devs["init_p3d"] = max(devs.get("init_p3d", 0.0), deviation(gp[gv], rp[rv]))
        devs["init_parallax"] = max(devs.get("init_parallax", 0.0),
                                    deviation(_cos_parallax(got[px + "par"][0].reshape(-1)), _cos_parallax(ref[px + "par"][0].reshape(-1)[perm])))


GROUPED = ("Hmot", "Hgood", "Hvb", "Hp3d", "Hpar", "Fmot", "Fgood", "Fvb", "Fp3d", "Fpar")
REQUIRED = {"sim3": ("got", "nomore", "rn", "rinl", "iters", "best", "T"), "pnp": ("maxits", "mininl", "maxerr"),
            "init": ("ok", "vbTri", "sets", "m1st", "m2nd", "pn1", "T1", "pn2", "T2", "Hinl", "Finl", "fHwin", "fFwin", "fHinl", "fFinl", "Hs", "Fs",
                     "Hsc", "Fsc", "Hmot", "Fmot", "Hgood", "Fgood", "Hvb", "Fvb", "Hp3d", "Fp3d", "Hpar", "Fpar", "R21", "t21", "vP3D")}


# DESIGN.md section 8 (written with the solver, before this pin): "the basis of the exactly-null singular vectors of the rank-8 / rank-10
# M^T M of a 4 / 5-point sample [is] implementation-defined in the reference and fixed here by decision ... here: the eigenvectors this
# library's own Jacobi sweep leaves".  For a request whose minSet is 4 the fields that this basis decides are therefore not compared
# with the reference's: the pose of a hypothesis, the flags and count that pose gives, and the value of a returned Tcw.  Everything the
# reference's text decides stays exact there (parameters, thresholds, the draws, and every non-float field of a transcript), and
# test_four_point_epnp_side_by_side shows both behaviours.  Five-point samples need no such leave: they agree.
FOUR_POINT_BASIS_FIELDS = ("R", "t", "ninl", "inl", "T")


def basis_decided_fields(kind, req):
    """the fields of this request's answer that the library's documented choice of null-space basis decides (none unless PnP, minSet 4)"""
    if kind == "pnp" and int(req.one("ipar").reshape(-1)[3]) == 4:
        return FOUR_POINT_BASIS_FIELDS
    return ()


def compare(kind, got, ref, leave=()):
    """got, ref: {tag: [arrays]} (Records.by, or a library view) -> ({quantity: deviation}, [exact fields that differ]).  Every tag of
    `got` is compared, but those in `leave` (basis_decided_fields); the tags of REQUIRED must be there."""
    devs, bad = {}, []
    got = {t: v for t, v in got.items() if t not in leave}
    for tag in REQUIRED[kind]:
        if tag not in got:
            bad.append("missing " + tag)
    for tag in got:
        if tag not in ref or len(got[tag]) != len(ref[tag]):
            bad.append("%s: %d records for %d" % (tag, len(got[tag]), len(ref.get(tag, ()))))
    if bad:
        return devs, bad
    for tag in EXACT[kind]:
        if tag in got and tag not in GROUPED:
            for k, (x, y) in enumerate(zip(got[tag], ref[tag])):
                x, y = np.asarray(x), np.asarray(y)
                if x.size != y.size or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                    bad.append("%s[%d]" % (tag, k))
    for tag, q in VALUES[kind].items():
        if tag in got and tag not in GROUPED:
            for k, (x, y) in enumerate(zip(got[tag], ref[tag])):
                x, y = np.asarray(x), np.asarray(y)
                if x.size != y.size:
                    bad.append(tag + " size")
                elif tag == "vP3D":
                    on = np.asarray(ref["vbTri"][0]).reshape(-1).astype(bool)
                    devs[q] = max(devs.get(q, 0.0), deviation(x.reshape(-1, 3)[on], y.reshape(-1, 3)[on]))
                else:
                    devs[q] = max(devs.get(q, 0.0), value_deviation(q, x, y))
    if kind == "init":
        _compare_init_groups(got, ref, devs, bad)
    return devs, bad


def compare_variants(kind, ra, rb):
    return compare(kind, ra.by, rb.by)


def check(kind, got, ref, leave=()):
    """asserts that `got` equals `ref` in every exact field and is within the measured tolerances elsewhere; returns the deviations"""
    devs, bad = compare(kind, got, ref, leave)
    assert not bad, bad
    for q, d in devs.items():
        assert d <= tol(q), "%s deviates by %.3g, tolerance %.3g (4 x the spread of the reference's own variants)" % (q, d, tol(q))
    return devs


# ---- the library, run the way the drivers run the reference: the same requests, the same record names

def _bits(flags, width=None):
    f = np.asarray(flags).astype(np.uint8).reshape(-1)
    return np.packbits(f, bitorder="little")


def sim3_reference_as_library(ref):
    """DESIGN.md section 18's deliberate definition: the library sets bNoMore on the call that reaches mRansacMaxIts also when that call
    returns a pose; the reference reports it one call later, on a call that iterates nothing.  -> the reference's groups with that
    last empty call folded into the one before it (a copy; unchanged when the transcript does not end that way)"""
    by = {k: list(v) for k, v in ref.items()}
    n = len(by["got"])
    maxits = int(by["maxits"][0].reshape(-1)[0])
    if n >= 2 and int(by["got"][-1].reshape(-1)[0]) == 0 and int(by["got"][-2].reshape(-1)[0]) == 1 and int(by["nomore"][-2].reshape(-1)[0]) == 0 \
            and int(by["iters"][-2].reshape(-1)[0]) == maxits == int(by["iters"][-1].reshape(-1)[0]):
        for tag in by:
            if len(by[tag]) == n:
                by[tag] = by[tag][:-1]
        by["nomore"][-1] = np.array([[1]], np.int32)
    return by


class CountedLcg:
    def __init__(self, seed):
        self.lcg, self.calls = sc.Lcg(seed), 0

    def __call__(self):
        self.calls += 1
        return self.lcg()


def _i(v):
    return np.array([[int(v)]], np.int32)


def _f(v):
    return np.array([[v]], np.float32)


def lib_sim3(orbx, req, matcher=None):
    """The library on a ref_sim3 request -> {tag: [arrays]}.  With a matcher every hypothesis comes from ONE orbm_sim3_hypotheses call
    (Sim3Solver.EvaluateAll) and the iterations are replays; without one they are the host path."""
    x1, x2 = req.one("x1"), req.one("x2")
    fix, seed, min_inliers, max_its, step, max_calls = [int(v) for v in req.one("ipar").reshape(-1)]
    s = orbx.Sim3Solver(x1, x2, req.one("sig1").reshape(-1), req.one("sig2").reshape(-1), req.one("K1").reshape(-1), req.one("K2").reshape(-1),
                        bool(fix), rand=sc.Lcg(seed), rand_max=sc.RAND_MAX)
    s.SetRansacParameters(float(req.one("prob")[0, 0]), min_inliers, max_its)
    st = s.ransac_state()
    e1, e2 = s.max_errors()
    v = {"maxits": [_i(st["max_its"])], "mininl": [_i(st["min_inliers"])], "err1": [e1.astype(np.float64)], "err2": [e2.astype(np.float64)]}
    results = None
    if matcher is not None:
        s.draw(st["max_its"])
        results = matcher.sim3_hypotheses([s])[0]
        s.attach_results(*results)
    N = len(x1)
    add = lambda tag, a: v.setdefault(tag, []).append(np.asarray(a))
    for _ in range(max_calls):
        if step == 1:
            k = s.ransac_state()["iterations"]
            if matcher is None:
                tri = s.draw(1)
                hyp = s.hypothesis(tri[0]) if len(tri) else None
            else:
                q = s.queued()
                tri = q[:1]
                hyp = None
                if len(q):
                    cnt, sRt, masks = results
                    bits = np.unpackbits(np.ascontiguousarray(masks[k]).view(np.uint8), bitorder="little")[:N].astype(bool)
                    hyp = (sRt[k, 1:10].reshape(3, 3), sRt[k, 10:13], np.float32(sRt[k, 0]), bits, int(cnt[k]))
        T, no_more, flags, n = s.iterate(step)
        st = s.ransac_state()
        add("got", _i(T is not None)); add("nomore", _i(no_more)); add("rn", _i(n)); add("rinl", flags.astype(np.uint8))
        add("T", np.zeros((4, 4), np.float32) if T is None else T.astype(np.float32))
        add("iters", _i(st["iterations"])); add("best", _i(st["best_inliers"]))
        est = s.estimated()
        add("es", _f(est[2] if est else 0)); add("eR", est[0] if est else np.zeros((3, 3), np.float32)); add("et", est[1] if est else np.zeros(3, np.float32))
        if step == 1:
            ran = hyp is not None
            add("ran", _i(ran)); add("tri", tri[0].astype(np.int32) if ran else np.zeros(3, np.int32))
            add("ninl", _i(hyp[4] if ran else 0)); add("inl", (hyp[3] if ran else np.zeros(N, bool)).astype(np.uint8))
            add("s", _f(hyp[2] if ran else 0)); add("R", np.asarray(hyp[0], np.float32) if ran else np.zeros((3, 3), np.float32))
            add("t", np.asarray(hyp[1], np.float32) if ran else np.zeros(3, np.float32))
        if no_more:
            break
    return v


def lib_pnp(orbx, req, matcher=None):
    """The library on a ref_pnp request -> {tag: [arrays]}.  Mode 1 gives the hypothesis fields (sample, R, t, ninl, inl) of as many
    draws as the request has calls; mode 2 the iterate(step) transcript.  With a matcher the hypotheses come from orbm_pnp_hypotheses."""
    p2d, sig2, p3d, K = req.one("p2d"), req.one("sig2").reshape(-1), req.one("p3d"), [float(x) for x in req.one("K").reshape(-1)]
    seed, min_inliers, max_its, min_set, mode, step, max_calls = [int(x) for x in req.one("ipar").reshape(-1)]
    prob, (eps, th2) = float(req.one("prob")[0, 0]), [float(x) for x in req.one("fpar").reshape(-1)]
    N = len(p2d)
    s = orbx.PnPsolver(p2d, sig2, p3d, *K, rand=sc.Lcg(seed), rand_max=sc.RAND_MAX)
    s.SetRansacParameters(prob, min_inliers, max_its, min_set, eps, th2)
    st = s.ransac_state()
    v = {"maxits": [_i(st["max_its"])], "mininl": [_i(st["min_inliers"])], "minset": [_i(s.min_set)], "eps": [_f(st["epsilon"])],
         "maxerr": [s.max_errors().astype(np.float32)]}
    add = lambda tag, a: v.setdefault(tag, []).append(np.asarray(a))
    if mode == 1:
        s.SetRansacParameters(prob, N, 1, min_set, eps, th2)          # one iteration per iterate(1) call, as the driver arranges
        for _ in range(max_calls):
            sm = s.draw(1)
            assert len(sm) == 1
            if matcher is None:
                R, t, inl, n = s.hypothesis(sm[0])
            else:
                cnt, Rt, masks = matcher.pnp_hypotheses([s])[0]
                R, t, n = Rt[0, :9].reshape(3, 3), Rt[0, 9:], int(cnt[0])
                inl = np.unpackbits(np.ascontiguousarray(masks[0]).view(np.uint8), bitorder="little")[:N].astype(bool)
            s.iterate(1)
            add("sample", sm[0].astype(np.int32)); add("R", np.asarray(R, np.float64)); add("t", np.asarray(t, np.float64))
            add("ninl", _i(n)); add("inl", inl.astype(np.uint8))
        return v
    for _ in range(max_calls):
        if matcher is not None:
            orbx.PnPsolver.EvaluateAll([s], matcher, step)
        T, no_more, flags, n = s.iterate(step)
        add("got", _i(T is not None)); add("nomore", _i(no_more)); add("rn", _i(n))
        add("rinl", np.zeros(N, np.uint8) if flags is None else flags.astype(np.uint8))
        add("T", np.zeros((4, 4), np.float32) if T is None else T.astype(np.float32)); add("iters", _i(s.ransac_state()["iterations"]))
        if no_more:
            break
    return v


INIT_RT_GOOD, INIT_RT_GOOD_LOW_PARALLAX = 0, 1       # orbm_init_rt_status (include/orbm.h): the two statuses CheckRT counts


def reduce_check_rt(status, cosp, p3d, first, n1):
    """orbm_init_check_rt's per-match outputs (status [k, N], cos_parallax [k, N], p3d [k, N, 3]) -> CheckRT's own results per motion
    (nGood [k], vbGood [k, n1], vP3D [k, 3 n1], parallax [k]) by src/Initializer.cc:888-904: a counted match writes vP3D at its first
    key, sets vbGood unless its parallax is low, and the parallax is acos of the min(50, nGood - 1)-th smallest cosine, in degrees."""
    k = len(status)
    first = np.asarray(first).reshape(-1)
    good, vb = np.zeros(k, np.int32), np.zeros((k, n1), np.uint8)
    pts, par = np.zeros((k, n1, 3), np.float32), np.zeros(k, np.float32)
    for j in range(k):
        counted = status[j] <= INIT_RT_GOOD_LOW_PARALLAX
        good[j] = int(counted.sum())
        vb[j, first[status[j] == INIT_RT_GOOD]] = 1
        pts[j, first[counted]] = p3d[j][counted]
        if good[j]:
            c = np.sort(cosp[j][counted])
            with np.errstate(invalid="ignore"):
                par[j] = np.float32(np.arccos(np.float64(c[min(50, len(c) - 1)])) * 180 / np.pi)
    return good, vb, pts.reshape(k, 3 * n1), par


def lib_init(orbx, req, matcher=None):
    """The library on a ref_init request -> {tag: [arrays]}.  With a matcher Initialize's hypotheses and CheckRT passes are the two GPU
    calls, the per-set records come from orbm_init_hypotheses and the per-motion CheckRT records from orbm_init_check_rt (reduced by
    reduce_check_rt); without one all of it is the host path."""
    keys1, keys2, m12 = req.one("keys1"), req.one("keys2"), req.one("m12").reshape(-1)
    seed, iterations, n_per = [int(x) for x in req.one("ipar").reshape(-1)]
    rand = CountedLcg(seed)
    it = orbx.Initializer(keys1, req.one("K").reshape(-1), float(req.one("sigma")[0, 0]), iterations, rand=rand, rand_max=sc.RAND_MAX)
    ok, R21, t21, p3d, tri = it.Initialize(keys2, m12, matcher)
    if matcher is not None:
        assert it.LastError() == "", it.LastError()
    sets = it._get()[3]
    first, second = it.matches()
    pn1, T1, pn2, T2 = it.normalized()
    N, n1 = it.N, len(keys1)
    v = {"ok": [_i(ok)], "R21": [R21 if ok else np.zeros((3, 3), np.float32)], "t21": [t21 if ok else np.zeros(3, np.float32)],
         "vP3D": [p3d if ok else np.zeros((n1, 3), np.float32)], "vbTri": [(tri if ok else np.zeros(n1, bool)).astype(np.uint8)],
         "sets": [sets.astype(np.int32)], "m1st": [first.astype(np.int32)], "m2nd": [second.astype(np.int32)], "nrand": [_i(rand.calls)],
         "pn1": [pn1], "T1": [T1], "pn2": [pn2], "T2": [T2]}
    n_per = min(n_per, iterations)
    W = (N + 7) // 8
    if matcher is not None and n_per:
        sm, cnt, masks = matcher.init_hypotheses([it])[0]              # the H of every set, then the F
    for px, model in (("H", 0), ("F", 1)):
        Ms, scs, inls = np.zeros((n_per, 9), np.float32), np.zeros(n_per, np.float32), np.zeros((n_per, W), np.uint8)
        for k in range(n_per):
            if matcher is None:
                M, sc_, inl, _ = it.hypothesis(model, sets[k])
            else:
                row = model * iterations + k
                M, sc_ = sm[row, 1:], sm[row, 0]
                inl = np.unpackbits(np.ascontiguousarray(masks[row]).view(np.uint8), bitorder="little")[:N]
            Ms[k], scs[k], inls[k] = np.asarray(M).reshape(9), sc_, _bits(inl)
        v[px + "s"], v[px + "sc"], v[px + "inl"] = [Ms], [scs], [inls]
    for px, model in (("H", 0), ("F", 1)):
        M, score, inl, win = it.find(model)
        v["f%s" % px], v["f%ssc" % px], v["f%swin" % px] = [M], [_f(score)], [_i(win)]
        v["f%sinl" % px] = [(inl if win >= 0 else np.zeros(0, bool)).astype(np.uint8)]
        Rt = it.motions(model, M) if win >= 0 else np.zeros((0, 12), np.float32)
        k = len(Rt)
        good, vb, pts, par = np.zeros(k, np.int32), np.zeros((k, n1), np.uint8), np.zeros((k, 3 * n1), np.float32), np.zeros(k, np.float32)
        if matcher is not None and k:                                  # k_init_check_rt itself, reduced as CheckRT reduces its loop
            uv, K4, th2 = it.check_rt_inputs()
            good, vb, pts, par = reduce_check_rt(*matcher.init_check_rt(uv, inl, K4, th2, Rt), first, n1)
        else:
            for j in range(k):
                good[j], p, g, par[j] = it.check_rt(Rt[j, :9], Rt[j, 9:], inl)
                vb[j], pts[j] = g, p.reshape(-1)
        v[px + "mot"], v[px + "good"], v[px + "vb"], v[px + "p3d"], v[px + "par"] = [Rt], [good], [vb], [pts], [par]
    return v


def measure_spreads():
    """Runs variants A and B on every pinned case -> ({quantity: spread}, [(kind, name, field) exact disagreements])"""
    assert ensure(variants=("", "_ubsan", "_b")), "the reference binaries and their B variants are needed"
    reqs = pinned_requests()
    ra = run_many([(k, r, "") for k, _, r in reqs])
    rb = run_many([(k, r, "_b") for k, _, r in reqs])
    spreads, disagreements = {}, []
    for (kind, name, _), a, b in zip(reqs, ra, rb):
        assert a[0] == 0 and b[0] == 0, (kind, name, a[0], a[2], b[0], b[2])
        devs, bad = compare_variants(kind, Records(a[1]), Records(b[1]))
        disagreements += [(kind, name, f) for f in bad]
        for q, d in devs.items():
            spreads[q] = max(spreads.get(q, 0.0), d)
    return spreads, disagreements


def record_fixtures():
    """Writes tests/golden/solvers/<kind>.npz from variant A, after asserting that A and B agree on every exact field of every case"""
    spreads, disagreements = measure_spreads()
    assert not disagreements, disagreements
    reqs = pinned_requests()
    res = run_many([(k, r, "") for k, _, r in reqs])
    os.makedirs(GOLDEN, exist_ok=True)
    for kind in KINDS:
        arrays = {}
        for (k, name, req), (rc, data, err) in zip(reqs, res):
            if k == kind:
                assert rc == 0, (kind, name, err)
                arrays[name + "/req"] = np.frombuffer(req, np.uint8)
                arrays[name + "/rsp"] = np.frombuffer(data, np.uint8)
        np.savez_compressed(fixture_path(kind), **arrays)
    return spreads
