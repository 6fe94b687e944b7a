"""The host path of Sim3Solver, PnPsolver and Initializer (include/orbp.h) against the reference's own src/Sim3Solver.cc,
src/PnPsolver.cc and src/Initializer.cc, compiled unmodified (oracle/ref/ref_sim3.cc, ref_pnp.cc, ref_init.cc), with no step through
the numpy restatements.  tests/ref_solvers.py runs the library on the very request the reference answered and names its results as
the drivers do; ref_solvers.check() then asserts

  exactly   the draws and mvSets, the RANSAC parameters and thresholds, Normalize's bytes, every inlier flag and count, which set
            wins each walk, CheckRT's flags and nGood, vbTriangulated, Initialize's return value, and every field of the iterate
            transcripts that is not a float value;
  by value  s, R, t, mRi, mti, Tcw, H21i / F21i (unit norm, sign aligned), the motions (as a set), vP3D, the scores and the parallax
            (as its cosine), each within 4 x the spread between the reference's own two arithmetic variants.

Every test that needs the binaries runs from the recorded fixtures as well (tests/golden/solvers/), so the suite checks the same
things where the reference is absent.

FOUR-POINT EPnP is the library's documented own definition (the basis of the four-dimensional null space of
M^T M is "implementation-defined in the reference and fixed here by decision").  For requests with minSet = 4 the pose of a
hypothesis, the flags that pose gives and the value of a returned Tcw are therefore left out of the comparison
(ref_solvers.basis_decided_fields); the draws, parameters, thresholds and every non-float field of the transcripts stay exact, and
test_four_point_epnp_side_by_side shows the reference's behaviour and the library's."""
import numpy as np
import pytest

import ref_solvers as rs
import sim3_cases as sc

FIXTURES = rs.load_fixtures()
NAMES = [(k, n) for k, n, _ in rs.pinned_requests()]
IDS = ["%s-%s" % kn for kn in NAMES]


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


@pytest.fixture(scope="module")
def reference():
    """{(kind, name): Records} from the binaries, or None where they cannot be had"""
    return rs.pinned_cases()


def run_library(orbx, kind, request, matcher=None):
    return getattr(rs, "lib_" + kind)(orbx, rs.Records(request), matcher)


def expected(kind, records):
    return rs.sim3_reference_as_library(records.by) if kind == "sim3" else records.by


def test_fixtures_cover_the_pinned_cases_and_their_requests_are_current():
    """the recorded requests are the ones pinned_requests() builds today: a changed case cannot keep an old answer"""
    reqs = rs.pinned_requests()
    assert sorted(FIXTURES) == sorted((k, n) for k, n, _ in reqs)
    for kind, name, req in reqs:
        assert FIXTURES[(kind, name)][0] == req, (kind, name)
    sizes = {kind: [int(rs.Records(req).one("x1" if kind == "sim3" else "p2d" if kind == "pnp" else "m12").shape[0 if kind != "init" else 1])
                    for k, _, req in reqs if k == kind] for kind in rs.KINDS}
    assert {3, 63, 64, 65, 129} <= set(sizes["sim3"]) and {4, 63, 64, 65, 129} <= set(sizes["pnp"])
    assert {8, 63, 64, 65, 129} <= {rs.ic.BY_NAME[n]["N"] for n in rs.INIT_NAMES}
    assert {c["set_size"] for c in rs.PNP_CASES.values()} == {4, 5, 6, 8}


@pytest.mark.parametrize("kind,name", NAMES, ids=IDS)
def test_library_equals_the_recorded_reference(built, kind, name):
    """from the fixtures alone"""
    req, rsp = FIXTURES[(kind, name)]
    devs = rs.check(kind, run_library(built, kind, req), expected(kind, rs.Records(rsp)), rs.basis_decided_fields(kind, rs.Records(req)))
    print(kind, name, {q: "%.3g of %.3g" % (d, rs.tol(q)) for q, d in devs.items()})


def test_binaries_reproduce_the_fixtures_byte_for_byte(reference):
    if reference is None:
        pytest.skip("no reference checkout: the fixtures stand in")
    for key, (req, rsp) in FIXTURES.items():
        assert reference[key].data == rsp, key


def test_library_equals_the_reference_binaries(built, reference):
    if reference is None:
        pytest.skip("no reference checkout: the fixtures stand in")
    failures = []
    for kind, name, req in rs.pinned_requests():
        try:
            rs.check(kind, run_library(built, kind, req), expected(kind, reference[(kind, name)]), rs.basis_decided_fields(kind, rs.Records(req)))
        except AssertionError as e:
            failures.append((kind, name, str(e)[:300]))
    assert not failures, failures


def test_ubsan_copies_give_the_same_bytes(reference):
    """every request through the UBSan copy of its driver (a stand-alone CPU program).  A report stops the run, except a float-to-int
    conversion out of range, which is printed: the reference's constructors make one at src/Sim3Solver.cc:133 / src/PnPsolver.cc:150
    with their default minInliers whenever N is below it, before the driver's own SetRansacParameters call overwrites the result."""
    if reference is None:
        pytest.skip("no reference checkout")
    reqs = rs.pinned_requests()
    for (kind, name, req), (rc, data, err) in zip(reqs, rs.run_many([(k, r, "_ubsan") for k, _, r in reqs])):
        assert rc == 0 and data == reference[(kind, name)].data, (kind, name, rc, err)
        r = rs.Records(req)
        small = (kind == "sim3" and r.one("x1").shape[0] < 6) or (kind == "pnp" and r.one("p2d").shape[0] < 8)
        lines = [ln for ln in err.splitlines() if "runtime error" in ln]
        if small:
            want = "Sim3Solver.cc:133" if kind == "sim3" else "PnPsolver.cc:150"
            assert len(lines) == 1 and want in lines[0], (kind, name, err)
        else:
            assert not lines, (kind, name, err)


def test_reference_variants_agree_on_every_exact_field():
    """the cap on the cases: zero exceptions.  Needs the B variants (make -C oracle/ref measure)"""
    if not rs.ensure(allow_build=True, variants=("", "_ubsan", "_b")):
        pytest.skip("no reference checkout")
    spreads, disagreements = rs.measure_spreads()
    assert not disagreements, disagreements
    for q, m in spreads.items():
        assert m <= rs.SPREADS[q], "%s: measured spread %.3e above the constant %.1e" % (q, m, rs.SPREADS[q])


def test_requests_without_a_defined_answer_are_refused():
    if not rs.ensure():
        pytest.skip("no reference checkout")
    few = dict(rs.ic.BY_NAME["plane8"])
    few["matches12"] = few["matches12"].copy()
    few["matches12"][np.flatnonzero(few["matches12"] >= 0)[0]] = -1                 # seven matches
    jobs = [("sim3", rs.sim3_request(sc.BY_NAME["n19_fix"], 5, 20), ""), ("sim3", rs.sim3_request(sc.BY_NAME["n0_free"], 5, 20), ""),
            ("pnp", rs.pnp_request(rs.PNP_CASES["p4_s4"], 2, (0.99, 10, 300, 4, 0.5, 5.991), 5, 10), ""),
            ("init", rs.init_request(few, 200, 0), ""), ("init", rs.init_request(rs.ic.BY_NAME["plane8"], 0, 0), "")]
    for (kind, _, _), (rc, data, err) in zip(jobs, rs.run_many(jobs)):
        assert rc == 2 and data == b"" and ("ref_" + kind) in err, (kind, rc, err)


# ---- the library's deliberate differences, side by side with the reference

def test_sim3_bnomore_comes_one_call_earlier_when_the_last_iteration_returns_a_pose(built):
    """with mRansacMaxIts = k0 + 1 the first all-inlier triple is the last allowed iteration.  The reference returns
    the pose with bNoMore false and says bNoMore on the next call, which iterates nothing; the library says it with the pose."""
    req, rsp = FIXTURES[("sim3", "run_n64_fix_last")]
    ref = rs.Records(rsp).by
    lib = run_library(built, "sim3", req)
    maxits = int(ref["maxits"][0][0, 0])
    got_r, nm_r, it_r = ([int(a[0, 0]) for a in ref[t]] for t in ("got", "nomore", "iters"))
    got_l, nm_l, it_l = ([int(a[0, 0]) for a in lib[t]] for t in ("got", "nomore", "iters"))
    assert len(got_r) == len(got_l) + 1
    assert (got_r[-2], nm_r[-2], it_r[-2]) == (1, 0, maxits) and (got_r[-1], nm_r[-1], it_r[-1]) == (0, 1, maxits)      # the reference
    assert (got_l[-1], nm_l[-1], it_l[-1]) == (1, 1, maxits)                                                          # the library
    assert got_r[:-2] == got_l[:-1] and nm_r[:-2] == nm_l[:-1] and not any(nm_l[:-1])
    assert ref["rinl"][-2].tobytes() == lib["rinl"][-1].tobytes() and not ref["rinl"][-1].any()


def test_the_library_views_supply_every_compared_field(built):
    """compare() walks the tags the library view supplies: every tag of the EXACT and VALUES tables must be among them, but the ones
    ref_solvers.REFERENCE_ONLY names with its reasons"""
    for kind, name in (("sim3", "hyp_n63_free"), ("pnp", "hyp_p65_s6"), ("pnp", "run_p65_s6"), ("init", "plane63")):
        req, rsp = FIXTURES[(kind, name)]
        lib, ref = run_library(built, kind, req), rs.Records(rsp).by
        table = set(rs.EXACT[kind]) | set(rs.VALUES[kind])
        assert set(ref) <= table, (kind, name, set(ref) - table)                    # nothing is recorded that no table names
        missing = (set(ref) & table) - set(lib) - set(rs.REFERENCE_ONLY.get(kind, ()))
        if kind == "pnp" and name.startswith("hyp_"):
            missing -= {"got", "nomore", "rn", "rinl", "T", "iters", "direct"}      # the driver's one-iteration arrangement, not a result
        assert not missing, (kind, name, missing)


def test_four_point_epnp_side_by_side(built):
    """DESIGN.md section 8.  M^T M of a four-point sample has a four-dimensional null space, EPnP's linearisations depend on the basis
    the SVD returns for it, and the library keeps the basis of its own Jacobi.  Side by side on the three four-point cases (exact
    projections, samples without a wrong match): the draws are the same; the reference (both of its arithmetic variants) fits every
    sample, so all of the sample's own points are inliers; the library always returns a rigid motion, fits a share of the samples --
    there it equals the reference within the tolerance -- and ends in another local solution on the rest."""
    shares = {}
    for name in ("hyp_p4_s4", "hyp_p129_s4", "hyp_p8_s4_coplanar"):
        req, rsp = FIXTURES[("pnp", name)]
        assert rs.basis_decided_fields("pnp", rs.Records(req)) == rs.FOUR_POINT_BASIS_FIELDS
        ref, lib = rs.Records(rsp).by, run_library(built, "pnp", req)
        same = 0
        for k in range(len(ref["sample"])):
            sm = ref["sample"][k].reshape(-1)
            assert np.array_equal(lib["sample"][k].reshape(-1), sm) and len(sm) == 4                      # the draws: exact
            assert ref["inl"][k].reshape(-1)[sm].all(), (name, k)                                           # the reference fits its sample
            R = np.asarray(lib["R"][k], np.float64).reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9, (name, k)  # the library: a rigid motion
            close = max(rs.deviation(lib["R"][k], ref["R"][k]), rs.deviation(lib["t"][k], ref["t"][k])) <= rs.tol("pnp_rt")
            flags = np.array_equal(np.asarray(lib["inl"][k]).reshape(-1), ref["inl"][k].reshape(-1))
            assert close <= flags, (name, k)                                                                # where it ends there, the flags agree
            same += close
        shares[name] = (same, len(ref["sample"]))
    print("four-point samples on which the library ends where the reference does:", shares)
    # the recorded shares (finding 1): a change of the library's basis, for better or worse, shows here
    assert shares == {"hyp_p4_s4": (1, 9), "hyp_p129_s4": (1, 3), "hyp_p8_s4_coplanar": (8, 9)}, shares
    # five-, six- and eight-point samples have no such leave
    for (kind, name), (req, _) in FIXTURES.items():
        if kind == "pnp" and int(rs.Records(req).one("ipar").reshape(-1)[3]) != 4:
            assert rs.basis_decided_fields(kind, rs.Records(req)) == ()


def test_sim3_thresholds_are_truncated_in_the_reference_too():
    """9.210 * 1.44 = 13.26 is stored as 13 (mvnMaxError1 is a vector<size_t>): the planted errors 13.1 / 12.9 / 9.1 are an outlier, an
    inlier and an outlier of every hypothesis drawn from the exact points"""
    by = rs.Records(FIXTURES[("sim3", "hyp_thresholds")][1]).by
    assert list(by["err1"][0].reshape(-1)) == [9, 9, 9, 13, 13, 9, 9, 9, 9] and set(by["err2"][0].reshape(-1)) == {118.0}
    flags = [tuple(inl.reshape(-1)[3:6]) for tri, inl in zip(by["tri"], by["inl"]) if not set(tri.reshape(-1)) & {3, 4, 5}]
    # a triple of exact points: 13.1 out and 12.9 in puts the threshold of sigma2 = 1.44 between them, 9.1 out puts that of sigma2 = 1 below
    # 9.1; a thin triple's float32 pose may lose the 12.9 as well, never gain the other two
    assert (0, 1, 0) in flags and set(flags) <= {(0, 1, 0), (0, 0, 0)}
