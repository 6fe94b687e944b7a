"""The host Initializer (orbp_init_* of include/orbp.h, csrc/orbp_init.cc over csrc/orbp_init_body.h) against the fp64 oracle
tests/initializer_oracle.py on the cases of tests/initializer_cases.py.  No GPU: everything here is the library's host path."""
import numpy as np
import pytest

import initializer_cases as ic
import initializer_oracle as O

ACCEPTED = [c["name"] for c in ic.CASES if ic.expect_ok(c)]
REFUSED = [c["name"] for c in ic.CASES if not ic.expect_ok(c)]


def solver(orbx, case, iterations=ic.ITERATIONS, current=True):
    s = orbx.Initializer(case["keys1"], ic.K, ic.SIGMA, iterations, rand=ic.Lcg(case["seed"]), rand_max=ic.RAND_MAX)
    if current:
        assert s.set_current(case["keys2"], case["matches12"]) == case["N"]
    return s


def unit(M, like=None):
    """M / ||M||_F, its sign chosen to agree with `like`"""
    M = np.asarray(M, np.float64)
    M = M / np.linalg.norm(M)
    if like is not None and (M * like).sum() < 0:
        M = -M
    return M


@pytest.mark.parametrize("name", [c["name"] for c in ic.CASES])
def test_draws_equal_the_reference_procedure(orbx, name):
    case = ic.BY_NAME[name]
    for k in ic.HYP_COUNTS:
        s = solver(orbx, case, k)
        got = s.draw()
        assert got.shape == (k, 8) and np.array_equal(got, case["sets"][:k])
        assert all(len(set(row)) == 8 for row in got.tolist())
        first, second = s.matches()
        assert np.array_equal(first, case["first"]) and np.array_equal(second, case["second"])       # mvMatches12 :54-63


def test_default_source_seeds_once_and_draws_with_libc_rand(orbx):
    case = ic.BY_NAME["general64"]
    s = orbx.Initializer(case["keys1"], ic.K, ic.SIGMA, 3)
    s.set_current(case["keys2"], case["matches12"])
    a = s.draw()
    assert a.shape == (3, 8) and (a >= 0).all() and (a < case["N"]).all() and all(len(set(r)) == 8 for r in a.tolist())
    b = s.draw()                                             # SeedRandOnce: no second srand(0), the sequence goes on
    assert not np.array_equal(a, b)


def test_normalize_is_the_float_sum_in_key_order(orbx, capsys):
    worst = 0.0
    for case in ic.CASES:
        s = solver(orbx, case)
        pn1, T1, pn2, T2 = s.normalized()
        for keys, pn, T in ((case["keys1"], pn1, T1), (case["keys2"], pn2, T2)):
            want_pn, want_T = O.normalize_f32(keys)          # over ALL keys of the frame, matched or not
            assert pn.tobytes() == want_pn.tobytes() and T.tobytes() == want_T.tobytes(), case["name"]
            d_pn, d_T = O.normalize(keys)
            for a, b in ((pn, d_pn), (T, d_T)):
                worst = max(worst, float((np.abs(a - b) / np.maximum(1, np.abs(b))).max()))
    with capsys.disabled():
        print("\n[initializer] Normalize against fp64: %.3e (NORM_MEASURED %.1e)" % (worst, ic.NORM_MEASURED))
    assert worst <= ic.NORM_TOL


def test_matrices_of_all_inlier_sets_against_oracle(orbx, capsys):
    worst, compared = 0.0, 0
    for case in ic.CASES:
        sets = ic.well_conditioned_pure_sets(case)
        if not sets:
            continue
        s = solver(orbx, case)
        uv, _, _, _ = ic.problem_arrays(case)
        Ms = ic.oracle_matrices(case)
        for k in sets:
            M, score, flags, n = s.hypothesis(case["model"], case["sets"][k])
            want = unit(Ms[k])
            worst = max(worst, float(np.abs(unit(M, want) - want).max()))
            _, want_flags = O.check(case["model"], Ms[k], uv, ic.SIGMA)
            assert n == int(flags.sum())
            # the flags of the planted inliers are the oracle's: the case keeps every chi-square MARGIN away from its threshold
            assert np.array_equal(flags[~case["wrong"]], want_flags[~case["wrong"]]), (case["name"], k)
            compared += 1
    with capsys.disabled():
        print("\n[initializer] H21i / F21i of %d sets against fp64: %.3e (MATRIX_MEASURED %.1e)" % (compared, worst, ic.MATRIX_MEASURED))
    assert compared > 500 and worst <= ic.MATRIX_TOL


@pytest.mark.parametrize("name", [c["name"] for c in ic.CASES])
def test_scores_are_the_float_sum_in_match_order(orbx, name):
    case = ic.BY_NAME[name]
    s = solver(orbx, case)
    uv = np.hstack([case["keys1"][case["first"]], case["keys2"][case["second"]]])
    positive = 0
    for model in (O.MODEL_H, O.MODEL_F):
        for st in case["sets"][:40]:
            M, score, flags, n = s.hypothesis(model, st)
            want, want_flags = O.score_f32(model, M, uv, ic.SIGMA)           # the oracle's ordered sum, fed the library's own matrix
            assert np.float32(score).tobytes() == np.float32(want).tobytes(), (name, model, score, want)
            assert np.array_equal(flags, want_flags) and n == int(flags.sum())
            positive += score > 0
    assert positive > 40


def test_find_keeps_the_first_of_equal_scores(orbx):
    case = ic.BY_NAME["general65"]
    s = solver(orbx, case, 5)
    s.draw()
    sm, cnt, masks = s.hypotheses(np.concatenate([case["sets"][:5]] * 2), [0] * 5 + [1] * 5)
    in_place = [s.find(m) for m in (0, 1)]
    for m in (0, 1):                                         # the walk, by hand: strict >
        best = -1
        for it in range(5):
            if sm[5 * m + it, 0] > (sm[5 * m + best, 0] if best >= 0 else 0):
                best = it
        assert in_place[m][3] == best and in_place[m][1] == sm[5 * m + best, 0]
        assert in_place[m][0].tobytes() == sm[5 * m + best, 1:].tobytes()
    s.attach_results(sm, cnt, masks)
    for m in (0, 1):                                         # the replay gives the same bytes
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(s.find(m), in_place[m]))
    tied = sm.copy()
    tied[[1, 3], 0] = 1e6                                    # H: iterations 1 and 3 tie at the top
    tied[5:, 0] = [0, 7, 7, 7, 3]                            # F: 1, 2, 3 tie
    tied[3, 1:] += 1                                         # the later of the tied H results is recognisably different
    s.attach_results(tied, cnt, masks)
    MH, sH, fH, itH = s.find(0)
    assert itH == 1 and sH == np.float32(1e6) and MH.tobytes() == tied[1, 1:].tobytes()
    assert s.find(1)[3] == 1
    zero = sm.copy()
    zero[:, 0] = 0                                           # nothing exceeds the initial score 0: no winner
    s.attach_results(zero, cnt, masks)
    M0, s0, f0, it0 = s.find(0)
    assert it0 == -1 and s0 == 0 and not f0.any() and not M0.any()


def recovered(case, R, t, P, tri):
    """deviations of an accepted Initialize from the planted motion and structure"""
    rot = float(np.abs(R - case["R"]).max())
    tn = case["t"] / np.linalg.norm(case["t"])
    dirn = float(np.abs(t - tn).max())
    X = case["X1_all"][case["point_of_key1"]]                # the planted point of every key of frame 1
    scale = np.linalg.norm(case["t"])                        # |t21| = 1 fixes the scale of the reconstruction
    struct = float((np.linalg.norm(P[tri] * scale - X[tri], axis=1) / X[tri][:, 2]).max())
    return rot, dirn, struct


def test_initialize_recovers_the_planted_motion_and_structure(orbx, capsys):
    worst = np.zeros(3)
    for name in ACCEPTED:
        case = ic.BY_NAME[name]
        s = solver(orbx, case, current=False)
        ok, R, t, P, tri = s.Initialize(case["keys2"], case["matches12"])
        assert ok, name
        want = ic.oracle_initialize(case)
        model, M, inl, Rt = s.plan_check_rt()
        assert model == want["model"] == case["model"] and len(Rt) == (8 if model == O.MODEL_H else 4)
        assert abs(np.linalg.norm(t) - 1) < 1e-6 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-5
        # triangulated: exactly the keys of correct matches (a wrong match never survives CheckRT here), none without a match
        matched_right = np.zeros(case["n1"], bool)
        matched_right[case["first"][~case["wrong"]]] = True
        assert not tri[~matched_right].any() and tri.sum() >= 0.9 * matched_right.sum(), name
        assert tri.sum() == int(want["good"].sum()), name
        worst = np.maximum(worst, recovered(case, R, t, P, tri))
    with capsys.disabled():
        print("\n[initializer] Initialize against the planted scene: R %.3e, t %.3e, structure %.3e (MEASURED %.1e, %.1e, %.1e)"
              % (*worst, ic.ROT_MEASURED, ic.DIR_MEASURED, ic.STRUCT_MEASURED))
    assert worst[0] <= ic.ROT_TOL and worst[1] <= ic.DIR_TOL and worst[2] <= ic.STRUCT_TOL


@pytest.mark.parametrize("name", REFUSED)
def test_initialize_refuses(orbx, name):
    case = ic.BY_NAME[name]
    s = solver(orbx, case, current=False)
    ok, R, t, P, tri = s.Initialize(case["keys2"], case["matches12"])
    assert not ok and not R.any() and not t.any() and not P.any() and not tri.any()       # outputs untouched
    assert not ic.oracle_initialize(case)["ok"]
    if case["scene"] == "rotation":                          # refused by the rules, not by a crash on the way: CheckRT was reached
        assert len(s.plan_check_rt()[3]) == 8


def test_fewer_than_eight_matches_are_refused(orbx):
    case = ic.BY_NAME["plane8"]
    m = case["matches12"].copy()
    m[case["first"][0]] = -1                                 # 7 matches
    s = orbx.Initializer(case["keys1"], ic.K, ic.SIGMA, 5, rand=ic.Lcg(1), rand_max=ic.RAND_MAX)
    assert s.set_current(case["keys2"], m) == 7
    with pytest.raises(orbx.OrbxError) as e:
        s.draw()
    assert e.value.code == orbx.ORBX_E_INVALID
    with pytest.raises(orbx.OrbxError) as e:
        s.initialize()
    assert e.value.code == orbx.ORBX_E_INVALID
    with pytest.raises(orbx.OrbxError):
        s.find(0)                                            # nothing was drawn
    with pytest.raises(orbx.OrbxError) as e:
        s.hypothesis(0, [0, 1, 2, 3, 4, 5, 6, 7])            # index 7 is outside the 7 matches
    assert e.value.code == orbx.ORBX_E_INVALID
    assert s.set_current(case["keys2"], case["matches12"]) == 8 and s.draw().shape == (5, 8)      # the handle is still good


def test_no_iterations_and_zero_scores_return_false(orbx):
    case = ic.BY_NAME["general64"]
    s = solver(orbx, case, 0)
    assert s.draw().shape == (0, 8)
    assert s.find(0)[3] == -1 and s.find(1)[3] == -1
    assert s.initialize()[0] is False                         # SH == SF == 0: RH is NaN (include/orbp.h)
    assert len(s.plan_check_rt()[3]) == 0


def test_a_second_initialize_is_independent_of_the_first(orbx):
    """one reference frame, two current frames on one handle: the second call gives what a fresh handle gives"""
    a = ic.BY_NAME["general128"]
    rng = np.random.default_rng(9)
    noisy = (a["keys2"] + rng.normal(0, 30, a["keys2"].shape)).astype(np.float32)       # a current frame that fits nothing
    # the second current frame: the case's own, its keys in reverse order and a third of the matches dropped
    m2 = a["matches12"].copy()
    m2[a["first"][::3]] = -1
    keys2, m2 = a["keys2"][::-1].copy(), np.where(m2 >= 0, a["n2"] - 1 - m2, -1).astype(np.int32)
    fresh = orbx.Initializer(a["keys1"], ic.K, ic.SIGMA, 50, rand=ic.Lcg(77), rand_max=ic.RAND_MAX)
    want = fresh.Initialize(keys2, m2)
    s = orbx.Initializer(a["keys1"], ic.K, ic.SIGMA, 50, rand=ic.Lcg(5), rand_max=ic.RAND_MAX)
    assert not s.Initialize(noisy, a["matches12"])[0]         # 30 px of noise: nothing to initialise from
    s.SetRand(ic.Lcg(77), ic.RAND_MAX)
    got = s.Initialize(keys2, m2)
    assert want[0] and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want))


@pytest.mark.parametrize("name", ["plane65", "general129", "rotation129", "few63", "plane9"])
def test_replaying_attached_results_equals_evaluating_in_place(orbx, name):
    case = ic.BY_NAME[name]
    want = solver(orbx, case, current=False).Initialize(case["keys2"], case["matches12"])
    s = solver(orbx, case)
    sets = s.draw()
    uv, pn, T1, T2, sigma, sets2, models = s.problem()
    assert np.array_equal(sets2, np.concatenate([sets, sets])) and np.array_equal(models, [0] * len(sets) + [1] * len(sets))
    s.attach_results(*s.hypotheses(sets2, models))
    model, M, inl, Rt = s.plan_check_rt()
    if len(Rt):
        status, cosp, p3d = s.check_rt_matches(Rt, inl)
        assert set(np.unique(status)) <= set(range(8)) and (status[:, ~inl] == orbx.ORBM_INIT_RT_NOT_INLIER).all()
        for k in range(len(Rt)):                             # the per-match verdicts add up to CheckRT's own answer
            n_good, P, good, parallax = s.check_rt(Rt[k, :9], Rt[k, 9:], inl)
            assert n_good == int((status[k] <= orbx.ORBM_INIT_RT_GOOD_LOW_PARALLAX).sum())
            assert good.sum() == int((status[k] == orbx.ORBM_INIT_RT_GOOD).sum())
        s.attach_check_rt(Rt, inl, status, cosp, p3d)
    got = s.initialize()
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want))


def test_motions_are_rotations_and_unit_translations(orbx):
    for name, n in (("plane128", 8), ("general128", 4)):
        case = ic.BY_NAME[name]
        s = solver(orbx, case)
        s.draw()
        M = s.find(case["model"])[0]
        Rt = s.motions(case["model"], M)
        assert Rt.shape == (n, 12)
        for row in Rt.astype(np.float64):
            R, t = row[:9].reshape(3, 3), row[9:]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1) < 1e-5 and abs(np.linalg.norm(t) - 1) < 1e-6
        # one of them is the planted motion, and the oracle's candidates are the same set
        want = O.motions_h(M.astype(np.float64), ic.K) if n == 8 else O.motions_f(M.astype(np.float64), ic.K)
        for R, t in want:
            assert min(max(np.abs(row[:9].reshape(3, 3) - R).max(), np.abs(row[9:] - t).max()) for row in Rt) < 1e-3
        tn = case["t"] / np.linalg.norm(case["t"])
        assert min(max(np.abs(row[:9].reshape(3, 3) - case["R"]).max(), np.abs(row[9:] - tn).max()) for row in Rt) < ic.DIR_TOL
    s = solver(orbx, ic.BY_NAME["plane64"])
    assert len(s.motions(0, np.eye(3, dtype=np.float32))) == 0                  # d1 / d2 < 1.00001: ReconstructH's exit :597
