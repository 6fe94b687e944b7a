"""No-GPU checks of the Sim3Solver (include/orbp.h orbp_sim3_*, csrc/orbm_sim3_body.h) and of the argument checks of
orbm_sim3_hypotheses (include/orbm.h): RANSAC parameters, draws, the hypothesis against the fp64 oracle of tests/sim3_oracle.py on
the cases of tests/sim3_cases.py, the integer-truncated thresholds, the iterate state machine, and the replay of attached results."""
import ctypes as C
import math

import numpy as np
import pytest

import sim3_cases as sc
import sim3_oracle as so


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_solver(built, case, scripted=True, min_inliers=sc.MIN_INLIERS, max_its=sc.MAX_ITERATIONS):
    s = built.Sim3Solver(case["x1"], case["x2"], case["sigma2_1"], case["sigma2_2"], case["K1"], case["K2"], case["fix"],
                         rand=sc.Lcg(case["seed"]) if scripted else None, rand_max=sc.RAND_MAX)
    s.SetRansacParameters(sc.PROBABILITY, min_inliers, max_its)
    return s


def first_pure(case):
    return next(k for k, tri in enumerate(case["triples"]) if not case["outlier"][tri].any())


def test_case_conditions_hold():
    """what makes the expected answers hand-derivable (sim3_cases.py asserts the same at import)"""
    for case in sc.CASES:
        assert sc.check_conditions(case) is None, case["name"]
        assert 0.5 <= case["s"] <= 2.0 and (case["s"] == 1.0) == case["fix"]


def test_elementary_functions_of_the_body(built):
    """the body's own atan2 / sin / cos against libm: about 1e-15, as the byte equality of host and device needs no more"""
    L = built.lib()
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.uniform(0, 2 * math.pi, 4000), [0.0, 1e-12, math.pi / 4, math.pi / 2, math.pi, 2 * math.pi, 6.5]])
    assert max(abs(L.orbp_sim3_math(1, x, 0) - math.sin(x)) for x in xs) < 1e-15
    assert max(abs(L.orbp_sim3_math(2, x, 0) - math.cos(x)) for x in xs) < 1e-15
    ys, ws = rng.uniform(0, 1, 4000), rng.uniform(-1, 1, 4000)
    assert max(abs(L.orbp_sim3_math(0, y, w) - math.atan2(y, w)) for y, w in zip(ys, ws)) < 2e-15
    for y, w in ((0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (1e-300, 1.0), (1.0, 1e-300), (1.0, -1e-300)):
        assert abs(L.orbp_sim3_math(0, y, w) - math.atan2(y, w)) < 2e-15


def test_ransac_parameters_equal_the_oracle(built):
    rng = np.random.default_rng(3)
    for N in (0, 2, 3, 6, 19, 20, 21, 64, 300, 2000):
        x = rng.uniform(1, 2, (N, 3)).astype(np.float32)
        s = built.Sim3Solver(x, x, np.ones(N), np.ones(N), sc.K1, sc.K2, True)
        st = s.ransac_state()
        assert (st["min_inliers"], st["max_its"]) == (6, so.ransac_iterations(N, 0.99, 6, 300))       # the constructor's defaults
        for mi in (3, 6, 20, 21):
            for mx in (1, 5, 300, 100000):
                for prob in (0.5, 0.99, 0.999999):
                    s.SetRansacParameters(prob, mi, mx)
                    st = s.ransac_state()
                    assert st["max_its"] == so.ransac_iterations(N, prob, mi, mx), (N, mi, mx, prob)
                    assert st["min_inliers"] == mi and st["iterations"] == 0
                    if N > 0:                                                   # the float epsilon of :125, bit for bit
                        assert np.float32(st["epsilon"]).tobytes() == so.ransac_epsilon(N, mi).tobytes(), (N, mi)
                    if N == mi or N < mi:
                        assert st["max_its"] == 1


def test_draws_follow_the_reference(built):
    case = sc.BY_NAME["n65_free"]
    s = make_solver(built, case)
    assert np.array_equal(s.draw(300), case["triples"][:s.ransac_state()["max_its"]])     # swap-with-back, pop; capped at mRansacMaxIts
    assert len(s.draw(5)) == 0 and len(s.queued()) == s.ransac_state()["max_its"]
    # draw + iterate consumes the same triples, and as many values of the source, as iterate alone
    calls = {"a": 0, "b": 0}

    def counted(key):
        lcg = sc.Lcg(case["seed"])

        def rand():
            calls[key] += 1
            return lcg()
        s = built.Sim3Solver(case["x1"], case["x2"], case["sigma2_1"], case["sigma2_2"], case["K1"], case["K2"], case["fix"], rand=rand,
                             rand_max=sc.RAND_MAX)
        s.SetRansacParameters(sc.PROBABILITY, sc.MIN_INLIERS, sc.MAX_ITERATIONS)
        return s

    a, b = counted("a"), counted("b")
    assert len(a.draw(3)) == 3 and calls["a"] == 9
    for _ in range(4):
        ga, gb = a.iterate(2), b.iterate(2)
        assert calls["a"] == max(calls["b"], 9)                                    # three values per iteration, drawn ahead or not
        assert (ga[0] is None) == (gb[0] is None) and (ga[0] is None or ga[0].tobytes() == gb[0].tobytes())
        assert ga[1] == gb[1] and np.array_equal(ga[2], gb[2]) and ga[3] == gb[3]
        assert a.ransac_state() == b.ransac_state()


def test_hypothesis_flags_and_values_against_oracle(built):
    """flags identical (the case conditions leave them to the oracle alone); s, R, t within 4x the measured deviation"""
    worst = 0.0
    for case in sc.CASES:
        if case["N"] < 3:
            continue
        s = make_solver(built, case)
        res = sc.oracle_results(case)
        for k in range(len(case["triples"])):
            R, t, scale, inl, n = s.hypothesis(case["triples"][k])
            so_, Ro, to, flags = res[k][:4]
            assert np.array_equal(inl, flags) and n == int(flags.sum()), (case["name"], k)
            got = np.concatenate([[scale], R.reshape(9), t]).astype(np.float64)
            want = np.concatenate([[so_], Ro.reshape(9), to])
            worst = max(worst, float((np.abs(got - want) / np.maximum(1, np.abs(want))).max()))
            if case["fix"]:
                assert scale == np.float32(1.0)
    print("largest deviation of the host path from the fp64 oracle: %.3g (SRT_MEASURED = %.3g)" % (worst, sc.SRT_MEASURED))
    assert worst <= sc.SRT_TOL and sc.SRT_TOL < 1e-3


def test_thresholds_are_truncated_to_integers(built):
    """sigma2 = 1.44: 9.210 * 1.44 = 13.26 is stored as 13, so err = 13.1 is an outlier and 12.9 an inlier; sigma2 = 1: 9.21 -> 9, so
    9.1 is an outlier.  Hand-derived: the points are moved sqrt(err) px along u in image 1, whose reprojection error is then err;
    side 2 is at octave 7 (threshold 118) and passes."""
    rng = np.random.default_rng(11)
    scale, R, t = 1.3, so.rodrigues(np.array([0.1, -0.2, 0.15])), np.array([0.2, -0.1, 0.05])
    x2 = np.stack([rng.uniform(-2, 2, 6), rng.uniform(-1, 1, 6), rng.uniform(4, 8, 6)], 1)
    x1 = scale * (x2 @ R.T) + t
    errs = (13.1, 12.9, 9.1)
    for k, e in enumerate(errs):
        x1[3 + k, 0] += math.sqrt(e) / float(sc.K1[0]) * x1[3 + k, 2]
    s144 = np.float32(1.2) * np.float32(1.2)
    sig1 = np.array([1, 1, 1, s144, s144, 1], np.float32)
    sig2 = np.full(6, np.float32(1.2) ** 14, np.float32)
    s = built.Sim3Solver(x1, x2, sig1, sig2, sc.K1, sc.K2, False)
    e1, e2 = s.max_errors()
    assert list(e1) == [9, 9, 9, 13, 13, 9] and list(e2) == [118] * 6           # 9.21 * 1.2^14 = 118.25
    inl = s.hypothesis([0, 1, 2])[3]
    assert list(inl) == [True, True, True, False, True, False]


def test_state_machine(built):
    case = sc.BY_NAME["n64_fix"]
    k0 = first_pure(case)
    assert k0 > 0                                                               # the case starts with a contaminated triple
    s = make_solver(built, case)
    assert s.estimated() is None
    T, no_more, flags, n = s.iterate(1)                                          # the first iteration always becomes best (count >= 0)
    R0, t0, s0, inl0, n0 = s.hypothesis(case["triples"][0])
    assert T is None and not no_more and not flags.any() and n == 0
    assert s.ransac_state()["best_inliers"] == n0 <= sc.MIN_INLIERS - 3
    R, t, scale = s.estimated()
    assert R.tobytes() == R0.tobytes() and t.tobytes() == t0.tobytes() and scale == s0
    T, no_more, flags, n = s.iterate(300)                                        # a pose at the first all-inlier triple
    st = s.ransac_state()
    assert T is not None and st["iterations"] == k0 + 1 and not no_more
    assert np.array_equal(flags, ~case["outlier"]) and n == int((~case["outlier"]).sum()) == st["best_inliers"]
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = case["s"] * case["R"], case["t"]
    assert (np.abs(T - want) / np.maximum(1, np.abs(want))).max() <= sc.SRT_TOL and list(T[3]) == [0, 0, 0, 1]
    T, no_more, flags, n = s.iterate(5)                                          # the state survives the success
    k1 = next(k for k in range(k0 + 1, 300) if not case["outlier"][case["triples"][k]].any())     # the next all-inlier triple
    assert s.ransac_state()["best_inliers"] == st["best_inliers"] and s.ransac_state()["iterations"] == min(k1 + 1, k0 + 6)
    assert (T is not None) == (k1 + 1 <= k0 + 6) and (T is None or np.array_equal(flags, ~case["outlier"]))
    # no_more on the call that reaches mRansacMaxIts: with a pose, and without one
    s = make_solver(built, case, max_its=k0 + 1)
    T, no_more, flags, n = s.iterate(300)
    assert T is not None and no_more and np.array_equal(flags, ~case["outlier"])
    s = make_solver(built, case, max_its=k0)
    T, no_more, flags, n = s.iterate(300)
    assert T is None and no_more and not flags.any() and n == 0 and s.ransac_state()["iterations"] == k0
    T, no_more, flags, n = s.iterate(300)
    assert T is None and no_more and s.ransac_state()["iterations"] == k0
    # N < minInliers: no_more at once, flags all false, nothing drawn; N == minInliers: one iteration, 20 > 20 is false
    for name in ("n0_free", "n2_fix", "n3_free", "n19_fix"):
        s = make_solver(built, sc.BY_NAME[name])
        T, no_more, flags, n = s.iterate(5)
        assert T is None and no_more and not flags.any() and n == 0 and s.ransac_state()["iterations"] == 0 and len(s.draw(5)) == 0
    s = make_solver(built, sc.BY_NAME["n20_free"])
    T, no_more, flags, n = s.iterate(5)
    assert T is None and no_more and s.ransac_state()["iterations"] == 1 and s.ransac_state()["best_inliers"] == 20
    s = make_solver(built, sc.BY_NAME["n21_free"])
    T, flags, n = s.find()
    assert T is not None and n == 21 and flags.all()


@pytest.mark.parametrize("name", ["n0_free", "n3_fix", "n19_fix", "n20_free", "n21_fix", "n63_free", "n64_fix", "n128_fix", "n300_free"])
def test_iterate_traces_equal_the_oracle_state_machine(built, name):
    """iterate(5) until bNoMore against sim3_oracle.Solver (the fp64 restatement of :140-207) on the same scripted draws: the same
    calls return a pose, with the same flags, counts, bNoMore and iteration numbers; the poses agree within SRT_TOL"""
    case = sc.BY_NAME[name]
    lib_s = make_solver(built, case)
    ora = so.Solver(case["x1"], case["x2"], case["sigma2_1"], case["sigma2_2"], case["K1"], case["K2"], case["fix"], sc.Lcg(case["seed"]),
                    sc.RAND_MAX)
    ora.SetRansacParameters(sc.PROBABILITY, sc.MIN_INLIERS, sc.MAX_ITERATIONS)
    assert lib_s.ransac_state()["max_its"] == ora.max_its
    for call in range(400):
        T, no_more, flags, n = lib_s.iterate(5)
        To, no_more_o, flags_o, n_o = ora.iterate(5)
        st = lib_s.ransac_state()
        assert (T is None) == (To is None) and no_more == no_more_o and n == n_o and np.array_equal(flags, flags_o), (name, call)
        assert st["iterations"] == ora.n_iter and st["best_inliers"] == ora.n_best, (name, call)
        if T is not None:
            assert (np.abs(T - To) / np.maximum(1, np.abs(To))).max() <= sc.SRT_TOL, (name, call)
        if no_more:
            break
    assert no_more and call < 399


def _run(s, step):
    out = []
    for _ in range(400):
        T, no_more, flags, n = s.iterate(step)
        out.append((None if T is None else T.tobytes(), no_more, flags.tobytes(), n, tuple(sorted(s.ransac_state().items())),
                    tuple(a.tobytes() for a in s.estimated())))
        if no_more:
            break
    return out


@pytest.mark.parametrize("name", ["n21_fix", "n63_free", "n64_fix", "n129_free", "n300_fix"])
def test_replay_of_attached_results_gives_the_same_bytes(built, name):
    case = sc.BY_NAME[name]
    want5, want_find = _run(make_solver(built, case), 5), make_solver(built, case).find()
    for step in (5, None):
        s = make_solver(built, case)
        tri = s.draw(300)
        assert len(tri) == s.ransac_state()["max_its"]
        s.attach_results(*s.hypotheses(tri))
        if step:
            assert _run(s, step) == want5
        else:
            got = s.find()
            assert got[0].tobytes() == want_find[0].tobytes() and np.array_equal(got[1], want_find[1]) and got[2] == want_find[2]
    # results for a part of the queue are refused; a solver without results evaluates its queued triples in place
    s = make_solver(built, case)
    tri = s.draw(300)
    with pytest.raises(built.OrbxError):
        s.attach_results(*s.hypotheses(tri[:1]))
    assert _run(s, 5) == want5


def _args(built, names=(("n65_free", 5), ("n3_fix", 1), ("n64_fix", 5))):
    probs = []
    for name, h in names:
        s = make_solver(built, sc.BY_NAME[name])
        e1, e2 = s.max_errors()
        probs.append((s.x1, s.x2, e1, e2, s.K1, s.K2, s.fix_scale, sc.BY_NAME[name]["triples"][:h]))
    keys = ("off", "x1", "x2", "e1", "e2", "cams", "hyp_off", "tri", "mask_off")
    a = dict(zip(keys, built.ORBmatcher.pack_sim3_problems(probs)))
    H, MW = int(a["hyp_off"][-1]), int(a["mask_off"][-1])
    a.update(B=len(probs), H=H, cnt=np.full(H, 77, np.int32), sRt=np.full((H, 13), 77, np.float32), masks=np.full(MW, 77, np.uint32))
    return a


ORDER = ("off", "x1", "x2", "e1", "e2", "cams", "hyp_off", "tri", "mask_off", "cnt", "sRt", "masks")


def _host(L, a, B=None):
    return L.orbm_sim3_hypotheses(None, a["B"] if B is None else B, *[p(a[k]) for k in ORDER])


def _device(L, a, B=None, H=None):
    return L.orbm_sim3_hypotheses_device(None, a["B"] if B is None else B, a["H"] if H is None else H, *[p(a[k]) for k in ORDER], None)


def _untouched(a):
    return (a["cnt"] == 77).all() and (a["sRt"] == 77).all() and (a["masks"] == 77).all()


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle every bad argument still gets ORBX_E_INVALID and a text, and the empty batches are ORBX_OK."""
    L = built.lib()
    E, OK = built.ORBX_E_INVALID, built.ORBX_OK
    a = _args(built)
    assert built.SIM3_CAM_DTYPE.itemsize == 36
    assert _host(L, a, B=-1) == E and _device(L, a, B=-1) == E and _device(L, a, H=-1) == E
    assert _host(L, a, B=0) == OK and _device(L, a, B=0) == OK and _device(L, a, H=0) == OK and _untouched(a)
    none = _args(built, (("n65_free", 0), ("n0_free", 0)))
    assert _host(L, none) == OK and _untouched(none)                               # no hypothesis at all
    for key in ORDER:
        b = dict(a)
        b[key] = None
        assert _host(L, b) == E and b"NULL" in L.orbm_last_error(), key
        assert _device(L, b) == E and b"NULL" in L.orbm_last_error(), key
    for key, at, val, text in (("off", 1, 70, b"off not monotone"), ("off", 0, 1, b"must be 0"), ("hyp_off", 2, 1, b"hyp_off not monotone"),
                               ("hyp_off", 0, 1, b"must be 0"), ("mask_off", 1, 14, b"mask_off"), ("mask_off", 0, 1, b"must be 0")):
        b = dict(a)
        b[key] = a[key].copy()
        b[key][at] = val
        if key == "off" and at == 1:
            b[key][2] = 69
        assert _host(L, b) == E and text in L.orbm_last_error(), (key, at, L.orbm_last_error())
    for at, val in ((0, -1), (4, 65), (3 * 5, 3), (3 * 6 + 2, 64)):                 # a triple index outside its problem
        b = dict(a)
        b["tri"] = a["tri"].copy()
        b["tri"].reshape(-1)[at] = val
        assert _host(L, b) == E and b"triple index" in L.orbm_last_error(), at
    odd = np.zeros(64, np.uint8)
    b = dict(a)
    args = [p(b[k]) for k in ORDER]
    args[1] = C.c_void_p(odd.ctypes.data + 1)
    assert L.orbm_sim3_hypotheses_device(None, b["B"], b["H"], *args, None) == E and b"aligned" in L.orbm_last_error()
    assert _untouched(a)
    # the NULL-handle rule of the pose batch: good arguments need the GPU
    import torch
    want = E if torch.cuda.is_available() else built.ORBX_E_HIP
    assert _host(L, a) == want and _device(L, a) == want and _untouched(a)
    if want != E:
        assert b"no CPU path" in L.orbm_last_error()
    # the host solver's own checks
    s = make_solver(built, sc.BY_NAME["n65_free"])
    for tri in ([0, 1, 65], [-1, 2, 3]):
        with pytest.raises(built.OrbxError):
            s.hypothesis(tri)
    c = sc.BY_NAME["n21_free"]
    with pytest.raises(built.OrbxError) as e:                                      # a source without its range
        built.Sim3Solver(c["x1"], c["x2"], c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"], rand=sc.Lcg(1))
    assert e.value.code == E and "rand_max" in str(e.value)
    assert L.orbp_sim3_create(None, 0, None, None, None, None, p(sc.K1), p(sc.K2), 0) < 0
    h = C.c_void_p()
    assert L.orbp_sim3_create(C.byref(h), -1, None, None, None, None, p(sc.K1), p(sc.K2), 0) < 0 and not h
    assert L.orbp_sim3_create(C.byref(h), 3, None, None, None, None, p(sc.K1), p(sc.K2), 0) < 0 and not h
