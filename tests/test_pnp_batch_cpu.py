"""No-GPU checks of the PnPsolver's draw-ahead interface (include/orbp.h orbp_pnp_draw / queued / get_problem / hypothesis /
attach_results, csrc/orbp_epnp_body.h) and of the argument checks of orbm_pnp_hypotheses (include/orbm.h):
  * the host solver did not move when EPnP's arithmetic went into the shared body: tests/golden/pnp/epnp_parent.npz holds the bytes
    the parent commit's orbp.cc produced (tools/gen_pnp_golden.py), compared with == on the raw bytes;
  * draw + hypothesis + attach_results + iterate equals the plain iterate on a second solver fed the same stream, call by call;
  * orbp_pnp_hypothesis at set_size 6 and 8 against oracle/pose_oracle.py's epnp at 1e-8 (the tolerance of
    tests/test_pose.py::test_epnp_equals_oracle for n = 6 to 8), flags equal to those recomputed from the oracle's pose;
  * tests/cxx/pnp_asan_main.cc under AddressSanitizer and UBSan, stand-alone on the CPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pose_oracle as po  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pnp", "epnp_parent.npz")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_solver(built, case, params=None, seed=None):
    fx, fy, cx, cy = (float(v) for v in case["K"])
    source = pc.Lcg(case["seed"] if seed is None else seed)
    s = built.PnPsolver(case["p2d"], case["sigma2"], case["p3d"], fx, fy, cx, cy, rand=source, rand_max=pc.RAND_MAX)
    s.source = source
    s.SetRansacParameters(*(params or case.get("params") or (0.99, min(10, case["N"]), 300, case["set_size"], 0.5, 5.991)))
    return s


# ------------------------------------------------------------------------------------------------- the refactor is pinned
def test_epnp_bytes_equal_the_parent_commit(built):
    g = np.load(GOLDEN)
    names = [str(n) for n in g["epnp_names"]]
    assert {"n4_exact", "n4_noisy", "n5_exact", "n6_noisy", "n8_exact", "n12_noisy", "n50_exact", "n50_noisy", "coplanar4"} <= set(names)
    for name in names:
        pws, us, K = g["epnp_%s_pws" % name], g["epnp_%s_us" % name], g["epnp_%s_K" % name]
        R, t = np.zeros(9), np.zeros(3)
        err = built.lib().orbp_epnp(len(pws), p(pws), p(us), *[float(v) for v in K], p(R), p(t))
        assert R.tobytes() == g["epnp_%s_R" % name].tobytes(), name
        assert t.tobytes() == g["epnp_%s_t" % name].tobytes(), name
        assert np.array([err]).tobytes() == g["epnp_%s_err" % name].tobytes(), name
    # the coplanar set is rank-deficient by construction: its world points have z = 0 exactly
    assert (g["epnp_coplanar4_pws"][:, 2] == 0).all()


def test_iterate_transcripts_equal_the_parent_commit(built):
    g = np.load(GOLDEN)
    for k in range(int(g["n_transcripts"][0])):
        K, prm = g["tr%d_K" % k], g["tr%d_params" % k]
        s = built.PnPsolver(g["tr%d_p2d" % k], g["tr%d_sigma2" % k], g["tr%d_p3d" % k], *[float(v) for v in K],
                            rand=pc.Lcg(int(g["tr%d_seed" % k][0])), rand_max=pc.RAND_MAX)
        s.SetRansacParameters(float(prm[0]), int(prm[1]), int(prm[2]), int(prm[3]), float(prm[4]), float(prm[5]))
        L, N = built.lib(), len(g["tr%d_sigma2" % k])
        for call in range(len(g["tr%d_ret" % k])):
            no_more, n = C.c_int(), C.c_int()
            inl, T = np.zeros(N, np.uint8), np.zeros(16, np.float32)
            r = L.orbp_pnp_iterate(s.h, 5, C.byref(no_more), p(inl), C.byref(n), p(T))
            want = [int(g["tr%d_%s" % (k, f)][call]) for f in ("ret", "no_more", "n_inliers", "iterations")]
            assert [r, no_more.value, n.value, s.ransac_state()["iterations"]] == want, (k, call)
            assert inl.tobytes() == g["tr%d_masks" % k][call].tobytes() and T.tobytes() == g["tr%d_T" % k][call].tobytes(), (k, call)
        assert no_more.value


# ------------------------------------------------------------------------------------------------- draw ahead + replay
def _call(s):
    T, no_more, inl, n = s.iterate(5)
    return (None if T is None else T.tobytes(), no_more, None if inl is None else inl.tobytes(), n, tuple(sorted(s.ransac_state().items())))


def _run(s, calls=200):
    out = []
    for _ in range(calls):
        out.append(_call(s))
        if out[-1][1]:
            break
    assert out[-1][1], "RANSAC did not end"
    return out


def _evaluate_all(s, n_iterations=5):
    s.draw(n_iterations)
    s.attach_results(*s.hypotheses(s.queued()))


@pytest.mark.parametrize("key", sorted(pc.RANSAC))
def test_draw_hypothesis_attach_iterate_equals_plain_iterate(built, key):
    case = pc.ransac_case(key)
    want = _run(make_solver(built, case))
    s = make_solver(built, case)
    max_its = s.ransac_state()["max_its"]
    sm = s.draw(5)
    assert len(sm) == max(max_its, 5) == len(s.queued()) and sm.shape[1] == case["set_size"]      # the || loop: all of them at once
    assert all(len(set(row)) == case["set_size"] and 0 <= min(row) and max(row) < case["N"] for row in sm.tolist())
    s.attach_results(*s.hypotheses(sm))
    assert _run(s) == want
    # re-armed before every call, as a caller that batches every round would do
    s = make_solver(built, case)
    got = []
    for _ in range(200):
        _evaluate_all(s)
        got.append(_call(s))
        if got[-1][1]:
            break
    assert got == want


def test_a_pose_in_the_middle_of_the_queue_then_iterating_on(built):
    case = pc.ransac_case("early")
    want = _run(make_solver(built, case))
    first = want[0]
    assert first[0] is not None and not first[1]
    its = dict(first[4])
    assert 0 < its["iterations"] < its["max_its"]                                   # the pose came before the queue was used up
    s = make_solver(built, case)
    _evaluate_all(s)
    assert _call(s) == first and len(s.queued()) == its["max_its"] - its["iterations"]  # the rest stays queued, with its results
    assert _run(s) == want[1:]


def test_max_its_below_the_step_runs_the_step(built):
    """`while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)`: max_its = 3 and iterate(5) run 5 iterations"""
    case = pc.ransac_case("never")
    prm = (0.99, case["params"][1], 3, 4, 0.5, 5.991)
    a, b = make_solver(built, case, prm), make_solver(built, case, prm)
    assert a.ransac_state()["max_its"] == 3
    assert len(b.draw(5)) == 5 and len(b.draw(5)) == 0 and len(b.draw(7)) == 2 and len(b.queued()) == 7
    b.attach_results(*b.hypotheses(b.queued()))
    ca, cb = _call(a), _call(b)
    assert ca == cb and dict(ca[4])["iterations"] == 5 and ca[1] and len(b.queued()) == 2
    assert len(b.draw(5)) == 3 and len(b.queued()) == 5                              # past max_its a call consumes its step
    assert _call(a) == _call(b) and a.ransac_state()["iterations"] == 10 and len(b.queued()) == 0      # 2 replayed, 3 in place


def test_too_few_correspondences_draw_nothing(built):
    case = pc.BY_NAME["n5_s4"]
    s = make_solver(built, case, (0.99, 10, 300, 4, 0.5, 5.991))                  # min_inliers 10 > N = 5
    assert len(s.draw(5)) == 0 and len(s.queued()) == 0
    s.attach_results(np.zeros(0, np.int32), np.zeros((0, 12)), np.zeros((0, 1), np.uint32))
    T, no_more, inl, n = s.iterate(5)
    assert T is None and no_more and n == 0 and s.ransac_state()["iterations"] == 0


def test_queue_without_results_partial_results_and_set_parameters(built):
    case = pc.ransac_case("set6")
    want = _run(make_solver(built, case))
    s = make_solver(built, case)
    sm = s.draw(5)
    assert _run(s) == want                                                          # a queue without results is evaluated in place
    s = make_solver(built, case)
    sm = s.draw(5)
    with pytest.raises(built.OrbxError) as e:
        s.attach_results(*s.hypotheses(sm[:3]))                                     # results for a part of the queue
    assert e.value.code == built.ORBX_E_INVALID and "queued" in str(e.value)
    assert _run(s) == want
    # SetRansacParameters drops the queue and the attached results: the solver draws again, from where its source stands
    a, b = make_solver(built, case), make_solver(built, case)
    a.draw(5)
    a.attach_results(*a.hypotheses(a.queued()))
    a.SetRansacParameters(*case["params"])
    assert len(a.queued()) == 0
    for _ in range(len(sm) * case["set_size"]):
        b.source()                                                                  # b's source skips what a drew and dropped
    assert _run(a) == _run(b)


def test_get_problem_is_what_the_batch_call_takes(built):
    case = pc.BY_NAME["n65_s6"]
    s = make_solver(built, case)
    p2d, p3d, e, K, ms, sm = s.problem()
    assert p2d.tobytes() == case["p2d"].tobytes() and p3d.tobytes() == case["p3d"].tobytes() and ms == 6 and len(sm) == 0
    assert e.tobytes() == (case["sigma2"] * np.float32(5.991)).astype(np.float32).tobytes()
    assert K.tobytes() == np.array(case["K"], np.float32).tobytes()
    for bad in ([0, 1, 2, 3, 4, 65], [-1, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 4]):
        with pytest.raises(built.OrbxError):
            s.hypothesis(bad)


# ------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", sorted(pc.ORACLE))
def test_hypothesis_equals_the_oracle_at_set_size_6_and_8(built, name):
    case = pc.ORACLE[name]
    s = make_solver(built, case)
    fx, fy, cx, cy = (float(v) for v in case["K"])
    e = s.max_errors()
    p3d, p2d = case["p3d"], case["p2d"]
    for sm in case["samples"]:
        R, t, inl, n = s.hypothesis(sm)
        Ro, to, _ = po.epnp(p3d[sm].astype(np.float64), p2d[sm].astype(np.float64), fx, fy, cx, cy)
        assert np.abs(R - Ro).max() <= 1e-8 and np.abs(t - to).max() <= 1e-8, (name, sm)
        # CheckInliers (src/PnPsolver.cc:312-344) with its float / double mix, from the oracle's pose
        X = p3d.astype(np.float64)
        Xc = (X @ Ro[0] + to[0]).astype(np.float32)
        Yc = (X @ Ro[1] + to[1]).astype(np.float32)
        iz = (1.0 / (X @ Ro[2] + to[2])).astype(np.float32)
        ue = cx + fx * Xc.astype(np.float64) * iz
        ve = cy + fy * Yc.astype(np.float64) * iz
        dx, dy = (p2d[:, 0] - ue).astype(np.float32), (p2d[:, 1] - ve).astype(np.float32)
        err2 = dx * dx + dy * dy
        near = np.abs(err2 - e) <= 1e-4 * e                                          # a flag a 1e-8 pose difference may turn
        flags = err2 < e
        assert np.array_equal(inl[~near], flags[~near]) and n == int(inl.sum()), (name, sm)


# ------------------------------------------------------------------------------------------------- orbm_pnp_hypotheses' checks
def _args(built, names=(("n65_s6", 5), ("n5_s5", 1), ("n64_s4", 5))):
    probs = []
    for name, h in names:
        case = pc.BY_NAME[name]
        s = make_solver(built, case)
        p2d, p3d, e, K, ms, _ = s.problem()
        probs.append((p2d, p3d, e, K, ms, case["samples"][:h]))
    keys = ("off", "p2d", "p3d", "e", "cams", "hyp_off", "sm", "mask_off")
    a = dict(zip(keys, built.ORBmatcher.pack_pnp_problems(probs)))
    H, MW = int(a["hyp_off"][-1]), int(a["mask_off"][-1])
    a.update(B=len(probs), H=H, cnt=np.full(H, 77, np.int32), Rt=np.full((H, 12), 77.0), masks=np.full(MW, 77, np.uint32))
    return a


ORDER = ("off", "p2d", "p3d", "e", "cams", "hyp_off", "sm", "mask_off", "cnt", "Rt", "masks")


def _host(L, a, B=None):
    return L.orbm_pnp_hypotheses(None, a["B"] if B is None else B, *[p(a[k]) for k in ORDER])


def _device(L, a, B=None, H=None):
    return L.orbm_pnp_hypotheses_device(None, a["B"] if B is None else B, a["H"] if H is None else H, *[p(a[k]) for k in ORDER], None)


def _untouched(a):
    return (a["cnt"] == 77).all() and (a["Rt"] == 77).all() and (a["masks"] == 77).all()


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle every bad argument still gets ORBX_E_INVALID and a text, and the empty batches are ORBX_OK."""
    L = built.lib()
    E, OK = built.ORBX_E_INVALID, built.ORBX_OK
    a = _args(built)
    assert built.PNP_CAM_DTYPE.itemsize == 20 and a["sm"].shape == (11, 8) and (a["sm"][:5, 6:] == -1).all()
    assert _host(L, a, B=-1) == E and _device(L, a, B=-1) == E and _device(L, a, H=-1) == E
    assert _host(L, a, B=0) == OK and _device(L, a, B=0) == OK and _device(L, a, H=0) == OK and _untouched(a)
    none = _args(built, (("n65_s6", 0), ("n5_s5", 0)))
    assert _host(L, none) == OK and _untouched(none)                               # no hypothesis at all
    for key in ORDER:
        b = dict(a)
        b[key] = None
        assert _host(L, b) == E and b"NULL" in L.orbm_last_error(), key
        assert _device(L, b) == E and b"NULL" in L.orbm_last_error(), key
    for key, at, val, text in (("off", 1, 80, b"off not monotone"), ("off", 0, 1, b"must be 0"), ("hyp_off", 2, 1, b"hyp_off not monotone"),
                               ("hyp_off", 0, 1, b"must be 0"), ("mask_off", 1, 14, b"mask_off"), ("mask_off", 0, 1, b"must be 0")):
        b = dict(a)
        b[key] = a[key].copy()
        b[key][at] = val
        if key == "off" and at == 1:
            b[key][2] = 70
        assert _host(L, b) == E and text in L.orbm_last_error(), (key, at, L.orbm_last_error())
    for at, val, text in (((0, 0), -1, b"outside"), ((1, 5), 65, b"outside"), ((5, 2), 5, b"outside"), ((6, 3), 64, b"outside"),
                          ((2, 1), int(a["sm"][2, 0]), b"repeated"), ((5, 4), int(a["sm"][5, 0]), b"repeated")):
        b = dict(a)
        b["sm"] = a["sm"].copy()
        b["sm"][at] = val
        assert _host(L, b) == E and text in L.orbm_last_error(), (at, L.orbm_last_error())
    for set_size in (3, 9, 0, -1):                                                   # the kernel takes samples of 4 to 8
        b = dict(a)
        b["cams"] = a["cams"].copy()
        b["cams"]["set_size"][1] = set_size
        assert _host(L, b) == E and b"set_size" in L.orbm_last_error(), set_size
    odd = np.zeros(64, np.uint8)
    for k, shift in ((1, 1), (9, 4), (7, 4)):                                      # p2d off by one byte; Rt and mask_off off by four
        args = [p(a[key]) for key in ORDER]
        args[k] = C.c_void_p((odd.ctypes.data + 7) // 8 * 8 + shift)
        assert L.orbm_pnp_hypotheses_device(None, a["B"], a["H"], *args, None) == E and b"aligned" in L.orbm_last_error(), k
    assert _untouched(a)
    # the NULL-handle rule of the other batch calls: good arguments need the GPU
    import torch
    want = E if torch.cuda.is_available() else built.ORBX_E_HIP
    assert _host(L, a) == want and _device(L, a) == want and _untouched(a)
    if want != E:
        assert b"no CPU path" in L.orbm_last_error()


# ------------------------------------------------------------------------------------------------- sanitizers, stand-alone
def test_the_host_solver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pnp_asan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cxx", "pnp_asan_main.cc"), os.path.join(CSRC, "orbp.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pnp_asan_main ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
