"""No-GPU checks of Optimizer::OptimizeSim3 (include/orbp.h orbp_optimize_sim3, include/orbm.h orbm_optimize_sim3_batch): the host
path against the oracle tests/optimize_sim3_oracle.py on every case of tests/optimize_sim3_cases.py (identical flags, identical
nIn, S12 within the bar of tests/golden/sim3opt/tolerance.json), the exports and their declarations, orbp_sim3_from_rts against
numpy, and the argument checks made before any device work."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import optimize_sim3_cases as sc
import optimize_sim3_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = json.load(open(os.path.join(ROOT, "tests", "golden", "sim3opt", "tolerance.json")))
BARS = tuple(TOL["bar"][k] for k in ("quaternion", "translation", "scale"))


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_symbols_are_exported_and_declared(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("orbm_optimize_sim3_batch", "orbm_optimize_sim3_batch_device", "orbp_optimize_sim3", "orbp_sim3_from_rts"):
        assert hasattr(lib, name), name
    orbm = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    orbp = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+orbm_optimize_sim3_batch\s*\(", orbm) and re.search(r"\bint\s+orbm_optimize_sim3_batch_device\s*\(", orbm)
    assert re.search(r"\bint\s+orbp_optimize_sim3\s*\(", orbp) and re.search(r"\bint\s+orbp_sim3_from_rts\s*\(", orbp)
    assert all(hasattr(built.ORBmatcher, a) for a in ("optimize_sim3_batch", "optimize_sim3_batch_device", "pack_sim3opt_problems"))
    assert hasattr(built, "OptimizeSim3") and hasattr(built, "sim3_from_rts")


def test_the_tolerance_file_is_what_the_script_measures():
    """4 x the spread of the oracle's two summation orders over the cases, per part of S12"""
    assert TOL["factor"] == 4
    for k in ("quaternion", "translation", "scale"):
        assert TOL["bar"][k] == 4 * TOL["spread"][k] and 0 < TOL["spread"][k] < 1e-5
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "measure_sim3opt_spread.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_cases_cover_what_they_should():
    cases = sc.cases()
    assert [len(q[0]) for q in cases["mixed"]] == list(sc.MIXED_SIZES)
    assert len({tuple(q[6]) for q in cases["mixed"]} | {tuple(q[7]) for q in cases["mixed"]}) == 2          # two cameras
    assert {q[9] for q in cases["mixed"]} == {True, False} and {round(q[8], 3) for q in cases["mixed"]} == {10.0, 5.991}
    for n in sc.SINGLE_SIZES:
        prs, orc = cases["single_%d" % n], sc.oracle("single_%d" % n)
        assert len(prs) == 8 and all(len(q[0]) == n for q in prs)
        if n < 10:
            assert all(o[0] is None and o[2] == 0 for o in orc)
        if n >= 63:                                           # the outlier variants removed pairs: optimize(10) ran
            assert all(o[1][:n // 5].all() and o[0] is not None for o in orc[1::2])


@pytest.mark.parametrize("name", sorted(sc.all_cases()))
def test_host_equals_oracle(built, name):
    for k, (pr, got, orc) in enumerate(zip(sc.cases()[name], sc.host(built, name), sc.oracle(name))):
        sc.assert_same(got, orc[:3], BARS, "%s[%d] n=%d" % (name, k, len(pr[0])))
        if orc[0] is None:                                    # :1211-1212: g2oS12 stays as it came, bit for bit
            assert got[2] == 0 and got[0].tobytes() == np.asarray(pr[10], np.float64).tobytes()
        else:
            assert got[0].tobytes() != np.asarray(pr[10], np.float64).tobytes() or name == "fixed_point"
    if name == "too_few_left":
        assert got[1][:6].all() and got[1].sum() == 6 and got[2] == 0
    if name == "fixed_point":
        assert got[2] == 100 and not got[1].any() and max(sc.diff3(got[0], pr[10])) < 1e-5


def test_fix_scale_keeps_the_scale_bit_for_bit(built):
    for name in ("single_64", "single_600"):
        for pr, got in zip(sc.cases()[name], sc.host(built, name)):
            if pr[9] and got[2] > 0:
                assert got[0][7] == pr[10][7]
            elif got[2] > 0:
                assert got[0][7] != pr[10][7]


def test_sim3_from_rts_equals_numpy(built):
    rng = np.random.default_rng(3)
    for k in range(40):
        w = rng.normal(size=3) * (3.0 if k % 2 else 0.3)      # large angles reach the branches of a negative trace
        R = sc.rot(w).astype(np.float32)
        t = rng.uniform(-3, 3, 3).astype(np.float32)
        s = float(np.float32(rng.uniform(0.5, 2)))
        got = built.sim3_from_rts(R, t, s)
        want = np.concatenate([so.quat_from_R(R.astype(np.float64)), t.astype(np.float64), [s]])
        assert np.array_equal(got, want), (k, got, want)
    assert built.lib().orbp_sim3_from_rts(None, p(t), 1.0, p(np.zeros(8))) == built.ORBX_E_INVALID


def _args(built):
    problems = sc.cases()["mixed"][3:7]
    names = ("off", "x1", "x2", "o1", "o2", "s1", "s2", "cams", "th2", "fix", "S")
    a = dict(zip(names, built.ORBmatcher.pack_sim3opt_problems(problems)))
    a["B"] = len(problems)
    a["flags"] = np.full(int(a["off"][-1]) + 16, 77, np.uint8)
    a["n_in"] = np.full(len(problems), 77, np.int32)
    return a


KEYS = ("off", "x1", "x2", "o1", "o2", "s1", "s2", "cams", "th2", "fix", "S", "flags", "n_in")


def _host(Lb, a, B=None):
    return Lb.orbm_optimize_sim3_batch(None, a["B"] if B is None else B, *[p(a[k]) for k in KEYS])


def _device(Lb, a, B=None):
    return Lb.orbm_optimize_sim3_batch_device(None, a["B"] if B is None else B, *[p(a[k]) for k in KEYS], None)


def _untouched(a, S0):
    return (a["flags"] == 77).all() and (a["n_in"] == 77).all() and a["S"].tobytes() == S0.tobytes()


def test_batch_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument still gets ORBX_E_INVALID and a text."""
    Lb = built.lib()
    E, OK = built.ORBX_E_INVALID, built.ORBX_OK
    a = _args(built)
    S0 = a["S"].copy()
    for call in (_host, _device):
        assert call(Lb, a, B=-1) == E and b"n_problems=-1" in Lb.orbm_last_error()
        assert call(Lb, a, B=0) == OK
        assert call(Lb, dict.fromkeys(a), B=0) == OK                                # n_problems == 0 reads no pointer
        for key in KEYS:
            b = dict(a)
            b[key] = None
            assert call(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key
    b = _args(built)
    b["off"][0] = 1
    assert _host(Lb, b) == E and b"off[0]" in Lb.orbm_last_error() and _untouched(b, S0)
    b = _args(built)
    b["off"][2] = b["off"][1] - 1
    assert _host(Lb, b) == E and b"not monotone at 1" in Lb.orbm_last_error() and _untouched(b, S0)
    for bad in (np.nan, np.inf):
        b = _args(built)
        b["S"][2, 5] = bad
        S1 = b["S"].copy()
        assert _host(Lb, b) == E and b"S12 of problem 2 is not finite" in Lb.orbm_last_error() and _untouched(b, S1)
    assert _untouched(a, S0)
    odd = np.zeros(256, np.uint8)                                                   # the device form wants aligned arrays
    c = dict(a)
    args = [p(c[k]) for k in KEYS]
    args[1] = C.c_void_p(odd.ctypes.data + 1)
    assert Lb.orbm_optimize_sim3_batch_device(None, c["B"], *args, None) == E and b"aligned" in Lb.orbm_last_error()
    args = [p(c[k]) for k in KEYS]
    args[10] = C.c_void_p(a["S"].ctypes.data + 4)
    assert Lb.orbm_optimize_sim3_batch_device(None, c["B"], *args, None) == E and b"8-byte" in Lb.orbm_last_error()


def test_the_batch_fails_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    a = _args(built)
    S0 = a["S"].copy()
    for call in (_host, _device):
        assert call(Lb, a) == built.ORBX_E_HIP
        assert b"no CPU path" in Lb.orbm_last_error()
        assert _untouched(a, S0)                                                    # no half answer


def test_host_argument_checks(built):
    Lb = built.lib()
    pr = sc.cases()["single_64"][0]
    arrs = [np.ascontiguousarray(x) for x in pr[:8]]
    S = np.array(pr[10])
    flags = np.full(64, 77, np.uint8)

    def call(arrs=arrs, n=64, S=S, flags=flags):
        return Lb.orbp_optimize_sim3(n, *[p(x) for x in arrs], pr[8], 1, p(S), p(flags))

    for k in range(8):
        b = list(arrs)
        b[k] = None
        assert call(b) == built.ORBX_E_INVALID and b"NULL" in Lb.orbp_last_error(), k
    assert call(S=None) == built.ORBX_E_INVALID and call(flags=None) == built.ORBX_E_INVALID and call(n=-1) == built.ORBX_E_INVALID
    for bad in (np.nan, -np.inf):
        S1 = S.copy()
        S1[7] = bad
        assert call(S=S1) == built.ORBX_E_INVALID and b"not finite" in Lb.orbp_last_error()
    assert (flags == 77).all() and np.array_equal(S, pr[10])
    assert call(n=0, arrs=[None] * 6 + arrs[6:], flags=None) == 0 and np.array_equal(S, pr[10])      # no edges: nothing is optimised
    with pytest.raises(built.OrbxError):
        built.OptimizeSim3(pr[0][:5], *pr[1:])
