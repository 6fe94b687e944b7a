"""No-GPU checks of the batched Optimizer::PoseOptimization (include/orbm.h, orbm_pose_optimization_batch): the two exports and
their declarations, the argument checks made before any device work, the loud failure without a GPU, and the cases of
tests/pose_cases.py against oracle/pose_oracle.py on the host path (the checker of tests/test_pose_batch_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_cases as pc
import pose_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_two_symbols_are_exported_and_declared(built):
    lib = C.CDLL(built.LIB_PATH)
    assert hasattr(lib, "orbm_pose_optimization_batch") and hasattr(lib, "orbm_pose_optimization_batch_device")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+orbm_pose_optimization_batch\s*\(", text) and re.search(r"\bint\s+orbm_pose_optimization_batch_device\s*\(", text)
    assert "typedef struct { float fx, fy, cx, cy, bf; } orbm_pose_camera;" in text
    assert all(hasattr(built.ORBmatcher, a) for a in ("pose_optimization_batch", "pose_optimization_batch_device", "pack_pose_problems"))
    assert built.POSE_CAM_DTYPE.itemsize == 20


def _args(built, with_stereo=True):
    problems = pc.mixed()[3:7] if with_stereo else [pc.fixed_point(), pc.all_outliers()]
    off, obs, ur, s2, xw, cams, T = built.ORBmatcher.pack_pose_problems(problems)
    n = int(off[-1])
    return dict(B=len(problems), off=off, obs=obs, ur=ur, s2=s2, xw=xw, cams=cams, T=T, out=np.full(n + 16, 77, np.uint8),
                good=np.full(len(problems), 77, np.int32))


INPUTS = ("off", "obs", "ur", "s2", "xw", "cams")
OUTPUTS = ("T", "out", "good")


def _host(Lb, a, handle=None, B=None):
    return Lb.orbm_pose_optimization_batch(handle, a["B"] if B is None else B, *[p(a[k]) for k in INPUTS + OUTPUTS])


def _device(Lb, a, handle=None, B=None):
    return Lb.orbm_pose_optimization_batch_device(handle, a["B"] if B is None else B, *[p(a[k]) for k in INPUTS + OUTPUTS], None)


def _untouched(a, T0):
    return (a["out"] == 77).all() and (a["good"] == 77).all() and np.array_equal(a["T"], T0)


def test_pack_pose_problems_is_the_csr_form():
    import my_slam_amd as ms
    problems = pc.mixed()
    off, obs, ur, s2, xw, cams, T = ms.ORBmatcher.pack_pose_problems(problems)
    assert list(np.diff(off)) == list(pc.MIXED_SIZES) and off[0] == 0
    assert len(obs) == len(ur) == len(s2) == len(xw) == off[-1] and T.shape == (13, 16)
    for k, pr in enumerate(problems):
        sl = slice(off[k], off[k + 1])
        assert np.array_equal(obs[sl], pr[0]) and np.array_equal(s2[sl], pr[1]) and np.array_equal(xw[sl], pr[2])
        assert np.array_equal(ur[sl], pr[8] if pr[8] is not None else np.full(len(pr[0]), -1, np.float32))
        assert tuple(cams[k]) == tuple(np.float32(v) for v in pr[3:7] + (pr[9],))
        assert np.array_equal(T[k].reshape(4, 4), pr[7])
    assert len({float(c["bf"]) for c in cams if c["bf"] > 0}) == 2 and len({float(c["fx"]) for c in cams}) == 2
    assert ms.ORBmatcher.pack_pose_problems([pc.fixed_point()])[2] is None           # no problem has u_right: all monocular


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument still gets ORBX_E_INVALID and a text."""
    Lb = built.lib()
    E, OK = built.ORBX_E_INVALID, built.ORBX_OK
    a = _args(built)
    T0 = a["T"].copy()
    for call in (_host, _device):
        assert call(Lb, a, B=-1) == E and b"n_problems=-1" in Lb.orbm_last_error()
        assert call(Lb, a, B=0) == OK
        none = dict.fromkeys(a)
        assert call(Lb, none, B=0) == OK                                            # n_problems == 0 reads no pointer
        for key in INPUTS + OUTPUTS:
            if key == "ur":
                continue                                                            # NULL: all monocular
            b = dict(a)
            b[key] = None
            assert call(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key
    b = _args(built)
    b["off"][0] = 1
    assert _host(Lb, b) == E and b"off[0]" in Lb.orbm_last_error() and _untouched(b, T0)
    b = _args(built)
    b["off"][2] = b["off"][1] - 1
    assert _host(Lb, b) == E and b"not monotone at 1" in Lb.orbm_last_error() and _untouched(b, T0)
    b = _args(built)
    stereo = int(np.flatnonzero(b["ur"][b["off"][0]:b["off"][1]] >= 0)[0])          # problem 0 (1500 edges) has stereo edges
    b["cams"]["bf"][0] = 0.0
    assert _host(Lb, b) == E and b"bf is 0" in Lb.orbm_last_error() and b"problem 0" in Lb.orbm_last_error() and _untouched(b, T0)
    b["ur"][b["off"][0]:b["off"][1]] = -1                                           # no stereo edge left in it: bf == 0 is fine
    assert _host(Lb, b) != E or b"bf" not in Lb.orbm_last_error()
    b["cams"]["bf"][0] = 0.0
    b["ur"] = None
    assert _host(Lb, b) != E or b"bf" not in Lb.orbm_last_error()
    assert stereo >= 0 and _untouched(a, T0)
    odd = np.zeros(64, np.uint8)                                                    # the device form wants 4-byte aligned arrays
    c = dict(a)
    assert Lb.orbm_pose_optimization_batch_device(None, c["B"], p(c["off"]), C.c_void_p(odd.ctypes.data + 1), *[p(c[k]) for k in INPUTS[2:] + OUTPUTS],
                                                  None) == E and b"aligned" in Lb.orbm_last_error()


def test_the_entry_points_fail_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    for stereo in (True, False):
        a = _args(built, stereo)
        T0 = a["T"].copy()
        for call in (_host, _device):
            assert call(Lb, a) == built.ORBX_E_HIP
            assert b"no CPU path" in Lb.orbm_last_error()
            assert _untouched(a, T0)                                                # no half answer


@pytest.mark.parametrize("name", sorted(pc.all_cases()))
def test_pose_cases_host_equals_oracle(built, name):
    """the checker of the GPU tests is itself held to oracle/pose_oracle.py, on every case they use, at the bar of tests/test_pose.py"""
    for k, (pr, got) in enumerate(zip(pc.cases()[name], pc.host(built, name))):
        obs, inv_s2, xw, fx, fy, cx, cy, T0, ur, bf = pr
        T2, o2, n2 = po.pose_optimization(obs, ur, inv_s2, xw, fx, fy, cx, cy, bf, T0)
        pc.assert_same(got, (T2, o2.astype(bool), n2), pr, "%s[%d]" % (name, k))
        if len(obs) < 3:
            assert got[2] == 0 and np.array_equal(got[0], T0) and not got[1].any()
    if name == "all_outliers":
        # the last round ran on an empty active set: nothing was optimised, the restart pose comes back (through the quaternion)
        assert got[2] == 0 and got[1].all() and np.abs(got[0] - pr[7]).max() < 1e-6
    if name == "fixed_point":
        assert got[2] == 100 and not got[1].any() and np.abs(got[0] - pr[7]).max() < 1e-5
    if name == "mixed":
        assert [len(q[0]) for q in pc.cases()[name]] == list(pc.MIXED_SIZES)
