"""No-GPU checks of Optimizer::LocalBundleAdjustment (include/orbp.h orbp_local_bundle_adjustment, include/orbm.h
orbm_local_bundle_adjustment): the host path against the oracle tests/lba_oracle.py on every case of tests/lba_cases.py (identical
erase flags, identical counts, poses / points / final chi2 within the bar of tests/golden/lba/tolerance.json), the semantics the
header lists (stale errors, vertices without active edges, fixed key frames, stop at entry), the exports and their declarations,
and the argument checks made before any work."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lba_cases as lc
import lba_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = json.load(open(os.path.join(ROOT, "tests", "golden", "lba", "tolerance.json")))
BARS = tuple(TOL["bar"][k] for k in lc.KEYS)


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_symbols_are_exported_and_declared(built):
    lib = C.CDLL(built.LIB_PATH)
    assert hasattr(lib, "orbp_local_bundle_adjustment") and hasattr(lib, "orbm_local_bundle_adjustment")
    orbm = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    orbp = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+orbm_local_bundle_adjustment\s*\(", orbm) and re.search(r"\bint\s+orbp_local_bundle_adjustment\s*\(", orbp)
    assert hasattr(built, "LocalBundleAdjustment") and hasattr(built, "pack_lba_problem")
    assert all(hasattr(built.ORBmatcher, a) for a in ("local_bundle_adjustment", "pack_lba_problem"))
    assert C.sizeof(built.LbaStats) == 40 and C.sizeof(built.LbaProblem) == 80


def test_the_tolerance_file_is_what_the_script_measures():
    """4 x the spread of the oracle's two summation orders over the cases, per part of the result"""
    assert TOL["factor"] == 4
    for k in lc.KEYS:
        assert TOL["bar"][k] == 4 * TOL["spread"][k] and 0 < TOL["spread"][k] < 1e-3
    assert set(TOL["scale"]) == set(lc.SCALE_NAMES)                     # each scale case has bars of its own, made the same way
    for name in lc.SCALE_NAMES:
        for k in lc.KEYS:
            s = TOL["scale"][name]
            assert s["bar"][k] == 4 * s["spread"][k] and 0 < s["spread"][k] < 1e-3 and s["worst_case"][k] == name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "measure_lba_spread.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_cases_cover_what_they_should():
    cs = lc.cases()
    free = {n: int((np.asarray(c["local_fixed"]) == 0).sum()) for n, c in cs.items()}
    assert {1, 2, 11, 43} <= set(free.values()) and 0 in free.values()
    assert {0, 1, 63, 64, 65, 257, 1500} <= {len(c["xw"]) for c in cs.values()}
    for name in ("k11_p257_mixed", "k43_p1500_mixed"):
        deg = np.diff(cs[name]["edge_off"])
        assert deg.min() == 2 and deg.max() == len(cs[name]["Tcw"])                    # degree 2 up to all key frames
        f = lc.oracle(name)[0]
        assert f["stats"]["n_level1"] >= len(deg) // 10 and f["stats"]["iterations"][1] == 10, f["stats"]
    assert (cs["k1_p63_mono"]["u_right"] < 0).all() and (cs["k2_p64_stereo"]["u_right"] >= 0).all()
    ur, off = cs["k2_p65_mixed"]["u_right"], cs["k2_p65_mixed"]["edge_off"]
    assert any((ur[a:b] < 0).any() and (ur[a:b] >= 0).any() for a, b in zip(off[:-1], off[1:]))       # mixed within a point
    assert lc.has_bad_point(cs["bad_point"], lc.oracle("bad_point")[0]) and lc.has_bad_kf(cs["bad_kf"], lc.oracle("bad_kf")[0])
    assert lc.has_behind(cs["behind"], lc.oracle("behind")[0]) and len(lc.stale_flips(cs["stale_flip"], lc.oracle("stale_flip")[0])) > 0
    assert cs["local_id0"]["local_fixed"].sum() == 1 and len(cs["local_id0"]["Tcw"]) == len(cs["local_id0"]["local_fixed"])
    # every tolerance case fixes the scale: two fixed key frames at least, or stereo edges
    for name in lc.TOLERANCE_NAMES:
        c = cs[name]
        n_fixed = len(c["Tcw"]) - free[name]
        assert n_fixed >= 2 or (c["u_right"] >= 0).any() or len(c["xw"]) == 0, name
    g = cs["gauge_mono"]
    assert (g["u_right"] < 0).all() and len(g["Tcw"]) - free["gauge_mono"] == 1
    for name in lc.NAMES:
        f, r = lc.oracle(name)
        assert min(f["margin"], r["margin"]) > lc.MARGIN and f["transcript"] == r["transcript"], name


def test_the_scale_case_is_at_the_cap_and_dense(built):
    """ORBM_LBA_MAX_LOCAL free key frames (768 unknowns: three strides of k_lba_solve's 256 threads), some fixed ones, every key frame
    with more than 64 edges, every tile of S occupied, a tenth gross outliers that the first round flags, and a second round"""
    pr = lc.case("scale_k128")
    f, r = lc.oracle("scale_k128")
    cap = int(re.search(r"#define\s+ORBM_LBA_MAX_LOCAL\s+(\d+)", open(os.path.join(ROOT, "include", "orbm.h")).read()).group(1))
    assert len(pr["local_fixed"]) == cap == 128 and pr["local_fixed"].sum() == 0 and len(pr["Tcw"]) == cap + 8 and 6 * cap == 3 * 256
    fewest, tiles = lc.density(pr)
    assert fewest > 64 and tiles >= 0.25
    assert min(f["margin"], r["margin"]) > lc.MARGIN and f["transcript"] == r["transcript"]
    assert f["stats"]["n_level1"] >= len(pr["edge_kf"]) // 20 and f["stats"]["iterations"][1] >= 1 and f["stats"]["second_round"] == 1


def scale_bars(name):
    return tuple(TOL["scale"][name]["bar"][k] for k in lc.KEYS)


@pytest.mark.parametrize("name", lc.NAMES + lc.SCALE_NAMES)
def test_host_equals_oracle(built, name):
    f = lc.oracle(name)[0]
    bars = scale_bars(name) if name in lc.SCALE_NAMES else BARS
    lc.assert_same(lc.host(built, name), f["Tcw"], f["xw"], f["erase"], f["stats"], bars, name, coordinates=name not in lc.GAUGE)


def test_stale_errors_decide_the_final_pass(built):
    """a level-1 edge keeps the first round's error: its erase flag is set although its chi2 at the final estimates is below the
    threshold (Optimizer.cc:715-743 reads e->chi2(), which nobody recomputed)"""
    pr, (f, _) = lc.case("stale_flip"), lc.oracle("stale_flip")
    flips = lc.stale_flips(pr, f)
    erase = lc.host(built, "stale_flip")[3]
    assert len(flips) > 0 and erase[flips].all()
    # recomputed from the host's own outputs the flags would be clear
    g = lo.Graph(dict(pr, Tcw=np.concatenate([lc.host(built, "stale_flip")[1], pr["Tcw"][len(pr["local_fixed"]):]]),
                      xw=lc.host(built, "stale_flip")[2]), "forward")
    fresh = g.chi2_of(g.errors_of(flips), flips)
    assert (fresh < np.where(pr["u_right"][flips] < 0, lo.TH_MONO, lo.TH_STEREO)).all()


def test_an_edge_behind_its_camera_is_erased_by_depth_alone(built):
    pr, (f, _) = lc.case("behind"), lc.oracle("behind")
    e = len(pr["edge_kf"]) - 1
    assert lc.host(built, "behind")[3][e] and f["stale_chi2"][e] < 0.5 * lo.TH_MONO


def _first_round(pr):
    """the oracle's estimates after optimize(5)"""
    g = lo.Graph(pr, "forward")
    g.optimize(0, 5, {"iterations": [0, 0], "trials": [0, 0], "lambda": 0.0, "chi2": 0.0})
    return g


def test_vertices_without_active_edges_stay_where_the_first_round_left_them(built):
    """the second round does not touch a point or key frame whose every edge is level 1: the product's final estimate of it is the
    oracle's after optimize(5) (to the bar and the output's float rounding), while its neighbours went on moving"""
    pr, g = lc.case("bad_point"), _first_round(lc.case("bad_point"))
    xw = lc.host(built, "bad_point")[2].astype(np.float64)
    assert np.abs(xw[-1] - g.X[-1]).max() <= BARS[2] + 2.0 ** -24 * np.abs(g.X[-1]).max()
    assert np.abs(xw[-1] - pr["xw"][-1]).max() > 1e-3 and np.abs(xw[:-1] - g.X[:-1]).max() > 100 * BARS[2]
    pr, g = lc.case("bad_kf"), _first_round(lc.case("bad_kf"))
    k = pr["k_bad"]
    Tcw = lc.host(built, "bad_kf")[1].astype(np.float64)
    assert np.abs(Tcw[k, :3, 3] - g.t[k]).max() <= BARS[1] + 2.0 ** -24 * np.abs(g.t[k]).max()
    assert np.abs(Tcw[k, :3, :3] - g.R[k]).max() <= BARS[0] + 2.0 ** -24
    assert np.abs(Tcw[k, :3, 3] - pr["Tcw"][k, :3, 3]).max() > 1e-3
    assert max(np.abs(Tcw[j, :3, 3] - g.t[j]).max() for j in range(k)) > 100 * BARS[1]


def test_fixed_key_frames_come_back_as_they_went_in(built):
    """a local key frame with mnId == 0 is fixed: its pose is the input's, through the quaternion and back"""
    pr = lc.case("local_id0")
    k = int(np.flatnonzero(pr["local_fixed"])[0])
    Tcw = lc.host(built, "local_id0")[1]
    assert np.abs(Tcw[k] - pr["Tcw"][k]).max() <= 2.0 ** -22 and np.abs(Tcw[0] - pr["Tcw"][0]).max() > 1e-4
    code, Tcw, xw, erase, stats = lc.host(built, "no_points")
    assert code == 0 and stats["iterations"] == (0, 0) and len(xw) == 0 and len(erase) == 0
    assert np.abs(Tcw - lc.case("no_points")["Tcw"][:2]).max() <= 2.0 ** -22
    code, Tcw, xw, erase, stats = lc.host(built, "no_free")
    assert stats["iterations"] == (5, 0) and erase.all() and np.abs(xw - lc.case("no_free")["xw"]).max() > 1e-3     # points alone moved


def _raw(built, pr, stop=None):
    return lc.raw_call(built.lib().orbp_local_bundle_adjustment, built, pr, stop=stop)


def test_guards_survive_and_stop_at_entry_writes_nothing(built):
    pr = lc.case("k2_p65_mixed")
    code, (T, x, er, st), ok, a = _raw(built, pr)
    want = lc.host(built, "k2_p65_mixed")
    assert code == built.ORBP_LBA_DONE and ok and T.tobytes() == want[1].tobytes() and x.tobytes() == want[2].tobytes()
    assert np.array_equal(er.astype(bool), want[3])
    code, (T, x, er, st), ok, a = _raw(built, pr, stop=np.ones(1, np.uint8))
    assert code == built.ORBP_LBA_STOPPED == 1 and ok
    assert (T == 7.25).all() and x.tobytes() == a["xw"].tobytes() and (er == 0x5A).all() and (st == 0x5A).all()
    code, (T, x, er, st), ok, a = _raw(built, pr, stop=np.zeros(1, np.uint8))
    assert code == 0 and T.tobytes() == want[1].tobytes()


def test_invalid_arguments(built):
    Lb = built.lib()
    E_INV = built.ORBX_E_INVALID
    pr = lc.case("k2_p65_mixed")

    def call(mutate=None, null=None, T_null=False, x_null=False, e_null=False):
        s, a = built.pack_lba_problem({k: np.array(v) for k, v in pr.items()})         # copies: the cases are shared
        if mutate:
            mutate(s, a)
        if null:
            setattr(s, null, None)
        T = np.full((len(pr["local_fixed"]), 16), 7.25, np.float32)
        er = np.full(len(a["edge_kf"]), 0x5A, np.uint8)
        x0 = a["xw"].copy()
        rc = Lb.orbp_local_bundle_adjustment(C.byref(s), None if T_null else p(T), None if x_null else p(a["xw"]), None if e_null else p(er),
                                             None, None)
        assert rc == 0 or ((T == 7.25).all() and (er == 0x5A).all() and a["xw"].tobytes() == x0.tobytes())     # refused before any work
        return rc, Lb.orbp_last_error()

    assert call()[0] == 0
    assert Lb.orbp_local_bundle_adjustment(None, None, None, None, None, None) == E_INV
    for field in ("local_fixed", "Tcw", "cam", "edge_off", "edge_kf", "obs", "u_right", "inv_sigma2"):
        rc, text = call(null=field)
        assert rc == E_INV and b"NULL" in text, field
    for kw in ("T_null", "x_null", "e_null"):
        assert call(**{kw: True})[0] == E_INV
    for field in ("n_local", "n_fixed", "n_points"):
        rc, text = call(lambda s, a, f=field: setattr(s, f, -1))
        assert rc == E_INV and b"negative" in text

    def kf_out(s, a):
        a["edge_kf"][5] = s.n_local + s.n_fixed
    assert call(kf_out)[0] == E_INV and b"outside" in Lb.orbp_last_error()

    def kf_neg(s, a):
        a["edge_kf"][0] = -1
    assert call(kf_neg)[0] == E_INV

    def kf_twice(s, a):
        a["edge_kf"][1] = a["edge_kf"][0]
    assert call(kf_twice)[0] == E_INV and b"twice" in Lb.orbp_last_error()

    def off0(s, a):
        a["edge_off"][0] = 1
    assert call(off0)[0] == E_INV and b"edge_off[0]" in Lb.orbp_last_error()

    def off_down(s, a):
        a["edge_off"][3] = a["edge_off"][2] - 1
    assert call(off_down)[0] == E_INV and b"not monotone at 2" in Lb.orbp_last_error()
    for bad in (np.nan, np.inf):
        def pose(s, a, bad=bad):
            a["Tcw"][1, 7] = bad
        assert call(pose)[0] == E_INV and b"pose of key frame 1" in Lb.orbp_last_error()

        def point(s, a, bad=bad):
            a["xw"][4, 2] = bad
        s, a = built.pack_lba_problem({k: np.array(v) for k, v in pr.items()})
        a["xw"][4, 2] = bad
        T = np.zeros((s.n_local, 16), np.float32)
        er = np.zeros(len(a["edge_kf"]), np.uint8)
        assert Lb.orbp_local_bundle_adjustment(C.byref(s), p(T), p(a["xw"]), p(er), None, None) == E_INV
        assert b"point 4 is not finite" in Lb.orbp_last_error()
    with pytest.raises(built.OrbxError):
        built.LocalBundleAdjustment(dict(pr, obs=pr["obs"][:-1]))


def test_the_gpu_call_checks_its_arguments_before_any_device_work(built):
    """with a NULL handle (none can be made without a GPU): bad arguments get ORBX_E_INVALID, stop at entry is answered"""
    Lb = built.lib()
    pr = lc.case("k2_p65_mixed")
    s, a = built.pack_lba_problem({k: np.array(v) for k, v in pr.items()})
    T = np.full((s.n_local, 16), 7.25, np.float32)
    er = np.full(len(a["edge_kf"]), 0x5A, np.uint8)
    a["edge_off"][0] = 1
    assert Lb.orbm_local_bundle_adjustment(None, C.byref(s), p(T), p(a["xw"]), p(er), None, None) == built.ORBX_E_INVALID
    assert b"edge_off[0]" in Lb.orbm_last_error()
    a["edge_off"][0] = 0
    assert Lb.orbm_local_bundle_adjustment(None, None, None, None, None, None, None) == built.ORBX_E_INVALID
    stop = np.ones(1, np.uint8)
    assert Lb.orbm_local_bundle_adjustment(None, C.byref(s), p(T), p(a["xw"]), p(er), p(stop), None) == built.ORBP_LBA_STOPPED
    assert (T == 7.25).all() and (er == 0x5A).all()


def test_the_gpu_call_fails_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    s, a = built.pack_lba_problem(lc.case("k2_p65_mixed"))
    T = np.full((s.n_local, 16), 7.25, np.float32)
    er = np.full(len(a["edge_kf"]), 0x5A, np.uint8)
    x0 = a["xw"].copy()
    assert Lb.orbm_local_bundle_adjustment(None, C.byref(s), p(T), p(a["xw"]), p(er), None, None) == built.ORBX_E_HIP
    assert b"no CPU path" in Lb.orbm_last_error()
    assert (T == 7.25).all() and (er == 0x5A).all() and a["xw"].tobytes() == x0.tobytes()
