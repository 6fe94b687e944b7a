"""No-GPU checks of Optimizer::BundleAdjustment (include/orbp.h orbp_bundle_adjustment, include/orbm.h orbm_bundle_adjustment): the
host path against the oracle tests/ba_oracle.py on every case of tests/ba_cases.py (identical iteration and trial counts; poses,
points and final chi2 within the bar of tests/golden/ba/tolerance.json), the semantics the header lists (one round, the robust
switch, `stop` without an entry check and at every read, vertices without edges, n_iterations and its bound), the exports and their
declarations, and the argument checks made before any work."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ba_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = json.load(open(os.path.join(ROOT, "tests", "golden", "ba", "tolerance.json")))
BARS = tuple(TOL["bar"][k] for k in bc.KEYS)
PROBE = C.CFUNCTYPE(None, C.c_void_p)


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def roundtrip(Tcw):
    """Converter::toSE3Quat -> toCvMat of float poses, by the oracle's own quaternion code"""
    out = np.array(Tcw, np.float64).reshape(-1, 4, 4)
    for T in out:
        T[:3, :3] = bc.bo.lo.rot_from_float(T[:3, :3].astype(np.float32))
    return out


def test_the_symbols_are_exported_and_declared(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("orbp_bundle_adjustment", "orbm_bundle_adjustment", "orbm_bundle_adjustment_split", "orbm_spd_solve_f64"):
        assert hasattr(lib, name), name
    orbm = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    orbp = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+orbm_bundle_adjustment\s*\(", orbm) and re.search(r"\bint\s+orbm_spd_solve_f64\s*\(", orbm)
    assert re.search(r"\bint\s+orbp_bundle_adjustment\s*\(", orbp)
    assert int(re.search(r"#define\s+ORBP_BA_MAX_ITERATIONS\s+(\d+)", orbp).group(1)) == built.ORBP_BA_MAX_ITERATIONS >= 20
    assert int(re.search(r"#define\s+ORBM_BA_MAX_KFS\s+(\d+)", orbm).group(1)) == built.ORBM_BA_MAX_KFS == 512
    assert hasattr(built, "BundleAdjustment") and all(hasattr(built.ORBmatcher, a) for a in ("bundle_adjustment", "spd_solve"))
    assert C.sizeof(built.BaStats) == 24
    # the panel the cases are shaped by is the solver's
    assert int(re.search(r"#define\s+SPD_NB\s+(\d+)", open(os.path.join(ROOT, "my-slam_amd", "csrc", "orbm_spd.hip")).read()).group(1)) == bc.NB
    assert bc.NB % 6 == 0 and bc.B == bc.NB // 6


def test_the_tolerance_file_is_what_the_script_measures():
    """4 x the spread of the oracle's two summation orders over the cases, per part of the result"""
    assert TOL["factor"] == 4
    for k in bc.KEYS:
        assert TOL["bar"][k] == 4 * TOL["spread"][k] and 0 < TOL["spread"][k] < 1e-3 and TOL["worst_case"][k] in bc.NAMES
    assert set(TOL["scale"]) == set(bc.SCALE_NAMES)                     # each scale case has bars of its own, made the same way
    for name in bc.SCALE_NAMES:
        for k in bc.KEYS:
            s = TOL["scale"][name]
            assert s["bar"][k] == 4 * s["spread"][k] and 0 < s["spread"][k] < 1e-3 and s["worst_case"][k] == name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "measure_ba_spread.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_cases_cover_what_they_should():
    cs = {n: bc.case(n) for n in bc.NAMES}
    free = {n: int((np.asarray(c[0]["local_fixed"]) == 0).sum()) - (1 if "empty_kf" in c[0] else 0) for n, c in cs.items()}
    B = bc.B
    assert {1, B - 1, B, B + 1, 3 * B + 1} <= set(free.values())
    assert {0, 1, 63, 64, 65, 400} <= {len(c[0]["xw"]) for c in cs.values()}
    assert {0, 1, 10, 20} <= {c[1] for c in cs.values()} and {True, False} == {bool(c[2]) for c in cs.values()}
    assert (cs["init_map_mono"][0]["u_right"] < 0).all() and len(cs["init_map_mono"][0]["local_fixed"]) == 2
    assert (cs["k7_p63_stereo"][0]["u_right"] >= 0).all()
    ur, off = cs["k25_p400_mixed"][0]["u_right"], cs["k25_p400_mixed"][0]["edge_off"]
    assert any((ur[a:b] < 0).any() and (ur[a:b] >= 0).any() for a, b in zip(off[:-1], off[1:]))       # mixed within a point
    big = cs[bc.LARGEST][0]
    K = len(big["local_fixed"])
    assert 6 * K > 3 * bc.NB and (6 * K) % bc.NB != 0                       # four panels, the last one ragged
    assert 0 < int(np.flatnonzero(big["local_fixed"])[0]) < K - 1           # the mnId == 0 key frame in the middle of the list
    far = [abs(int(a) - int(b)) for s, e in zip(big["edge_off"][:-1], big["edge_off"][1:]) for a in big["edge_kf"][s:e] for b in big["edge_kf"][s:e]]
    assert max(far) >= 2 * B                                                # a point seen by key frames two panels apart
    assert cs["k8_p64_robust"][0] is cs["k8_p64_plain"][0]
    assert bc.oracle("nbad_stops")[0]["ended_by_nbad"] and bc.oracle("nbad_stops")[0]["stats"]["iterations"] < cs["nbad_stops"][1]
    assert bc.oracle("rejecting")[0]["stats"]["trials"] > bc.oracle("rejecting")[0]["stats"]["iterations"]
    assert bc.oracle(bc.LARGEST)[0]["stats"]["iterations"] == 10
    e = cs["empty_vertices"][0]
    assert (e["edge_kf"] != e["empty_kf"]).all() and e["edge_off"][e["empty_point"]] == e["edge_off"][e["empty_point"] + 1]
    nf = cs["n_fixed_2"][0]
    assert len(nf["Tcw"]) - len(nf["local_fixed"]) == 2 and nf["local_fixed"].sum() == 0
    assert cs["no_fixed_gauge"][0]["local_fixed"].sum() == 0 and len(cs["no_fixed_gauge"][0]["Tcw"]) == len(cs["no_fixed_gauge"][0]["local_fixed"])
    for name in bc.TOLERANCE_NAMES:                                         # every tolerance case fixes the scale
        c = cs[name][0]
        n_fix = len(c["Tcw"]) - int((np.asarray(c["local_fixed"]) == 0).sum())
        assert n_fix >= 2 or (c["u_right"] >= 0).any() or len(c["xw"]) == 0, name
    for name in bc.NAMES:
        f, r = bc.oracle(name)
        assert min(f["margin"], r["margin"]) > bc.MARGIN and f["transcript"] == r["transcript"], name


def test_the_scale_cases_are_dense_and_reach_the_cap(built):
    """49, 89 and 512 blocks of the reduced system (294, 534 and 3072 unknowns: k_spd_backward's second and third workgroup, and
    ORBM_BA_MAX_KFS = ORBM_SPD_MAX_N / 6), no key frame without edges, every key frame with more than 64, at least a quarter of the
    48 x 48 tiles below S's diagonal occupied, the key frame x point table of the cap case inside ORBM_BA_MAX_TABLE, and every
    decision of the oracle clear of its boundary in both orders"""
    cs = {n: bc.case(n) for n in bc.SCALE_NAMES}
    assert [len(c[0]["local_fixed"]) for c in cs.values()] == [49, 89, built.ORBM_BA_MAX_KFS]
    assert 6 * 49 == 6 * bc.NB + 6 and 6 * 89 == 11 * bc.NB + 6 and 6 * built.ORBM_BA_MAX_KFS == built.ORBM_SPD_MAX_N
    assert [c[1] for c in cs.values()] == [2, 1, 1]
    for name, (pr, n_it, robust) in cs.items():
        K = len(pr["local_fixed"])
        fewest, tiles = bc.density(pr)
        assert fewest > 64 and tiles >= 0.25, (name, fewest, tiles)
        assert pr["local_fixed"].sum() == 1 and 0 < int(np.flatnonzero(pr["local_fixed"])[0]) < K - 1 and len(pr["Tcw"]) == K
        assert (pr["u_right"] >= 0).any() and (pr["u_right"] < 0).any()
        assert K * len(pr["xw"]) <= built.ORBM_BA_MAX_TABLE
        f, r = bc.oracle(name)
        assert min(f["margin"], r["margin"]) > bc.MARGIN and f["transcript"] == r["transcript"], name
        assert f["stats"]["iterations"] == f["stats"]["trials"] == n_it, name


def scale_bars(name):
    return tuple(TOL["scale"][name]["bar"][k] for k in bc.KEYS)


@pytest.mark.parametrize("name", bc.NAMES + bc.SCALE_NAMES[:2])
def test_host_equals_oracle(built, name):
    """The host path is left out at scale_k512: its dense 3072 x 3072 factorisation is plain host code and the call took 47 s on the
    CPU this was written on, against the 10 s it was allowed; tests/test_ba_gpu.py holds the GPU call to the oracle there."""
    f = bc.oracle(name)[0]
    bars = scale_bars(name) if name in bc.SCALE_NAMES else BARS
    bc.assert_same(bc.host(built, name), f["Tcw"], f["xw"], f["stats"], bars, name, coordinates=name not in bc.GAUGE)


def test_robust_on_and_off_differ(built):
    """a tenth gross outliers: Huber (sqrt(5.99) / sqrt(7.815)) and no kernel end in different places, each where the oracle does"""
    a, b = bc.host(built, "k8_p64_robust"), bc.host(built, "k8_p64_plain")
    assert np.abs(a[1] - b[1]).max() > 1e-3 and np.abs(a[2] - b[2]).max() > 1e-3 and b[3]["chi2"] > 2 * a[3]["chi2"]
    # Huber's deltas are BundleAdjustment's, not LocalBundleAdjustment's: the first chi2 of a robust run tells sqrt(5.99) from
    # sqrt(5.991) on a monocular scene with outliers
    pr = bc.case("init_map_mono")[0]
    pr = dict(pr, obs=pr["obs"] + np.float32(9.0))
    _, _, _, st = built.BundleAdjustment(pr, 1, True)
    f = bc.bo.bundle_adjustment(pr, 1, True)
    assert abs(st["chi2"] - f["stats"]["chi2"]) <= 1e-12 * f["stats"]["chi2"], (st, f["stats"])
    import lba_oracle
    g = lba_oracle.Graph(pr, "forward")                                     # the same run with LocalBundleAdjustment's deltas
    s5991 = {"iterations": [0, 0], "trials": [0, 0], "lambda": 0.0, "chi2": 0.0}
    g.optimize(0, 1, s5991)
    assert abs(s5991["chi2"] - f["stats"]["chi2"]) > 1e-6 * f["stats"]["chi2"]


def test_one_round_and_no_more(built):
    """optimize(n_iterations) is all: no iteration beyond the budget, 0 optimises nothing, 1 runs one"""
    code, Tcw, xw, st = bc.host(built, "iterations_0")
    pr = bc.case("iterations_0")[0]
    assert code == 0 and st == {"iterations": 0, "trials": 0, "lambda": 0.0, "chi2": 0.0}
    assert xw.tobytes() == np.asarray(pr["xw"], np.float32).tobytes()
    assert np.abs(Tcw - roundtrip(pr["Tcw"])[:len(Tcw)]).max() <= 2.0 ** -24
    assert bc.host(built, "k9_p65_mixed")[3]["iterations"] == 1 and bc.host(built, bc.LARGEST)[3]["iterations"] == 10
    assert bc.host(built, "nbad_stops")[3]["iterations"] < 20               # the fork's _nBad stop


def test_vertices_without_edges(built):
    pr = bc.case("empty_vertices")[0]
    code, Tcw, xw, st = bc.host(built, "empty_vertices")
    k, pt = pr["empty_kf"], pr["empty_point"]
    assert xw[pt].tobytes() == pr["xw"][pt].tobytes()                      # vbNotIncludedMP: the bits
    assert np.abs(Tcw[k] - roundtrip(pr["Tcw"][k])[0]).max() <= 2.0 ** -24  # the round-tripped pose
    assert np.abs(xw[pt + 1] - pr["xw"][pt + 1]).max() > 1e-4 and np.abs(Tcw[0] - pr["Tcw"][0]).max() > 1e-4
    # the fixed key frame comes back as it went in
    kf = int(np.flatnonzero(pr["local_fixed"])[0])
    assert np.abs(Tcw[kf] - pr["Tcw"][kf]).max() <= 2.0 ** -22
    code, Tcw, xw, st = bc.host(built, "k1_p0")
    assert code == 0 and st["iterations"] == 0 and len(xw) == 0


def stopped_at(built, call, n, name):
    """call(problem, n_iterations, robust, stop) with the flag set just before read number n of `stop` (0: never) -> (result, reads)"""
    flag = np.zeros(1, np.uint8)
    reads = [0]

    def probe(_):
        reads[0] += 1
        if reads[0] == n:
            flag[0] = 1

    cb = PROBE(probe)
    built.lib().orbp_lba_set_stop_probe(C.cast(cb, C.c_void_p), None)
    try:
        pr, n_it, robust = bc.case(name)
        res = call(pr, n_it, robust, flag)
    finally:
        built.lib().orbp_lba_set_stop_probe(None, None)
    return res, reads[0]


def sweep_of(built, call, name):
    full, n_reads = stopped_at(built, call, 0, name)
    sweep = {0: full, "reads": n_reads}
    for n in range(1, n_reads + 2):
        sweep[n] = stopped_at(built, call, n, name)[0]
    return sweep


def check_sweep(sweep, name, what):
    """what every stop position must give, from the order of the reads alone: one at every iteration's top
    (sparse_optimizer.cpp:376) and one after every rejected trial that is not its iteration's tenth
    (optimization_algorithm_levenberg.cpp:149); none at entry and none after the loop"""
    pr = bc.case(name)[0]
    full, n_reads = sweep[0], sweep["reads"]
    it, tr = full[3]["iterations"], full[3]["trials"]
    assert n_reads == it + (tr - it), (what, full[3], n_reads)
    code, Tcw, xw, st = sweep[1]                                            # set before the first read: zero iterations, returns 0
    assert code == 0 and st["iterations"] == 0 and st["trials"] == 0, (what, st)
    assert xw.tobytes() == np.asarray(pr["xw"], np.float32).tobytes(), what
    assert np.abs(Tcw - roundtrip(pr["Tcw"])[:len(Tcw)]).max() <= 2.0 ** -24, what
    seen = set()
    for n in range(1, n_reads + 1):
        code, Tcw, xw, st = sweep[n]
        assert code == 0 and np.isfinite(Tcw).all() and np.isfinite(xw).all(), (what, n)
        assert st["iterations"] <= it and st["trials"] <= tr, (what, n, st)
        seen.add(st["iterations"])
        if n > 1:
            prev = sweep[n - 1][3]
            assert (prev["iterations"], prev["trials"]) <= (st["iterations"], st["trials"]), (what, n)
    assert set(range(it)) <= seen, (what, sorted(seen))                     # every iteration's top is a stop position
    last = sweep[n_reads + 1]                                               # a flag set after the last read changes nothing
    assert last[3] == full[3] and last[1].tobytes() == full[1].tobytes() and last[2].tobytes() == full[2].tobytes(), what


_SWEEP = {}


def host_sweep(built, name):
    if name not in _SWEEP:
        _SWEEP[name] = sweep_of(built, built.BundleAdjustment, name)
    return _SWEEP[name]


@pytest.mark.parametrize("name", ("k8_p64_robust", "rejecting"))
def test_the_host_path_reads_stop_where_g2o_does(built, name):
    sweep = host_sweep(built, name)
    check_sweep(sweep, name, "host " + name)
    assert sweep[0][3] == bc.host(built, name)[3]
    if name == "rejecting":                                                 # a rejected trial is followed by a read
        assert sweep["reads"] > sweep[0][3]["iterations"]


def test_stop_has_no_entry_check(built):
    """a flag that is set when the call begins still returns 0 with the round-tripped inputs (LocalBundleAdjustment returns
    ORBP_LBA_STOPPED and writes nothing); with n_iterations == 0 the flag is not even read"""
    pr, n_it, robust = bc.case("k8_p64_robust")
    stop = np.ones(1, np.uint8)
    code, Tcw, xw, st = built.BundleAdjustment(pr, n_it, robust, stop)
    assert code == 0 and st["iterations"] == 0 and xw.tobytes() == pr["xw"].tobytes()
    assert np.abs(Tcw - roundtrip(pr["Tcw"])).max() <= 2.0 ** -24 and (Tcw[:, 3, 3] == 1).all()
    _, reads = stopped_at(built, built.BundleAdjustment, 0, "iterations_0")
    assert reads == 0


def _call(built, pr, n_it=5, robust=1, mutate=None, null=None, T_null=False, x_null=False):
    Lb = built.lib()
    s, a = built.pack_lba_problem({k: np.array(v) for k, v in pr.items() if not k.startswith("empty")})
    if mutate:
        mutate(s, a)
    if null:
        setattr(s, null, None)
    T = np.full((len(pr["local_fixed"]), 16), 7.25, np.float32)
    x0 = a["xw"].copy()
    st = np.full(24, 0x5A, np.uint8)
    rc = Lb.orbp_bundle_adjustment(C.byref(s), n_it, robust, None if T_null else p(T), None if x_null else p(a["xw"]), None, p(st))
    assert rc == 0 or ((T == 7.25).all() and a["xw"].tobytes() == x0.tobytes() and (st == 0x5A).all())     # refused before any work
    return rc, Lb.orbp_last_error()


def test_invalid_arguments(built):
    Lb = built.lib()
    E_INV = built.ORBX_E_INVALID
    pr = bc.case("k8_p64_robust")[0]
    assert _call(built, pr)[0] == 0
    assert Lb.orbp_bundle_adjustment(None, 5, 1, None, None, None, None) == E_INV
    for field in ("local_fixed", "Tcw", "cam", "edge_off", "edge_kf", "obs", "u_right", "inv_sigma2"):
        rc, text = _call(built, pr, null=field)
        assert rc == E_INV and b"NULL" in text and text.startswith(b"bundle_adjustment:"), (field, text)
    for kw in ("T_null", "x_null"):
        assert _call(built, pr, **{kw: True})[0] == E_INV
    for field in ("n_local", "n_fixed", "n_points"):
        rc, text = _call(built, pr, mutate=lambda s, a, f=field: setattr(s, f, -1))
        assert rc == E_INV and b"negative" in text

    def kf_out(s, a):
        a["edge_kf"][5] = s.n_local + s.n_fixed
    assert _call(built, pr, mutate=kf_out)[0] == E_INV and b"outside" in Lb.orbp_last_error()

    def kf_neg(s, a):
        a["edge_kf"][0] = -1
    assert _call(built, pr, mutate=kf_neg)[0] == E_INV

    def kf_twice(s, a):
        a["edge_kf"][1] = a["edge_kf"][0]
    assert _call(built, pr, mutate=kf_twice)[0] == E_INV and b"twice" in Lb.orbp_last_error()

    def off0(s, a):
        a["edge_off"][0] = 1
    assert _call(built, pr, mutate=off0)[0] == E_INV and b"edge_off[0]" in Lb.orbp_last_error()

    def off_down(s, a):
        a["edge_off"][3] = a["edge_off"][2] - 1
    assert _call(built, pr, mutate=off_down)[0] == E_INV and b"not monotone at 2" in Lb.orbp_last_error()
    for bad in (np.nan, np.inf):
        for what, where, text in (("Tcw", (1, 7), b"pose of key frame 1"), ("cam", (2, 0), b"calibration of key frame 2"),
                                  ("xw", (4, 2), b"point 4 is not finite"), ("obs", (3, 1), b"observation of edge 3"),
                                  ("u_right", (3,), b"observation of edge 3"), ("inv_sigma2", (3,), b"observation of edge 3")):
            def poke(s, a, what=what, where=where, bad=bad):
                a[what][where] = bad
            rc, got = _call(built, pr, mutate=poke)
            assert rc == E_INV and text in got, (what, got)
    # n_iterations: 0 and the bound are legal, beyond it and below 0 are not
    top = built.ORBP_BA_MAX_ITERATIONS
    assert _call(built, pr, n_it=0)[0] == 0 and _call(built, pr, n_it=top)[0] == 0
    for n_it in (top + 1, -1, 1 << 30):
        rc, text = _call(built, pr, n_it=n_it)
        assert rc == E_INV and b"n_iterations" in text, (n_it, text)
    with pytest.raises(built.OrbxError):
        built.BundleAdjustment(dict(pr, obs=pr["obs"][:-1]))
    with pytest.raises(built.OrbxError):
        built.BundleAdjustment(pr, top + 1)


def big_counts(built, n_local, n_points):
    """a problem whose counts alone are large: no edges, and arrays only as long as the argument checks read"""
    s = built.LbaProblem()
    keep = {"local_fixed": np.zeros(n_local, np.uint8), "Tcw": np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n_local, 1)),
            "cam": np.ones((n_local, 5), np.float32), "edge_off": np.zeros(n_points + 1, np.int32),
            "xw": np.ones((n_points, 3), np.float32), "T_out": np.full((n_local, 16), 7.25, np.float32)}
    s.n_local, s.n_fixed, s.n_points = n_local, 0, n_points
    s.local_fixed, s.Tcw, s.cam, s.edge_off = (keep[k].ctypes.data for k in ("local_fixed", "Tcw", "cam", "edge_off"))
    return s, keep


def test_the_gpu_call_checks_arguments_and_capacity_before_any_device_work(built):
    """with a NULL handle (none can be made without a GPU): bad arguments get ORBX_E_INVALID and counts beyond the capacity
    ORBX_E_CAPACITY, both before the handle is looked at"""
    Lb = built.lib()
    pr = bc.case("k8_p64_robust")[0]
    s, a = built.pack_lba_problem({k: np.array(v) for k, v in pr.items()})
    T = np.full((s.n_local, 16), 7.25, np.float32)
    a["edge_off"][0] = 1
    assert Lb.orbm_bundle_adjustment(None, C.byref(s), 5, 1, p(T), p(a["xw"]), None, None) == built.ORBX_E_INVALID
    assert b"edge_off[0]" in Lb.orbm_last_error()
    a["edge_off"][0] = 0
    assert Lb.orbm_bundle_adjustment(None, C.byref(s), built.ORBP_BA_MAX_ITERATIONS + 1, 1, p(T), p(a["xw"]), None, None) == built.ORBX_E_INVALID
    assert Lb.orbm_bundle_adjustment(None, None, 5, 1, None, None, None, None) == built.ORBX_E_INVALID
    for n_local, n_points in ((built.ORBM_BA_MAX_KFS + 1, 0), (built.ORBM_BA_MAX_KFS, built.ORBM_BA_MAX_TABLE // built.ORBM_BA_MAX_KFS + 1)):
        s, keep = big_counts(built, n_local, n_points)
        rc = Lb.orbm_bundle_adjustment(None, C.byref(s), 10, 0, p(keep["T_out"]), p(keep["xw"]), None, None)
        assert rc == built.ORBX_E_CAPACITY and (keep["T_out"] == 7.25).all(), (n_local, n_points, Lb.orbm_last_error())
    x = np.zeros(6)
    ok = C.c_int(7)
    A = np.eye(6)
    assert Lb.orbm_spd_solve_f64(None, None, p(x), 6, p(x), C.byref(ok)) == built.ORBX_E_INVALID
    assert Lb.orbm_spd_solve_f64(None, p(A), p(x), 0, p(x), C.byref(ok)) == built.ORBX_E_INVALID
    assert Lb.orbm_spd_solve_f64(None, p(A), p(x), built.ORBM_SPD_MAX_N + 1, p(x), C.byref(ok)) == built.ORBX_E_CAPACITY and ok.value == 7


def test_the_gpu_call_fails_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    s, a = built.pack_lba_problem(bc.case("k8_p64_robust")[0])
    T = np.full((s.n_local, 16), 7.25, np.float32)
    x0 = a["xw"].copy()
    assert Lb.orbm_bundle_adjustment(None, C.byref(s), 5, 1, p(T), p(a["xw"]), None, None) == built.ORBX_E_HIP
    assert b"no CPU path" in Lb.orbm_last_error()
    assert (T == 7.25).all() and a["xw"].tobytes() == x0.tobytes()
