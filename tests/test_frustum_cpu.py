"""No-GPU checks of Frame::isInFrustum as the library restates it (include/orbm.h, orbm_frustum): the numpy oracle
tests/frustum_oracle.py on the suite's scenes (every status occurs, it agrees with a naive float64 computation away from the
gates), the reference's quirks on hand-made inputs, the ceil boundary of MapPoint::PredictScale, the correctly rounded logf
against the host's logf (orbm_predict_scale), the three exports, the argument checks made before any device work, and the loud
failure without a GPU."""
import ctypes as C

import numpy as np
import pytest

import frustum_oracle as F

f32, f64, ld = np.float32, np.float64, np.longdouble


def test_every_status_occurs_on_the_suite():
    seen = np.zeros(8, int)
    for k in range(len(F.SUITE)):
        sc = F.suite_scene(k)
        st = F.frustum(*sc.args(), 0.5)[0]
        seen += np.bincount(st, minlength=8)
    assert (seen >= 20).all(), dict(zip(F.STATUS_NAMES, seen))


def test_outputs_are_zero_unless_in_view_and_the_count_is_the_in_view_points():
    sc = F.suite_scene(0)
    st, px, py, pxr, lv, vc, n_to_match = F.frustum(*sc.args(), 0.5)
    out = st != F.IN_VIEW
    assert not (px[out].any() or py[out].any() or pxr[out].any() or lv[out].any() or vc[out].any())
    assert n_to_match == int((st == F.IN_VIEW).sum()) > 500
    assert (st[sc.skip != 0] == F.SKIPPED).all() and (st[sc.skip == 0] != F.SKIPPED).all()
    b = sc.view["bounds"]
    ok = ~out
    assert (px[ok] >= b[0]).all() and (px[ok] <= b[1]).all() and (py[ok] >= b[2]).all() and (py[ok] <= b[3]).all()
    assert (vc[ok] >= 0.5).all() and (lv[ok] >= 0).all() and (lv[ok] < 8).all() and (pxr[ok] < px[ok]).all()


@pytest.mark.parametrize("k", range(len(F.SUITE)))
def test_oracle_agrees_with_float64_away_from_the_gates(k):
    """points whose float64 margin to every gate exceeds 1e-4 (relative): same status, same level, values to float precision"""
    sc = F.suite_scene(k)
    st, px, py, pxr, lv, vc, _ = F.frustum(*sc.args(), 0.5)
    st64, u, v, ur, level, vc64, margin = F.frustum_f64(*sc.args(), 0.5)
    with np.errstate(invalid="ignore"):
        clear = margin > 1e-4                                           # nan (a degenerate point) compares false
    if sc.view["log_scale_factor"] != 0:                                # with 0 no level quotient is finite: only skipped points are clear
        assert clear.sum() > 0.5 * len(sc)
    assert np.array_equal(st[clear], st64[clear])
    ok = clear & (st == F.IN_VIEW)
    assert np.array_equal(lv[ok], level[ok].astype(np.int32))
    assert np.allclose(px[ok], u[ok], rtol=1e-5, atol=1e-2) and np.allclose(py[ok], v[ok], rtol=1e-5, atol=1e-2)
    assert np.allclose(pxr[ok], ur[ok], rtol=1e-5, atol=1e-2) and np.allclose(vc[ok], vc64[ok], rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", sorted(F.quirk_cases()))
def test_quirks_and_hand_made_inputs(name):
    sc, limit, want = F.quirk_cases()[name]
    st, px, py, pxr, lv, vc, n = F.frustum(*sc.args(), limit)
    assert list(st) == want
    if name == "base point is in view":
        assert px[0] == 345.0 and py[0] == 252.5 and pxr[0] == 335.0 and lv[0] == 2 and abs(vc[0] - 1) < 1e-6 and n == 1
    if name == "NaN u passes to the end":
        assert np.isnan(px[0]) and np.isnan(pxr[0]) and py[0] == 252.5
    if name == "NaN v passes :293":
        assert np.isnan(py[0]) and px[0] == 345.0
    if name == "NaN viewCos passes :310":
        assert np.isnan(vc[0]) and lv[0] == 2


def test_depth_zero_is_not_behind_but_a_negative_depth_is():
    tiny = np.nextafter(f32(0), f32(-1))
    sc = F._points(F._rig(), [[0.1, 0.05, 0.0], [0.1, 0.05, tiny]])
    assert list(F.frustum(*sc.args(), 0.5)[0]) == [F.OUT_X, F.BEHIND]


def test_ceil_boundary_of_predict_scale():
    """ratio = mvScaleFactors[k] exactly and its two float neighbours: log(ratio) / mfLogScaleFactor is k up to rounding, so the
    level is k or k + 1 there, at most k just below and at least k... k + 1 just above; never decreasing in the ratio."""
    for sc, k in F.ceil_boundary_scenes():
        st, _, _, _, lv, _, _ = F.frustum(*sc.args(), 0.5)
        nl = int(sc.view["nlevels"])
        assert (st == F.IN_VIEW).all()
        lo, at, hi = lv[0::3], lv[1::3], lv[2::3]
        kk = k[0::3]
        top = lambda a: np.minimum(a, nl - 1)
        assert ((at == kk) | (at == top(kk + 1))).all()
        assert ((lo == kk) | (lo == top(kk + 1)) | (lo == np.maximum(kk - 1, 0))).all() and (lo <= at).all()
        assert ((hi == top(kk + 1)) | (hi == kk)).all() and (hi >= at).all()
        assert (np.diff(lv) >= 0).all()
        assert lv[0] == 0 and lv[1] == 0 and lv[2] == min(1, nl - 1)    # log(1) = 0 exactly; just above 1 the quotient is positive


# ---- the library without a GPU

@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def count_level_differences(built):
    """-> (points compared, differences, differences outside the bound): the oracle's level (correctly rounded logf) against
    orbm_predict_scale (the host's logf) on every point of the suite and of the ceil-boundary inputs that reaches PredictScale
    with a defined result.  A difference is inside the bound when the quotient computed in long double lies within |q| * 2^-21
    of an integer: under 1 ulp of logf error (2^-23 relative, twice that in q after the division's own rounding, and the float
    quotient's half ulp) is less than |q| * 2^-21."""
    scenes = [F.suite_scene(k) for k in range(len(F.SUITE))] + [sc for sc, _ in F.ceil_boundary_scenes()]
    total = diff = outside = 0
    for sc in scenes:
        dist = F.distance(sc.view, sc.xw)
        logsf, nl = sc.view["log_scale_factor"], int(sc.view["nlevels"])
        level, undefined = F.predict_scale(sc.mf_max, dist, logsf, nl)
        with np.errstate(all="ignore"):
            ratio = sc.mf_max / dist
            use = ~undefined & np.isfinite(ratio) & (ratio > 0) & (logsf != 0)
            q = np.log(ratio.astype(ld)) / ld(logsf)
            near = np.abs(q - np.rint(q)) <= np.abs(q) * ld(2.0) ** -21
        host = built.ORBmatcher.PredictScale(sc.mf_max[use], dist[use], float(logsf), nl)
        d = host != level[use]
        total += int(use.sum()); diff += int(d.sum()); outside += int((d & ~near[use]).sum())
    return total, diff, outside


def test_correctly_rounded_logf_against_the_hosts_logf(built):
    total, diff, outside = count_level_differences(built)
    print("PredictScale: %d points, %d levels differ between the correctly rounded logf and the host's, %d outside the bound" % (total, diff, outside))
    assert total > 10000 and outside == 0


def test_the_three_symbols_are_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    assert hasattr(lib, "orbm_frustum") and hasattr(lib, "orbm_frustum_device") and hasattr(lib, "orbm_search_local_points")
    assert all(hasattr(built.ORBmatcher, a) for a in ("frustum", "frustum_device", "search_local_points"))
    assert built.VIEW_DTYPE == F.VIEW_DTYPE and built.KP_DTYPE == F.KP_DTYPE


def _args(built, n=40, seed=3):
    sc = F.make_scene(np.random.default_rng(seed), n)
    fr = F.make_frame(np.random.default_rng(seed), sc, n_clutter=30)
    m = len(fr.kps)
    return dict(view=np.array([sc.view]), skip=sc.skip, xw=sc.xw, normal=sc.normal, mf_max=sc.mf_max, mf_min=sc.mf_min, n=n,
                st=np.full(n, 77, np.uint8), px=np.full(n, 77, f32), py=np.full(n, 77, f32), pxr=np.full(n, 77, f32), lv=np.full(n, 77, np.int32),
                vc=np.full(n, 77, f32), nt=np.full(1, 77, np.int32), mp_desc=fr.mp_desc, mp_obs=fr.mp_obs, kps=fr.kps, desc=fr.desc, ur=fr.u_right,
                n_cur=m, cur_obs=fr.cur_obs.copy(), cm=np.full(m, 77, np.int32), nm=np.full(1, 77, np.int32))


INPUTS = ("view", "skip", "xw", "normal", "mf_max", "mf_min")
OUTPUTS = ("st", "px", "py", "pxr", "lv", "vc", "nt")


def _frustum(Lb, a, handle=None, n=None):
    return Lb.orbm_frustum(handle, p(a["view"]), a["n"] if n is None else n, *[p(a[k]) for k in INPUTS[1:]], C.c_float(0.5), *[p(a[k]) for k in OUTPUTS])


def _device(Lb, a, handle=None, n=None):
    return Lb.orbm_frustum_device(handle, p(a["view"]), a["n"] if n is None else n, *[p(a[k]) for k in INPUTS[1:]], C.c_float(0.5),
                                  *[p(a[k]) for k in OUTPUTS[:-1]], None)


def _local(Lb, a, handle=None, n=None, n_cur=None):
    return Lb.orbm_search_local_points(handle, p(a["view"]), a["n"] if n is None else n, *[p(a[k]) for k in INPUTS[1:]], C.c_float(0.5),
                                       p(a["mp_desc"]), p(a["mp_obs"]), p(a["kps"]), p(a["desc"]), p(a["ur"]), a["n_cur"] if n_cur is None else n_cur,
                                       C.c_float(3.0), C.c_float(0.8), *[p(a[k]) for k in OUTPUTS], p(a["cur_obs"]), p(a["cm"]), p(a["nm"]))


def _untouched(a):
    return all((a[k] == 77).all() for k in OUTPUTS + ("cm", "nm"))


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument still gets ORBX_E_INVALID and a text."""
    Lb = built.lib()
    E, OK = built.ORBX_E_INVALID, built.ORBX_OK
    a = _args(built)
    for call in (_frustum, _device, _local):
        assert call(Lb, a, n=-1) == E and b"n=-1" in Lb.orbm_last_error()
        assert call(Lb, a, n=0) == OK
    assert _local(Lb, a, n_cur=-1) == E and b"n_cur=-1" in Lb.orbm_last_error()
    none = dict.fromkeys(a)
    none["n"], none["n_cur"] = 0, 0
    assert _frustum(Lb, none) == OK and _device(Lb, none) == OK and _local(Lb, none) == OK       # n == 0 reads no pointer
    for key in INPUTS + OUTPUTS:
        b = dict(a)
        b[key] = None
        assert _frustum(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key
        assert _local(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key
        if key != "nt":
            assert _device(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key
    for key in ("mp_desc", "mp_obs", "kps", "desc", "cur_obs", "cm", "nm"):
        b = dict(a)
        b[key] = None
        assert _local(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key
    for nlevels in (0, -1, 17):
        b = _args(built)
        b["view"]["nlevels"] = nlevels
        for call in (_frustum, _local):
            assert call(Lb, b) == E and b"nlevels=%d" % nlevels in Lb.orbm_last_error()
            assert _untouched(b)
    b = _args(built)
    b["view"]["mbf"] = 0.0                                              # a monocular frame cannot gate on mvuRight
    assert _local(Lb, b) == E and b"mbf" in Lb.orbm_last_error() and _untouched(b)
    b["ur"] = None
    assert _local(Lb, b) != E or b"mbf" not in Lb.orbm_last_error()
    assert _untouched(a)


def test_the_entry_points_fail_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    a = _args(built)
    for call in (_frustum, _device, _local):
        assert call(Lb, a) == built.ORBX_E_HIP
        assert b"no CPU path" in Lb.orbm_last_error()
        assert _untouched(a)                                            # no half answer
    with pytest.raises(built.OrbxError) as ei:
        built.ORBmatcher()
    assert ei.value.code == built.ORBX_E_HIP
