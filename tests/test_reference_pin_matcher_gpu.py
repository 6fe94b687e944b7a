"""The library's eleven ORBmatcher searches against the reference's own src/ORBmatcher.cc, with no step through the oracle: the
cases and fields of tests/test_reference_pin_matcher_cpu.py, through my_slam_amd.ORBmatcher and the C ABI calls that
tests/test_kf_matchers.py and tests/test_window_cases_gpu.py make (host projection helper -> PredictScale -> search on the GPU).
The host half is compared too: the reference's call log tells which MapPoints reached PredictScale and the level it returned; the
library's orbm_project_points*, orbm_sim3_decompose, orbm_sim3_relative and orbm_predict_scale must select the same points and
predict the same levels.  The answers come from oracle/_ref/ref_matcher where it travelled with the tree and from
tests/golden/matcher/ otherwise (cases the fixtures do not hold are then skipped); the reference checkout is never read."""
import numpy as np
import pytest

import oracle_lib as O
import ref_matcher as R

pytestmark = pytest.mark.gpu
F32, U8 = np.float32, np.uint8
CASES = R.all_cases()


def _kps(angle):
    k = np.zeros(len(angle), O.KP_DTYPE)
    k["angle"] = angle
    return k


def _gate(ok, usable, d3, mn, mx):
    return (np.asarray(usable).astype(bool) & ok.astype(bool) & ~(d3 < mn) & ~(d3 > mx)).astype(U8)


def lib_run(orbx, case):
    """the case's call on the library -> (outputs as R.run names them, {MapPoint: predicted level} of the points the host half let
    through, or None where the call has no projection step of its own)"""
    a, k = case.args, case.kind
    M = orbx.ORBmatcher
    mk = lambda nn, ori: M(nn, ori, max_queries=4096, max_train=4096, max_pairs=1 << 20)
    host = None
    if k == "proj_map":
        m = mk(a["nnratio"], True)
        m.grid_build(a["frame"][1], *a["frame"][2])
        obs = a["cur_obs"].copy()
        r, n = m.SearchByProjectionMap(a["in_view"], a["proj_x"], a["proj_y"], a["pred_level"], a["view_cos"], a["mp_desc"], a["mp_obs"], a["scale_factors"],
                                       a["frame"][1], a["desc_cur"], obs, a["th"], a.get("proj_xr"), a.get("u_right"))
        out = dict(match=r, n=n, cur_obs=obs)
    elif k == "proj_last":
        m = mk(0.9, a["check_ori"])
        m.grid_build(a["frame"][1], *a["frame"][2])
        obs = a["cur_obs"].copy()
        r, n = m.SearchByProjectionLast(a["has_point"], a["xw"], a["mp_desc"], a["mp_obs"], a["kps_last"], a["Tcw"], a["Tlw"], a["K"], a["mb"], a["mbf"],
                                        a["frame"][2], a["scale_factors"], a["frame"][1], a["desc_cur"], obs, a["th"], a["mono"], a.get("u_right"))
        out = dict(match=r, n=n, cur_obs=obs)
    elif k == "proj_kf":
        m = mk(0.9, a["check_ori"])
        m.grid_build(a["frame"][1], *a["frame"][2])
        u, v, iz, d3, ok = M.ProjectPoints(a["Tcw"], a["K"], a["frame"][2], a["xw"])
        use = _gate(ok, a["usable"], d3, a["min_inv"], a["max_inv"])
        lv = M.PredictScale(a["mf_max"], d3, a["log_sf"], len(a["scale_factors"]))
        has = a["cur_has"].copy()
        r, n = m.SearchByProjectionKF(use, u, v, lv, a["mp_desc"], a["kf_angle"], a["scale_factors"], a["frame"][1], a["desc_cur"], has, a["th"], a["orb_dist"])
        out, host = dict(match=r, n=n, cur_has=has), (use, lv)
    elif k in ("proj_sim3", "fuse_sim3", "fuse"):
        m = mk(0.75, True)
        m.grid_build_kf(a["kf"][1], a["kf"][2])
        if k == "fuse":
            T, Ow = a["Tcw"], a["Ow"]
        else:
            T, Ow = M.Sim3Decompose(a["Scw"])
        u, v, iz, d3, ok = M.ProjectPointsKF(T, a["K"], a["bounds"], a["xw"], a["normal"], Ow)
        use = _gate(ok, a["usable"], d3, a["min_inv"], a["max_inv"])
        lv = M.PredictScale(a["mf_max"], d3, a["log_sf"], len(a["scale_factors"]))
        host = (use, lv)
        if k == "proj_sim3":
            matched = a["kf_matched"].copy()
            r, n = m.SearchByProjectionSim3(use, u, v, lv, a["mp_desc"], a["scale_factors"], a["kf"][1], a["desc_kf"], matched, a["th"])
            out = dict(match=r, n=n, kf_matched=matched)
        elif k == "fuse_sim3":
            r, n = m.FuseSim3(use, u, v, lv, a["mp_desc"], a["scale_factors"], a["kf"][1], a["desc_kf"], a["th"])
            out = dict(best_idx=r, n=n)
        else:
            with np.errstate(invalid="ignore"):                                             # 0 * inf for a point the gates have dropped
                ur = (u - F32(a["bf"]) * iz).astype(F32)                                    # :870
            r, n = m.Fuse(use, u, v, ur, lv, a["mp_desc"], a["scale_factors"], a["inv_sigma2"], a["kf"][1], a["ur_kf"], a["desc_kf"], a["th"])
            out = dict(best_idx=r, n=n)
    elif k == "sim3":
        m = mk(0.75, True)
        s1, s2 = a["side1"], a["side2"]
        sR12, sR21, t21 = M.Sim3Relative(a["s12"], a["R12"], a["t12"])
        u1, v1, d1, ok1 = M.ProjectPointsSim3(s1["Tw"], sR21, t21, a["K"], s2["bounds"], s1["xw"])
        u2, v2, d2, ok2 = M.ProjectPointsSim3(s2["Tw"], sR12, a["t12"], a["K"], s1["bounds"], s2["xw"])
        use1 = _gate(ok1, s1["usable"], d1, s1["min_inv"], s1["max_inv"]); use2 = _gate(ok2, s2["usable"], d2, s2["min_inv"], s2["max_inv"])
        lv1 = M.PredictScale(s1["mf_max"], d1, s2["log_sf"], len(s2["sf"])); lv2 = M.PredictScale(s2["mf_max"], d2, s1["log_sf"], len(s1["sf"]))
        r, n = m.SearchBySim3(use1, u1, v1, lv1, s1["mp_desc"], use2, u2, v2, lv2, s2["mp_desc"], s1["kf"][1], s1["desc"], s1["kf"][2], s1["sf"],
                              s2["kf"][1], s2["desc"], s2["kf"][2], s2["sf"], a["th"])
        out = dict(match=r, n=n)
    elif k == "bow":
        m = mk(a["nnratio"], a["check_ori"])
        r, n = m.SearchByBoW(_kps(a["angle_kf"]), a["desc_kf"], a["fv_kf"], _kps(a["angle_f"]), a["desc_f"], a["fv_f"], a.get("valid_kf"))
        out = dict(match=r, n=n)
    elif k == "bow_kf":
        m = mk(a["nnratio"], a["check_ori"])
        r, n = m.SearchByBoWKF(_kps(a["angle1"]), a["desc1"], a["fv1"], a["valid1"], _kps(a["angle2"]), a["desc2"], a["fv2"], a["valid2"])
        out = dict(match=r, n=n)
    elif k == "init":
        m = mk(a["nnratio"], a["check_ori"])
        m.grid_build(a["frame"][1], *a["frame"][2])
        prev = a["prev"].copy()
        r, n = m.SearchForInitialization(a["kps1"], a["desc1"], a["frame"][1], a["desc2"], prev, a["window"])
        out = dict(match=r, n=n, prev=prev.view(np.uint32))
    elif k == "triang":
        m = mk(0.6, a["check_ori"])
        r, n = m.SearchForTriangulation(a["kps1"], a["desc1"], a["has_mp1"], a["ur1"], a["fv1"], a["kps2"], a["desc2"], a["has_mp2"], a["ur2"], a["fv2"],
                                        a["Cw"], a["T2w"], a["K2"], a["F12"], a["sf2"], a["sigma2_2"], a["only_stereo"])
        out = dict(match=r, n=n)
    else:
        raise KeyError(k)
    m.close()
    return out, host


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_library_equals_reference(orbx, case):
    want, rec = R.ask_case(case)
    got, host = lib_run(orbx, case)
    assert R.same(got, want), {f: (got[f], want[f]) for f in got if not np.array_equal(np.asarray(got[f]), np.asarray(want[f]))}
    for f, v in case.expect.items():
        assert np.array_equal(got[f], v), f
    if host is not None:
        # the host half against the reference's loop body: the points the library lets through are the points on which the
        # reference reached PredictScale, and the levels are the reference's
        use, lv = host
        levels = {int(mp): int(arg) for call, mp, arg in R.log(rec) if call == R.PREDICT_SCALE}
        assert sorted(levels) == [int(i) for i in np.nonzero(use)[0]]
        assert all(levels[i] == int(lv[i]) for i in levels)

