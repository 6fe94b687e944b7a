"""The windowed ORBmatcher searches on the planted fixtures of tests/window_cases.py: the C ABI through the Python bindings equals
the oracle, bit for bit, on every output array and every count.  tests/test_window_cases_cpu.py pins the oracle's answers on the
same fixtures to the reference's lines.
Part 1: k_search_kf (csrc/orbm_kf.hip) behind orbm_fuse, orbm_fuse_sim3 and both directions of orbm_search_by_sim3, on three
key-frame grids.  Part 2: the five searches whose scan runs on the host over the lists of k_area_list and the CSR distances."""
import numpy as np
import pytest

import oracle_lib as O
import window_cases as WC

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", params=WC.KF_GRIDS)
def kf(request):
    return WC.kf_case(request.param)


def _matcher(orbx, nnratio=0.6, ori=True):
    return orbx.ORBmatcher(nnratio, ori, max_queries=64, max_train=256, max_pairs=4096)


def _named(fx, got, want):
    return {n: (int(g), int(w)) for n, g, w in zip(fx["names"], got, want) if g != w}


def test_fuse_planted(orbx, kf):
    """orbm_fuse: ties, octave window, TH_LOW, window edges, degenerate windows and the chi-square gate at its float boundaries;
    then with 1, 4 and 5 usable queries."""
    fx = kf
    m = _matcher(orbx)
    m.grid_build_kf(fx["kps"], fx["grid"])
    ur = (fx["u"] - F32(fx["bf"])).astype(F32)
    for use in [fx["use"]] + [WC.kf_subset(fx, k) for k in (1, 4, 5)]:
        bi, nf = m.Fuse(use, fx["u"], fx["v"], ur, fx["lv"], fx["qdesc"], fx["sf"], fx["inv_sigma2"], fx["kps"], fx["ur_kf"], fx["desc"], fx["th"])
        obi, onf = WC.oracle_fuse(fx, use)
        assert np.array_equal(bi, obi), _named(fx, bi, obi)
        assert nf == onf
    m.close()


def test_fuse_sim3_planted(orbx, kf):
    fx = kf
    m = _matcher(orbx)
    m.grid_build_kf(fx["kps"], fx["grid"])
    for use in [fx["use"]] + [WC.kf_subset(fx, k) for k in (1, 4, 5)]:
        bi, nf = m.FuseSim3(use, fx["u"], fx["v"], fx["lv"], fx["qdesc"], fx["sf"], fx["kps"], fx["desc"], fx["th"])
        obi, onf = WC.oracle_fuse_sim3(fx, use)
        assert np.array_equal(bi, obi), _named(fx, bi, obi)
        assert nf == onf
    m.close()


@pytest.mark.parametrize("big_first,n_small", [(False, None), (True, None), (False, 5)])
def test_search_by_sim3_planted(orbx, kf, big_first, n_small):
    """orbm_search_by_sim3 with the planted searches as its 1 -> 2 direction (the big frame is key frame 2), as its 2 -> 1 direction
    (roles swapped: the second result block, at an offset that depends on nq1), and with n1 = 5.  TH_HIGH, the agreement check,
    and the grid that the call leaves in the handle."""
    fx = kf
    s1, s2 = WC.sim3_sides(fx, big_first, n_small)
    m = _matcher(orbx)
    m12, nf = m.SearchBySim3(s1["usable"], s1["u"], s1["v"], s1["lv"], s1["mp_desc"], s2["usable"], s2["u"], s2["v"], s2["lv"], s2["mp_desc"],
                             s1["kps"], s1["desc"], s1["grid_t"], fx["sf"], s2["kps"], s2["desc"], s2["grid_t"], fx["sf"], fx["th"])
    om12, onf = WC.oracle_sim3(fx, big_first, n_small)
    assert np.array_equal(m12, om12), {i: (int(g), int(w)) for i, (g, w) in enumerate(zip(m12, om12)) if g != w}
    assert nf == onf and nf >= (4 if n_small else 20)
    assert m.grid_count() == len(s1["kps"])
    m.close()


def test_search_by_projection_sim3_planted(orbx):
    fx = WC.sim3proj_case()
    m = _matcher(orbx)
    m.grid_build_kf(fx["kps"], fx["grid"])
    matched = fx["matched"].copy()
    km, nm = m.SearchByProjectionSim3(fx["use"], fx["u"], fx["v"], fx["lv"], fx["qdesc"], WC.SF, fx["kps"], fx["desc"], matched, fx["th"])
    okm, onm, omatched = WC.oracle_sim3proj(fx)
    assert np.array_equal(km, okm) and nm == onm and np.array_equal(matched, omatched)
    m.close()


@pytest.mark.parametrize("ori", [True, False])
def test_search_for_initialization_planted(orbx, ori):
    fx = WC.init_case()
    m = _matcher(orbx, fx["nnratio"], ori)
    m.grid_build(fx["kps"], *WC.FRAME_BOUNDS)
    prev = fx["prev"].copy()
    m12, nm = m.SearchForInitialization(fx["kps1"], fx["qdesc"], fx["kps"], fx["desc"], prev, fx["window"])
    om12, onm, oprev = WC.oracle_init(fx, ori)
    assert np.array_equal(m12, om12) and nm == onm
    assert np.array_equal(prev.view(np.uint32), oprev.view(np.uint32))
    m.close()


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("mode", list(WC.LAST_MODES))
def test_search_by_projection_last_planted(orbx, mode, ori):
    fx = WC.last_case()
    m = _matcher(orbx, 0.9, ori)
    m.grid_build(fx["kps"], *WC.FRAME_BOUNDS)
    xw, Tcw, Tlw = WC.last_pose(fx, mode)
    cur_obs = fx["cur_obs"].copy()
    cm, nm = m.SearchByProjectionLast(fx["has"], xw, fx["qdesc"], fx["mp_obs"], fx["kps_last"], Tcw, Tlw, WC.KID, fx["mb"], fx["mbf"], WC.WIDE, WC.SF,
                                      fx["kps"], fx["desc"], cur_obs, fx["th"], False, fx["u_right"])
    ocm, onm, ocur = WC.oracle_last(fx, mode, ori)
    assert np.array_equal(cm, ocm) and nm == onm and np.array_equal(cur_obs, ocur)
    m.close()


def test_search_by_projection_map_planted(orbx):
    fx = WC.map_case()
    m = _matcher(orbx, fx["nnratio"])
    m.grid_build(fx["kps"], *WC.FRAME_BOUNDS)
    cur_obs = fx["cur_obs"].copy()
    cm, nm = m.SearchByProjectionMap(fx["in_view"], fx["px"], fx["py"], fx["lv"], fx["vc"], fx["qdesc"], fx["mp_obs"], WC.SF, fx["kps"], fx["desc"],
                                     cur_obs, fx["th"], fx["pxr"], fx["u_right"])
    ocm, onm, ocur = WC.oracle_map(fx)
    assert np.array_equal(cm, ocm) and nm == onm and np.array_equal(cur_obs, ocur)
    m.close()


@pytest.mark.parametrize("ori", [True, False])
def test_search_by_projection_kf_planted(orbx, ori):
    fx = WC.kfproj_case()
    m = _matcher(orbx, 0.9, ori)
    m.grid_build(fx["kps"], *WC.FRAME_BOUNDS)
    has = fx["has"].copy()
    cm, nm = m.SearchByProjectionKF(fx["use"], fx["u"], fx["v"], fx["lv"], fx["qdesc"], fx["kf_angle"], WC.SF, fx["kps"], fx["desc"], has,
                                    fx["th"], fx["orb_dist"])
    ocm, onm, ohas = WC.oracle_kfproj(fx, ori)
    assert np.array_equal(cm, ocm) and nm == onm and np.array_equal(has, ohas)
    m.close()
