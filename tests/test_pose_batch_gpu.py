"""orbm_pose_optimization_batch / orbm_pose_optimization_batch_device (include/orbm.h) on the GPU against the host path
orbp_pose_optimization on the cases of tests/pose_cases.py, at the bar tests/test_pose.py sets for this function: |dTcw| <= 2e-6 per
entry (the output is fp32), outlier flags identical, n_good identical.  Only the order of the sums over the edges differs between
the two sides, so a flag can flip only for an edge whose fp64 chi2 lies within rounding of its threshold; assert_same shows that
chi2 should a seed ever do it."""
import ctypes as C

import numpy as np
import pytest

import frustum_oracle as F
import oracle_lib as O
import pose_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


def against_host(orbx, got, name, what=""):
    want = pc.host(orbx, name)
    assert len(got) == len(want)
    for k, (g, w, pr) in enumerate(zip(got, want, pc.cases()[name])):
        pc.assert_same(g, w, pr, "%s %s[%d] n=%d" % (what, name, k, len(pr[0])))
        if len(pr[0]) < 3:                                  # the pose stays as it came, bit for bit
            assert g[2] == 0 and not g[1].any() and np.array_equal(g[0].view(np.uint32), np.asarray(pr[7], np.float32).view(np.uint32))


def same_bytes(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b))


@pytest.mark.parametrize("n", pc.SINGLE_SIZES)
def test_single_problems_equal_the_host(m, orbx, n):
    """the untouched pose below 3, the one-round rule below 10, the wave and workgroup edges, several edges per thread"""
    name = "single_%d" % n
    got = [m.pose_optimization_batch([pr])[0] for pr in pc.cases()[name]]
    against_host(orbx, got, name)


def raw_batch(m, orbx, problems, guard=32):
    """the C call on packed arrays with a guard pattern around the flags -> (results, out array, off)"""
    off, obs, ur, s2, xw, cams, T = orbx.ORBmatcher.pack_pose_problems(problems)
    N, B = int(off[-1]), len(problems)
    out = np.full(N + 2 * guard, 0xA5, np.uint8)
    good = np.full(B + 2, -77, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = m.L.orbm_pose_optimization_batch(m.h, B, p(off), p(obs), p(ur), p(s2), p(xw), p(cams), p(T), C.c_void_p(out.ctypes.data + guard), p(good))
    assert rc == orbx.ORBX_OK, m.L.orbm_last_error()
    assert (out[:guard] == 0xA5).all() and (out[N + guard:] == 0xA5).all() and (good[B:] == -77).all()
    flags = out[guard:N + guard]
    assert ((flags == 0) | (flags == 1)).all()
    return [(T[k].reshape(4, 4).copy(), flags[off[k]:off[k + 1]].astype(bool), int(good[k])) for k in range(B)]


def test_mixed_batch_equals_the_host_problem_by_problem(m, orbx):
    """13 problems of sizes 0 .. 1500 in one launch: mono and stereo-mixed, three cameras, two values of bf; the flags outside the
    problems' ranges keep the guard pattern"""
    got = raw_batch(m, orbx, pc.cases()["mixed"])
    against_host(orbx, got, "mixed")
    assert same_bytes(got, m.pose_optimization_batch(pc.cases()["mixed"]))


def test_all_outliers_and_the_fixed_point(m, orbx):
    got = m.pose_optimization_batch(pc.cases()["all_outliers"])
    against_host(orbx, got, "all_outliers")
    assert got[0][2] == 0 and got[0][1].all()
    got = m.pose_optimization_batch(pc.cases()["fixed_point"])
    against_host(orbx, got, "fixed_point")
    pr = pc.cases()["fixed_point"][0]
    assert got[0][2] == 100 and not got[0][1].any() and np.abs(got[0][0] - pr[7]).max() < 1e-5


def test_large_rotations_equal_the_host(m, orbx):
    """rotations of 2.2, 2.9 and 3.1 rad about x, y and z: the three branches of Quaterniond(Matrix3d) below a positive trace"""
    against_host(orbx, m.pose_optimization_batch(pc.cases()["large_rotation"]), "large_rotation")


def test_a_result_depends_on_its_problem_alone(m):
    """the batch is byte-equal to B single-problem calls, to a second run and to the same problems in reversed order"""
    problems = pc.cases()["mixed"]
    batch = m.pose_optimization_batch(problems)
    singles = [m.pose_optimization_batch([pr])[0] for pr in problems]
    assert same_bytes(batch, singles)
    assert same_bytes(batch, m.pose_optimization_batch(problems))
    assert same_bytes(batch, m.pose_optimization_batch(problems[::-1])[::-1])


def test_device_pointer_form_gives_the_same_bytes(m, orbx):
    import torch
    problems = pc.cases()["mixed"]
    want = m.pose_optimization_batch(problems)
    off, obs, ur, s2, xw, cams, T = orbx.ORBmatcher.pack_pose_problems(problems)
    B, N = len(problems), int(off[-1])
    dev = torch.device("cuda")
    cams_f = np.ascontiguousarray(cams.view(np.float32).reshape(B, 5))
    host_in = [off, obs, ur, s2, xw, cams_f]
    d_in = [torch.from_numpy(a).to(dev) for a in host_in]
    d_T = torch.from_numpy(T.copy()).to(dev)
    d_out = torch.full((N + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d_good = torch.full((B,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    m.pose_optimization_batch_device(B, *d_in, d_T, d_out[32:32 + N], d_good, stream=stream)
    stream.synchronize()
    Tg, og, gg = d_T.cpu().numpy(), d_out.cpu().numpy(), d_good.cpu().numpy()
    got = [(Tg[k].reshape(4, 4), og[32 + off[k]:32 + off[k + 1]].astype(bool), int(gg[k])) for k in range(B)]
    assert same_bytes(got, want)
    assert (og[:32] == 0xA5).all() and (og[32 + N:] == 0xA5).all()
    for d, h in zip(d_in, host_in):                         # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), h)
    m.pose_optimization_batch_device(0, *([None] * 9))      # n_problems == 0: nothing is read
    with pytest.raises(orbx.OrbxError) as e:
        m.pose_optimization_batch_device(B, *d_in[:5], None, d_T, d_out[32:32 + N], d_good)
    assert e.value.code == orbx.ORBX_E_INVALID


def test_a_small_handle_grows(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        big, small = pc.cases()["single_1500"], pc.cases()["single_63"]
        got_big = h.pose_optimization_batch(big)            # 9000 observations: the handle grows
        got_small = h.pose_optimization_batch(small)
        against_host(orbx, got_big, "single_1500", "grown handle")
        against_host(orbx, got_small, "single_63", "grown handle")
        assert same_bytes(got_big, h.pose_optimization_batch(big))
    finally:
        h.close()


def test_the_handle_keeps_its_grid_and_its_neighbours_results(m, orbx):
    """in the manner of tests/test_frustum_gpu.py: a grid query and a frustum call before and after a batch"""
    sc = F.suite_scene(0)
    fr = F.make_frame(np.random.default_rng(31), sc)
    bounds = tuple(float(b) for b in sc.view["bounds"])
    m.grid_build(fr.kps, *bounds)
    og = O.FrameGrid(fr.kps, *bounds)
    rng = np.random.default_rng(5)
    qx, qy = rng.uniform(0, bounds[1], 200).astype(np.float32), rng.uniform(0, bounds[3], 200).astype(np.float32)

    def neighbours():
        off, idx = m.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        for q in (0, 17, 199):
            assert np.array_equal(idx[off[q]:off[q + 1]], og.features_in_area(float(qx[q]), float(qy[q]), 25.0, 0, 3))
        return (off, idx) + tuple(m.frustum(*sc.args(), 0.5))

    before = neighbours()
    want_fr = F.frustum(*sc.args(), 0.5)
    assert np.array_equal(before[2], want_fr[0]) and before[8] == want_fr[6]
    against_host(orbx, m.pose_optimization_batch(pc.cases()["mixed"]), "mixed")
    assert m.grid_count() == len(fr.kps)
    after = neighbours()
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    against_host(orbx, m.pose_optimization_batch(pc.cases()["single_257"]), "single_257")
    assert m.grid_count() == len(fr.kps)
