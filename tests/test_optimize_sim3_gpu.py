"""orbm_optimize_sim3_batch / orbm_optimize_sim3_batch_device (include/orbm.h) on the GPU against the host path orbp_optimize_sim3
on the cases of tests/optimize_sim3_cases.py: flags identical, nIn identical, S12 within the bar of
tests/golden/sim3opt/tolerance.json (4 x the spread of the oracle's two summation orders, measured by
tests/tools/measure_sim3opt_spread.py).  Host and kernel run one text (csrc/orbp_sim3opt_body.h); the order of the sums over the
pairs and the device's sin / cos / exp are what differs.  The cases keep every chi2 away from th2 in the oracle, so a flag cannot
flip for rounding."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import frustum_oracle as F
import oracle_lib as O
import optimize_sim3_cases as sc

pytestmark = pytest.mark.gpu

TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3opt", "tolerance.json")))
BARS = tuple(TOL["bar"][k] for k in ("quaternion", "translation", "scale"))


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


def against_host(orbx, got, name, what=""):
    want = sc.host(orbx, name)
    assert len(got) == len(want)
    for k, (g, w, pr) in enumerate(zip(got, want, sc.cases()[name])):
        sc.assert_same(g, w, BARS, "%s %s[%d] n=%d" % (what, name, k, len(pr[0])))
        start = np.asarray(pr[10], np.float64).tobytes()
        if w[0].tobytes() == start:                         # fewer than 10 pairs left: S12 stays as it came, bit for bit
            assert w[2] == 0 and g[0].tobytes() == start


def same_bytes(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b))


@pytest.mark.parametrize("n", sc.SINGLE_SIZES)
def test_single_problems_equal_the_host(m, orbx, n):
    """the early return below 10, the wave and workgroup edges, several pairs per thread; with outliers the second optimize() runs
    10 iterations"""
    name = "single_%d" % n
    got = [m.optimize_sim3_batch([pr])[0] for pr in sc.cases()[name]]
    against_host(orbx, got, name)


def raw_batch(m, orbx, problems, guard=32):
    """the C call on packed arrays with a guard pattern around flags and n_in"""
    off, x1, x2, o1, o2, s1, s2, cams, th2, fix, S = orbx.ORBmatcher.pack_sim3opt_problems(problems)
    N, B = int(off[-1]), len(problems)
    out = np.full(N + 2 * guard, 0xA5, np.uint8)
    n_in = np.full(B + 2 * guard, -77, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = m.L.orbm_optimize_sim3_batch(m.h, B, p(off), p(x1), p(x2), p(o1), p(o2), p(s1), p(s2), p(cams), p(th2), p(fix), p(S),
                                      C.c_void_p(out.ctypes.data + guard), C.c_void_p(n_in.ctypes.data + 4 * guard))
    assert rc == orbx.ORBX_OK, m.L.orbm_last_error()
    assert (out[:guard] == 0xA5).all() and (out[N + guard:] == 0xA5).all()
    assert (n_in[:guard] == -77).all() and (n_in[B + guard:] == -77).all()
    flags = out[guard:N + guard]
    assert ((flags == 0) | (flags == 1)).all()
    return [(S[k].copy(), flags[off[k]:off[k + 1]].astype(bool), int(n_in[guard + k])) for k in range(B)]


def test_mixed_batch_equals_the_host_problem_by_problem(m, orbx):
    """13 problems of 0 .. 600 pairs in one launch: two cameras, both fix_scale values, th2 10 and 5.991; the bytes around flags and
    n_in keep the guard pattern"""
    got = raw_batch(m, orbx, sc.cases()["mixed"])
    against_host(orbx, got, "mixed")
    assert same_bytes(got, m.optimize_sim3_batch(sc.cases()["mixed"]))


def test_too_few_left_and_the_fixed_point(m, orbx):
    got = m.optimize_sim3_batch(sc.cases()["too_few_left"])
    against_host(orbx, got, "too_few_left")
    pr = sc.cases()["too_few_left"][0]
    assert got[0][2] == 0 and got[0][1][:6].all() and got[0][0].tobytes() == pr[10].tobytes()
    got = m.optimize_sim3_batch(sc.cases()["fixed_point"])
    against_host(orbx, got, "fixed_point")
    pr = sc.cases()["fixed_point"][0]
    assert got[0][2] == 100 and not got[0][1].any() and max(sc.diff3(got[0][0], pr[10])) < 1e-5


def test_a_result_depends_on_its_problem_alone(m):
    """the batch is byte-equal to B single-problem calls, to a second run and to the same problems in reversed order"""
    problems = sc.cases()["mixed"]
    batch = m.optimize_sim3_batch(problems)
    singles = [m.optimize_sim3_batch([pr])[0] for pr in problems]
    assert same_bytes(batch, singles)
    assert same_bytes(batch, m.optimize_sim3_batch(problems))
    assert same_bytes(batch, m.optimize_sim3_batch(problems[::-1])[::-1])


def test_device_pointer_form_gives_the_same_bytes(m, orbx):
    import torch
    problems = sc.cases()["mixed"]
    want = m.optimize_sim3_batch(problems)
    packed = orbx.ORBmatcher.pack_sim3opt_problems(problems)
    off, S = packed[0], packed[10]
    B, N = len(problems), int(off[-1])
    dev = torch.device("cuda")
    host_in = list(packed[:10])
    d_in = [torch.from_numpy(a).to(dev) for a in host_in]
    d_S = torch.from_numpy(S.copy()).to(dev)
    d_out = torch.full((N + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d_nin = torch.full((B + 16,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    m.optimize_sim3_batch_device(B, *d_in, d_S, d_out[32:32 + N], d_nin[8:8 + B], stream=stream)
    stream.synchronize()
    Sg, og, ng = d_S.cpu().numpy(), d_out.cpu().numpy(), d_nin.cpu().numpy()
    got = [(Sg[k], og[32 + off[k]:32 + off[k + 1]].astype(bool), int(ng[8 + k])) for k in range(B)]
    assert same_bytes(got, want)
    assert (og[:32] == 0xA5).all() and (og[32 + N:] == 0xA5).all()
    assert (ng[:8] == -77).all() and (ng[8 + B:] == -77).all()
    for d, h in zip(d_in, host_in):                         # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), h)
    m.optimize_sim3_batch_device(0, *([None] * 13))         # n_problems == 0: nothing is read
    with pytest.raises(orbx.OrbxError) as e:
        m.optimize_sim3_batch_device(B, *d_in[:9], None, d_S, d_out[32:32 + N], d_nin[8:8 + B])
    assert e.value.code == orbx.ORBX_E_INVALID


def test_a_small_handle_grows(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        big, small = sc.cases()["single_600"], sc.cases()["single_63"]
        got_big = h.optimize_sim3_batch(big)                # 4800 pairs: the handle grows
        got_small = h.optimize_sim3_batch(small)
        against_host(orbx, got_big, "single_600", "grown handle")
        against_host(orbx, got_small, "single_63", "grown handle")
        assert same_bytes(got_big, h.optimize_sim3_batch(big))
    finally:
        h.close()


def test_the_handle_keeps_its_grid_and_its_neighbours_results(m, orbx):
    """in the manner of tests/test_pose_batch_gpu.py: a grid query and a frustum call before and after a batch"""
    scn = F.suite_scene(0)
    fr = F.make_frame(np.random.default_rng(31), scn)
    bounds = tuple(float(b) for b in scn.view["bounds"])
    m.grid_build(fr.kps, *bounds)
    og = O.FrameGrid(fr.kps, *bounds)
    rng = np.random.default_rng(5)
    qx, qy = rng.uniform(0, bounds[1], 200).astype(np.float32), rng.uniform(0, bounds[3], 200).astype(np.float32)

    def neighbours():
        off, idx = m.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        for q in (0, 17, 199):
            assert np.array_equal(idx[off[q]:off[q + 1]], og.features_in_area(float(qx[q]), float(qy[q]), 25.0, 0, 3))
        return (off, idx) + tuple(m.frustum(*scn.args(), 0.5))

    before = neighbours()
    want_fr = F.frustum(*scn.args(), 0.5)
    assert np.array_equal(before[2], want_fr[0]) and before[8] == want_fr[6]
    against_host(orbx, m.optimize_sim3_batch(sc.cases()["mixed"]), "mixed")
    assert m.grid_count() == len(fr.kps)
    after = neighbours()
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    against_host(orbx, m.optimize_sim3_batch(sc.cases()["single_257"]), "single_257")
    assert m.grid_count() == len(fr.kps)
