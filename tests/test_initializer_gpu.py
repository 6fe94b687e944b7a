"""orbm_init_hypotheses / orbm_init_check_rt and their _device forms (include/orbm.h) on the GPU against the host path
orbp_init_hypothesis / orbp_init_check_rt_matches on the cases of tests/initializer_cases.py: host and kernels run one body
(csrc/orbp_init_body.h), so scores, matrices, counts, masks, verdicts, cosines and points are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import frustum_oracle as F
import initializer_cases as ic

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5
PAD = 16


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def solver(orbx, case, iterations=ic.ITERATIONS):
    s = orbx.Initializer(case["keys1"], ic.K, ic.SIGMA, iterations, rand=ic.Lcg(case["seed"]), rand_max=ic.RAND_MAX)
    s.set_current(case["keys2"], case["matches12"])
    return s


def problem(orbx, case, k):
    """the case as a problem of k iterations: the H of its first k sets, then their F"""
    s = solver(orbx, case, k)
    s.draw()
    return s.problem()


_HOST = {}


def host(orbx, name):
    """orbp_init_hypothesis on every set of the case and both models, once: (score_M, counts, masks), the H block first"""
    if name not in _HOST:
        case = ic.BY_NAME[name]
        s = solver(orbx, case)
        _HOST[name] = s.hypotheses(np.concatenate([case["sets"], case["sets"]]), [0] * ic.ITERATIONS + [1] * ic.ITERATIONS)
    return _HOST[name]


def host_k(orbx, name, k):
    rows = np.r_[0:k, ic.ITERATIONS:ic.ITERATIONS + k]
    return tuple(a[rows] for a in host(orbx, name))


def run(orbx, m, problems):
    """orbm_init_hypotheses with guard words around the three outputs -> [(score_M, counts, masks)] per problem"""
    off, uv, pn, params, hyp_off, sets, models, mask_off = orbx.ORBmatcher.pack_init_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    sm = np.full(10 * H + 2 * PAD, GUARD, np.uint32)
    cnt = np.full(H + 2 * PAD, GUARD, np.uint32)
    masks = np.full(MW + 2 * PAD, GUARD, np.uint32)
    rc = m.L.orbm_init_hypotheses(m.h, B, p(off), p(uv), p(pn), p(params), p(hyp_off), p(sets), p(models), p(mask_off), p(sm[PAD:]),
                                  p(cnt[PAD:]), p(masks[PAD:]))
    assert rc == orbx.ORBX_OK, m.L.orbm_last_error()
    for a, n in ((sm, 10 * H), (cnt, H), (masks, MW)):
        assert (a[:PAD] == GUARD).all() and (a[PAD + n:] == GUARD).all()
    out = []
    for k in range(B):
        h0, h1, n = int(hyp_off[k]), int(hyp_off[k + 1]), int(off[k + 1] - off[k])
        W = (n + 31) // 32
        c = cnt[PAD + h0:PAD + h1].view(np.int32).copy()
        mk = masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].reshape(h1 - h0, W).copy()
        bits = np.unpackbits(mk.view(np.uint8).reshape(h1 - h0, 4 * W), axis=1, bitorder="little")
        assert not bits[:, n:].any()                                            # bits >= n are zero
        assert np.array_equal(bits.sum(1), c)                                   # the count is the mask's popcount
        out.append((sm[PAD + 10 * h0:PAD + 10 * h1].view(np.float32).reshape(h1 - h0, 10).copy(), c, mk))
    return out


def same(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


def against_host(orbx, got, name, k, what=""):
    for g, w, field in zip(got, host_k(orbx, name, k), ("score_M", "n_inliers", "masks")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s %s k=%d: %s differs from the host path" % (what, name, k, field)


@pytest.mark.parametrize("name", [c["name"] for c in ic.CASES])
def test_single_problems_equal_the_host_byte_for_byte(m, orbx, name):
    case = ic.BY_NAME[name]
    for k in ic.HYP_COUNTS:
        got = run(orbx, m, [problem(orbx, case, k)])
        against_host(orbx, got[0], name, k, "single")
    sm = got[0][0]
    assert (sm[:, 0] >= 0).all() and (sm[:, 0] > 0).sum() >= ic.ITERATIONS // 2  # real scores, not a row of zeros


def mixed(orbx):
    return [problem(orbx, ic.BY_NAME[name], k) for name, k in ic.MIXED]


def test_mixed_batch_equals_the_host_problem_by_problem(m, orbx):
    got = run(orbx, m, mixed(orbx))
    for g, (name, k) in zip(got, ic.MIXED):
        against_host(orbx, g, name, k, "mixed")


def test_a_result_depends_on_its_problem_set_and_model_alone(m, orbx):
    problems = mixed(orbx)
    batch = run(orbx, m, problems)
    for g, pr in zip(batch, problems):
        assert same(g, run(orbx, m, [pr])[0])                                    # the batch equals the single-problem calls
    assert all(same(a, b) for a, b in zip(batch, run(orbx, m, problems)))         # a second run
    assert all(same(a, b) for a, b in zip(batch, run(orbx, m, problems[::-1])[::-1]))
    assert all(same(a, b) for a, b in zip(batch, m.init_hypotheses(problems)))    # the unguarded wrapper


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_pointer_form_gives_the_same_bytes(m, orbx, own_stream):
    import torch
    problems = mixed(orbx)
    want = run(orbx, m, problems)
    off, uv, pn, params, hyp_off, sets, models, mask_off = orbx.ORBmatcher.pack_init_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    dev = torch.device("cuda")
    host_in = [off, uv, pn, np.ascontiguousarray(params.view(np.uint8).reshape(B, 76)), hyp_off, sets, models, mask_off]
    d_in = [torch.from_numpy(a).to(dev) for a in host_in]
    d_sm = torch.full((10 * H + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if own_stream else None
    m.init_hypotheses_device(B, H, *d_in, d_sm[PAD:PAD + 10 * H], d_cnt[PAD:PAD + H], d_masks[PAD:PAD + MW], stream=stream)
    torch.cuda.synchronize()
    sm, cnt, masks = d_sm.cpu().numpy(), d_cnt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((sm, 10 * H), (cnt, H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    for k in range(B):
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        got = (sm[PAD + 10 * h0:PAD + 10 * h1].reshape(-1, 10), cnt[PAD + h0:PAD + h1],
               masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].view(np.uint32).reshape(want[k][2].shape))
        assert same(got, want[k]), ic.MIXED[k]
    for d, h in zip(d_in, host_in):                                              # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), h)
    m.init_hypotheses_device(0, 0, *([None] * 11))                              # nothing to do: nothing is read
    with pytest.raises(orbx.OrbxError) as e:
        m.init_hypotheses_device(B, H, *d_in[:3], None, *d_in[4:], d_sm[PAD:PAD + 10 * H], d_cnt[PAD:PAD + H], d_masks[PAD:PAD + MW])
    assert e.value.code == orbx.ORBX_E_INVALID


def test_the_frame_steps_over_empty_problems_and_zero_fills_a_problem_without_matches(m, orbx):
    """What the kernels' shared frame (csrc/orbm_hyp.h) decides, on the device form: a problem without hypotheses first and last,
    n = 33 with 3 hypotheses, n = 0 with 2 hypotheses (the host form refuses it; the kernel gives count 0, a zero row and no mask
    word), n = 65 with 2 hypotheses: H = 7 leaves a partial last workgroup."""
    import torch
    c65 = ic.BY_NAME["general65"]
    m33 = c65["matches12"].copy()
    m33[np.flatnonzero(m33 >= 0)[33:]] = -1                                      # the first 33 matches of the case
    s33, s65 = solver(orbx, dict(c65, matches12=m33)), solver(orbx, c65)
    assert (s33.N, s65.N) == (33, 65)
    rng = np.random.default_rng(33)
    sets33, models33 = np.stack([rng.permutation(33)[:8] for _ in range(3)]).astype(np.int32), np.array([0, 1, 0], np.int32)
    sets65, models65 = c65["sets"][:2], np.array([1, 0], np.int32)
    uv33, pn33, T1, T2, sigma = s33.problem()[:5]
    uv65, pn65, U1, U2, _ = s65.problem()[:5]
    none8, none1 = np.zeros((0, 8), np.int32), np.zeros(0, np.int32)
    nothing = (uv65[:9], pn65[:9], U1, U2, sigma, none8, none1)
    problems = [nothing, (uv33, pn33, T1, T2, sigma, sets33, models33),
                (uv65[:0], pn65[:0], U1, U2, sigma, np.zeros((2, 8), np.int32), np.array([0, 1], np.int32)),
                (uv65, pn65, U1, U2, sigma, sets65, models65), nothing]
    want = {1: s33.hypotheses(sets33, models33), 3: s65.hypotheses(sets65, models65)}     # the host path
    off, uv, pn, params, hyp_off, sets, models, mask_off = orbx.ORBmatcher.pack_init_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    assert (B, H, MW) == (5, 7, 3 * 2 + 2 * 3) and list(np.diff(off)) == [9, 33, 0, 65, 9] and list(np.diff(hyp_off)) == [0, 3, 2, 2, 0]
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (off, uv, pn, np.ascontiguousarray(params.view(np.uint8).reshape(B, 76)), hyp_off, sets,
                                                  models, mask_off)]
    d_sm = torch.full((10 * H + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.init_hypotheses_device(B, H, *d_in, d_sm[PAD:PAD + 10 * H], d_cnt[PAD:PAD + H], d_masks[PAD:PAD + MW])
    torch.cuda.synchronize()
    sm, cnt, masks = d_sm.cpu().numpy(), d_cnt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((sm, 10 * H), (cnt, H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    for k, w in want.items():                                                    # every mask word belongs to one of the two
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        got = (sm[PAD + 10 * h0:PAD + 10 * h1].reshape(-1, 10), cnt[PAD + h0:PAD + h1],
               masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].view(np.uint32).reshape(w[2].shape))
        assert same(got, w), k
        assert (w[0][:, 0] > 0).all()                                            # real scores
    assert mask_off[2] == mask_off[3] and (cnt[PAD + 3:PAD + 5] == 0).all()
    assert sm[PAD + 10 * 3:PAD + 10 * 5].tobytes() == bytes(4 * 10 * 2)


def rt_inputs(orbx, name):
    """(solver, uv, K, th2, inlier flags, motions) of the model the case's Initialize reconstructs"""
    s = solver(orbx, ic.BY_NAME[name])
    s.draw()
    model, M, inl, Rt = s.plan_check_rt()
    uv, K, th2 = s.check_rt_inputs()
    return s, uv, K, th2, inl, Rt, model


@pytest.mark.parametrize("name,n_motions", [("plane8", 8), ("general8", 4), ("plane65", 8), ("general65", 4), ("plane300", 8),
                                            ("general300", 4)])
def test_check_rt_equals_the_host_byte_for_byte(m, orbx, name, n_motions):
    s, uv, K, th2, inl, Rt, model = rt_inputs(orbx, name)
    assert len(Rt) == n_motions and th2 == 4.0
    n, k = len(uv), n_motions
    want = s.check_rt_matches(Rt, inl)
    status = np.full(k * n + 2 * PAD, 0xA5, np.uint8)
    cosp = np.full(k * n + 2 * PAD, GUARD, np.uint32)
    p3d = np.full(3 * k * n + 2 * PAD, GUARD, np.uint32)
    flags = np.ascontiguousarray(inl.astype(np.uint8))
    rc = m.L.orbm_init_check_rt(m.h, n, p(uv), p(flags), p(K), C.c_float(th2), k, p(Rt), p(status[PAD:]), p(cosp[PAD:]), p(p3d[PAD:]))
    assert rc == orbx.ORBX_OK, m.L.orbm_last_error()
    assert (status[:PAD] == 0xA5).all() and (status[PAD + k * n:] == 0xA5).all()
    for a, cnt in ((cosp, k * n), (p3d, 3 * k * n)):
        assert (a[:PAD] == GUARD).all() and (a[PAD + cnt:] == GUARD).all()
    got = (status[PAD:PAD + k * n].reshape(k, n), cosp[PAD:PAD + k * n].view(np.float32).reshape(k, n),
           p3d[PAD:PAD + 3 * k * n].view(np.float32).reshape(k, n, 3))
    for g, w, field in zip(got, want, ("status", "cos_parallax", "p3d")):
        assert g.tobytes() == w.tobytes(), "%s: %s differs from the host path" % (name, field)
    assert same(got, m.init_check_rt(uv, inl, K, th2, Rt))                       # the unguarded wrapper
    if n >= 65:                                                                  # the verdicts are not all one kind
        assert (got[0] <= orbx.ORBM_INIT_RT_GOOD_LOW_PARALLAX).any() and (got[0] >= orbx.ORBM_INIT_RT_BEHIND1).any()
    import torch
    dev = torch.device("cuda")
    d_uv, d_inl, d_Rt = (torch.from_numpy(a).to(dev) for a in (uv, flags, Rt))
    d_st = torch.full((k * n + 2 * PAD,), 0x5A, dtype=torch.uint8, device=dev)
    d_cos = torch.full((k * n + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    d_p3d = torch.full((3 * k * n + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    m.init_check_rt_device(n, d_uv, d_inl, K, th2, k, d_Rt, d_st[PAD:PAD + k * n], d_cos[PAD:PAD + k * n], d_p3d[PAD:PAD + 3 * k * n],
                           stream=stream)
    torch.cuda.synchronize()
    st, co, pt = d_st.cpu().numpy(), d_cos.cpu().numpy(), d_p3d.cpu().numpy()
    assert (st[:PAD] == 0x5A).all() and (st[PAD + k * n:] == 0x5A).all() and (co[:PAD] == -77).all() and (co[PAD + k * n:] == -77).all()
    assert (pt[:PAD] == -77).all() and (pt[PAD + 3 * k * n:] == -77).all()
    assert st[PAD:PAD + k * n].tobytes() == want[0].tobytes() and co[PAD:PAD + k * n].tobytes() == want[1].tobytes()
    assert pt[PAD:PAD + 3 * k * n].tobytes() == want[2].tobytes()
    assert np.array_equal(d_uv.cpu().numpy(), uv) and np.array_equal(d_inl.cpu().numpy(), flags) and np.array_equal(d_Rt.cpu().numpy(), Rt)


def test_degenerate_sets_stay_in_their_slots(m, orbx):
    """8 collinear points and a set with a repeated point: ORBX_OK, flags 0/1 with count = popcount (run() checks both and the
    guards), and the neighbours' bytes are those of a batch without the degenerate sets.  Values are not compared."""
    uv, pn, T1, T2, sigma, sets, models = problem(orbx, ic.BY_NAME["general65"], 3)
    uv, pn = uv.copy(), pn.copy()
    for j in range(8):                                                           # matches 10..17 lie on one line in both images
        pn[10 + j] = (0.25 * j - 1, 0.125 * j, 0.5 * j - 1.5, -0.25 * j + 0.5)
        uv[10 + j] = (100 + 16 * j, 80 + 8 * j, 90 + 32 * j, 300 - 16 * j)
    pn[19], uv[19] = pn[18], uv[18]                                             # 18 and 19 are one point
    line, twice = list(range(10, 18)), [18, 19, 20, 21, 22, 23, 24, 25]
    st = sets[:3]
    with_sets = np.array([st[0], line, st[1], twice, line, st[2], twice, st[0]], np.int32)
    with_models = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
    other = problem(orbx, ic.BY_NAME["plane64"], 5)
    with_deg = run(orbx, m, [(uv, pn, T1, T2, sigma, with_sets, with_models), other])
    without = run(orbx, m, [(uv, pn, T1, T2, sigma, with_sets[[0, 2, 5, 7]], with_models[[0, 2, 5, 7]]), other])
    assert same(tuple(a[[0, 2, 5, 7]] for a in with_deg[0]), without[0]) and same(with_deg[1], without[1])


def test_a_small_handle_grows_and_keeps_its_grid(orbx):
    """a batch larger than the workspace grows the handle; a windowed search gives the same answer before and after"""
    h = orbx.ORBmatcher(0.8, True, max_queries=256, max_train=8192, max_pairs=256)
    try:
        scene = F.suite_scene(0)
        fr = F.make_frame(np.random.default_rng(31), scene)
        bounds = tuple(float(b) for b in scene.view["bounds"])
        h.grid_build(fr.kps, *bounds)
        rng = np.random.default_rng(5)
        qx, qy = rng.uniform(0, bounds[1], 200).astype(np.float32), rng.uniform(0, bounds[3], 200).astype(np.float32)
        before = h.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        assert len(before[1]) > 0
        problems = mixed(orbx)                                                   # thousands of output words against 256
        got = run(orbx, h, problems)
        for g, (name, k) in zip(got, ic.MIXED):
            against_host(orbx, g, name, k, "grown handle")
        s, uv, K, th2, inl, Rt, model = rt_inputs(orbx, "plane300")
        assert same(h.init_check_rt(uv, inl, K, th2, Rt), s.check_rt_matches(Rt, inl))
        assert h.grid_count() == len(fr.kps)
        after = h.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(before, after))
        assert all(same(a, b) for a, b in zip(got, run(orbx, h, problems)))
    finally:
        h.close()


@pytest.mark.parametrize("name", [c["name"] for c in ic.CASES])
def test_initialize_through_the_gpu_equals_the_host_in_every_byte(m, orbx, name):
    case = ic.BY_NAME[name]
    on_host = solver(orbx, case)
    want = on_host.Initialize(case["keys2"], case["matches12"])
    s = solver(orbx, case)
    got = s.Initialize(case["keys2"], case["matches12"], matcher=m)
    assert s.LastError() == ""
    assert got[0] == want[0] == ic.expect_ok(case)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want))
    for model in (0, 1):                                                         # the walks replayed the GPU's results
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(s.find(model), on_host.find(model)))
    s.SetUseGpu(False)
    s.SetRand(ic.Lcg(case["seed"]), ic.RAND_MAX)
    again = s.Initialize(case["keys2"], case["matches12"], matcher=m)             # SetUseGpu(False): the host path, the same bytes
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(again, want))
