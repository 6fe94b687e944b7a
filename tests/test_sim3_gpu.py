"""orbm_sim3_hypotheses / orbm_sim3_hypotheses_device (include/orbm.h) on the GPU against the host path orbp_sim3_hypothesis on the
cases of tests/sim3_cases.py: host and kernel run one body (csrc/orbm_sim3_body.h), so counts, s / R / t and masks are compared
byte for byte."""
import ctypes as C

import numpy as np
import pytest

import frustum_oracle as F
import sim3_cases as sc

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


def solver(orbx, case, scripted=True):
    s = orbx.Sim3Solver(case["x1"], case["x2"], case["sigma2_1"], case["sigma2_2"], case["K1"], case["K2"], case["fix"],
                        rand=sc.Lcg(case["seed"]) if scripted else None, rand_max=sc.RAND_MAX)
    s.SetRansacParameters(sc.PROBABILITY, sc.MIN_INLIERS, sc.MAX_ITERATIONS)
    return s


def problem(orbx, case, triples):
    s = solver(orbx, case)
    e1, e2 = s.max_errors()
    return (s.x1, s.x2, e1, e2, s.K1, s.K2, s.fix_scale, np.asarray(triples, np.int32).reshape(-1, 3))


_HOST = {}


def host(orbx, name):
    """orbp_sim3_hypothesis on every triple of the case, once: (counts, sRt, masks)"""
    if name not in _HOST:
        case = sc.BY_NAME[name]
        _HOST[name] = solver(orbx, case).hypotheses(case["triples"])
    return _HOST[name]


def run(orbx, m, problems):
    """orbm_sim3_hypotheses with guard words around the three outputs -> [(counts, sRt, masks)] per problem"""
    off, x1, x2, e1, e2, cams, hyp_off, tri, mask_off = orbx.ORBmatcher.pack_sim3_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    cnt = np.full(H + 2 * PAD, GUARD, np.uint32)
    sRt = np.full(13 * H + 2 * PAD, GUARD, np.uint32)
    masks = np.full(MW + 2 * PAD, GUARD, np.uint32)
    rc = m.L.orbm_sim3_hypotheses(m.h, B, p(off), p(x1), p(x2), p(e1), p(e2), p(cams), p(hyp_off), p(tri), p(mask_off),
                                  p(cnt[PAD:]), p(sRt[PAD:]), p(masks[PAD:]))
    assert rc == orbx.ORBX_OK, m.L.orbm_last_error()
    for a, n in ((cnt, H), (sRt, 13 * H), (masks, MW)):
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
        out.append((c, sRt[PAD + 13 * h0:PAD + 13 * h1].view(np.float32).reshape(h1 - h0, 13).copy(), mk))
    return out


def same(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


def against_host(orbx, got, name, h, what=""):
    want = tuple(a[:h] for a in host(orbx, name))
    for g, w, field in zip(got, want, ("n_inliers", "sRt", "masks")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s %s h=%d: %s differs from the host path" % (what, name, h, field)


@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES])
def test_single_problems_equal_the_host_byte_for_byte(m, orbx, name):
    case = sc.BY_NAME[name]
    for h in sc.HYP_COUNTS:
        h = min(h, len(case["triples"]))
        got = run(orbx, m, [problem(orbx, case, case["triples"][:h])])
        against_host(orbx, got[0], name, h, "single")
    if case["N"] >= 21:                                                          # the planted answer, by hand: an all-inlier triple
        k = next(k for k, tri in enumerate(case["triples"]) if not case["outlier"][tri].any())
        cnt, sRt, mk = run(orbx, m, [problem(orbx, case, case["triples"][k:k + 1])])[0]
        bits = np.unpackbits(mk.view(np.uint8), bitorder="little")[:case["N"]].astype(bool)
        assert np.array_equal(bits, ~case["outlier"]) and cnt[0] == int((~case["outlier"]).sum())
        want = np.concatenate([[case["s"]], case["R"].reshape(9), case["t"]])
        assert (np.abs(sRt[0] - want) / np.maximum(1, np.abs(want))).max() <= sc.SRT_TOL


def mixed(orbx):
    return [problem(orbx, sc.BY_NAME[name], sc.BY_NAME[name]["triples"][:h]) for name, h in sc.MIXED]


def test_mixed_batch_equals_the_host_problem_by_problem(m, orbx):
    got = run(orbx, m, mixed(orbx))
    for g, (name, h) in zip(got, sc.MIXED):
        against_host(orbx, g, name, h, "mixed")


def test_a_result_depends_on_its_problem_and_triple_alone(m, orbx):
    problems = mixed(orbx)
    batch = run(orbx, m, problems)
    for g, pr in zip(batch, problems):
        assert same(g, run(orbx, m, [pr])[0])                                    # the batch equals the single-problem calls
    assert all(same(a, b) for a, b in zip(batch, run(orbx, m, problems)))         # a second run
    assert all(same(a, b) for a, b in zip(batch, run(orbx, m, problems[::-1])[::-1]))
    via_python = m.sim3_hypotheses(problems)                                      # the unguarded wrapper
    assert all(same(a, b) for a, b in zip(batch, via_python))


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_pointer_form_gives_the_same_bytes(m, orbx, own_stream):
    import torch
    problems = mixed(orbx)
    want = run(orbx, m, problems)
    off, x1, x2, e1, e2, cams, hyp_off, tri, mask_off = orbx.ORBmatcher.pack_sim3_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    dev = torch.device("cuda")
    host_in = [off, x1, x2, e1, e2, np.ascontiguousarray(cams.view(np.uint8).reshape(B, 36)), hyp_off, tri, mask_off]
    d_in = [torch.from_numpy(a).to(dev) for a in host_in]
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_sRt = torch.full((13 * H + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if own_stream else None
    m.sim3_hypotheses_device(B, H, *d_in, d_cnt[PAD:PAD + H], d_sRt[PAD:PAD + 13 * H], d_masks[PAD:PAD + MW], stream=stream)
    torch.cuda.synchronize()
    cnt, sRt, masks = d_cnt.cpu().numpy(), d_sRt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((cnt, H), (sRt, 13 * H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    for k in range(B):
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        got = (cnt[PAD + h0:PAD + h1], sRt[PAD + 13 * h0:PAD + 13 * h1].reshape(-1, 13),
               masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].view(np.uint32).reshape(want[k][2].shape))
        assert same(got, want[k]), sc.MIXED[k]
    for d, h in zip(d_in, host_in):                                              # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), h)
    m.sim3_hypotheses_device(0, 0, *([None] * 12))                              # nothing to do: nothing is read
    with pytest.raises(orbx.OrbxError) as e:
        m.sim3_hypotheses_device(B, H, *d_in[:5], None, *d_in[6:], d_cnt[PAD:PAD + H], d_sRt[PAD:PAD + 13 * H], d_masks[PAD:PAD + MW])
    assert e.value.code == orbx.ORBX_E_INVALID


def test_the_frame_steps_over_empty_problems_and_zero_fills_a_problem_without_correspondences(m, orbx):
    """What the kernels' shared frame (csrc/orbm_hyp.h) decides, on the device form: a problem without hypotheses first and last,
    n = 33 with 3 hypotheses, n = 0 with 2 hypotheses (the host form refuses it; the kernel gives count 0, a zero row and no mask
    word), n = 65 with 2 hypotheses: H = 7 leaves a partial last workgroup."""
    import torch
    c65 = sc.BY_NAME["n65_free"]
    c33 = dict(c65, **{k: c65[k][:33] for k in ("x1", "x2", "sigma2_1", "sigma2_2")})     # its first 33 correspondences
    tri33 = np.array([t for t in c65["triples"] if t.max() < 33][:3], np.int32)
    tri65 = c65["triples"][:2]
    assert tri33.shape == (3, 3)
    nothing = problem(orbx, sc.BY_NAME["n21_free"], [])
    problems = [nothing, problem(orbx, c33, tri33), problem(orbx, sc.BY_NAME["n0_free"], np.zeros((2, 3), np.int32)),
                problem(orbx, c65, tri65), nothing]
    want = {1: solver(orbx, c33).hypotheses(tri33), 3: solver(orbx, c65).hypotheses(tri65)}     # the host path
    off, x1, x2, e1, e2, cams, hyp_off, tri, mask_off = orbx.ORBmatcher.pack_sim3_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    assert (B, H, MW) == (5, 7, 3 * 2 + 2 * 3) and list(np.diff(off)) == [21, 33, 0, 65, 21] and list(np.diff(hyp_off)) == [0, 3, 2, 2, 0]
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (off, x1, x2, e1, e2, np.ascontiguousarray(cams.view(np.uint8).reshape(B, 36)), hyp_off,
                                                  tri, mask_off)]
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_sRt = torch.full((13 * H + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.sim3_hypotheses_device(B, H, *d_in, d_cnt[PAD:PAD + H], d_sRt[PAD:PAD + 13 * H], d_masks[PAD:PAD + MW])
    torch.cuda.synchronize()
    cnt, sRt, masks = d_cnt.cpu().numpy(), d_sRt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((cnt, H), (sRt, 13 * H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    for k, w in want.items():                                                    # every mask word belongs to one of the two
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        got = (cnt[PAD + h0:PAD + h1], sRt[PAD + 13 * h0:PAD + 13 * h1].reshape(-1, 13),
               masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].view(np.uint32).reshape(w[2].shape))
        assert same(got, w), k
    assert mask_off[2] == mask_off[3] and (cnt[PAD + 3:PAD + 5] == 0).all()
    assert sRt[PAD + 13 * 3:PAD + 13 * 5].tobytes() == bytes(4 * 13 * 2)


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
        for g, (name, k) in zip(got, sc.MIXED):
            against_host(orbx, g, name, k, "grown handle")
        assert h.grid_count() == len(fr.kps)
        after = h.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(before, after))
        assert all(same(a, b) for a, b in zip(got, run(orbx, h, problems)))
    finally:
        h.close()


def _compute_sim3_loop(solvers):
    """the while loop of LoopClosing::ComputeSim3 (:287-343) without its early exit: iterate(5) round-robin until every solver
    says bNoMore; the trace of every call"""
    trace, alive = [], [s is not None for s in solvers]
    while any(alive):
        for i, s in enumerate(solvers):
            if not alive[i]:
                continue
            T, no_more, flags, n = s.iterate(5)
            if no_more:
                alive[i] = False
            est = s.estimated()
            trace.append((i, None if T is None else T.tobytes(), no_more, flags.tobytes(), n, s.ransac_state()["iterations"],
                          s.ransac_state()["best_inliers"], None if est is None else tuple(a.tobytes() for a in est)))
    return trace


def test_evaluate_all_then_replay_equals_the_all_host_run(m, orbx):
    names = ("n129_fix", "n128_fix", "n19_fix", "n300_fix", "n64_free")
    want = _compute_sim3_loop([solver(orbx, sc.BY_NAME[n]) for n in names])
    first = next(t for t in want if t[1] is not None)
    assert first[0] == 3 and first[5] == 3 and first[4] == 225                     # n300_fix at its third triple, by hand from the case
    solvers = [solver(orbx, sc.BY_NAME[n]) for n in names]
    orbx.Sim3Solver.EvaluateAll(solvers + [None], m)                              # a NULL entry of vpSim3Solvers is skipped
    assert [len(s.queued()) for s in solvers] == [s.ransac_state()["max_its"] if s.N >= sc.MIN_INLIERS else 0 for s in solvers]
    got = _compute_sim3_loop(solvers)
    assert got == want


def test_degenerate_triples_stay_in_their_slots(m, orbx):
    """three collinear points and two coincident points: ORBX_OK, flags 0/1 with count = popcount (run() checks both and the guards),
    and the neighbours' bytes are those of a batch without the degenerate triples.  Values are not compared."""
    case = dict(sc.BY_NAME["n65_free"])
    x1, x2 = case["x1"].copy(), case["x2"].copy()
    d = np.array([0.25, -0.125, 0.5], np.float32)                                # exact in float32: 10, 11, 12 are collinear in camera 2
    x2[11], x2[12] = x2[10] + d, x2[10] + 2 * d
    x1[10:13] = (case["s"] * (x2[10:13].astype(np.float64) @ case["R"].T) + case["t"]).astype(np.float32)
    x2[14], x1[14] = x2[13], x1[13]                                              # 13 and 14 coincide
    case["x1"], case["x2"] = x1, x2
    t = case["triples"]
    other = problem(orbx, sc.BY_NAME["n64_fix"], sc.BY_NAME["n64_fix"]["triples"][:5])
    with_deg = run(orbx, m, [problem(orbx, case, [t[0], [10, 11, 12], t[1], [13, 14, 20], [13, 13, 13], t[2]]), other])
    without = run(orbx, m, [problem(orbx, case, [t[0], t[1], t[2]]), other])
    keep = [0, 2, 5]
    assert same(tuple(a[keep] for a in with_deg[0]), without[0]) and same(with_deg[1], without[1])
