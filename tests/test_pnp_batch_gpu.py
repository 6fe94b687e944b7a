"""orbm_pnp_hypotheses / orbm_pnp_hypotheses_device (include/orbm.h) on the GPU against the host path orbp_pnp_hypothesis on the
cases of tests/pnp_cases.py: host and kernel run one body (csrc/orbp_epnp_body.h), so counts, the 96 bytes of R | t and the masks
are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import frustum_oracle as F
import pnp_cases as pc

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
    fx, fy, cx, cy = (float(v) for v in case["K"])
    s = orbx.PnPsolver(case["p2d"], case["sigma2"], case["p3d"], fx, fy, cx, cy, rand=pc.Lcg(case["seed"]) if scripted else None,
                       rand_max=pc.RAND_MAX)
    s.SetRansacParameters(*(case.get("params") or (0.99, min(10, case["N"]), 300, case["set_size"], 0.5, 5.991)))
    return s


def problem(orbx, case, samples):
    p2d, p3d, e, K, ms, _ = solver(orbx, case).problem()
    return (p2d, p3d, e, K, ms, np.asarray(samples, np.int32).reshape(-1, ms))


_HOST = {}


def host(orbx, case):
    """orbp_pnp_hypothesis on every sample of the case, once: (counts, Rt, masks)"""
    if case["name"] not in _HOST:
        _HOST[case["name"]] = solver(orbx, case).hypotheses(case["samples"])
    return _HOST[case["name"]]


def run(orbx, m, problems):
    """orbm_pnp_hypotheses with guard words around the three outputs -> [(counts, Rt, masks)] per problem"""
    off, p2d, p3d, e, cams, hyp_off, sm, mask_off = orbx.ORBmatcher.pack_pnp_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    cnt = np.full(H + 2 * PAD, GUARD, np.uint32)
    Rt = np.full(24 * H + 2 * PAD, GUARD, np.uint32)                            # PAD is even: the doubles stay 8-byte aligned
    masks = np.full(MW + 2 * PAD, GUARD, np.uint32)
    rc = m.L.orbm_pnp_hypotheses(m.h, B, p(off), p(p2d), p(p3d), p(e), p(cams), p(hyp_off), p(sm), p(mask_off), p(cnt[PAD:]), p(Rt[PAD:]),
                                 p(masks[PAD:]))
    assert rc == orbx.ORBX_OK, m.L.orbm_last_error()
    for a, n in ((cnt, H), (Rt, 24 * H), (masks, MW)):
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
        out.append((c, Rt[PAD + 24 * h0:PAD + 24 * h1].copy().view(np.float64).reshape(h1 - h0, 12), mk))
    return out


def same(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


def against_host(orbx, got, case, h, what=""):
    want = tuple(a[:h] for a in host(orbx, case))
    for g, w, field in zip(got, want, ("n_inliers", "Rt", "masks")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s %s h=%d: %s differs from the host path" % (what, case["name"], h, field)


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_single_problems_equal_the_host_byte_for_byte(m, orbx, name):
    """N = 4 (the sample is the whole problem) to 130, set_size 4 / 5 / 6 / 8, exact and noisy points at 4 to 200 m, a coplanar
    sample; 1, 3, 4, 5 and 9 hypotheses: around the 4 waves of a workgroup"""
    case = pc.BY_NAME[name]
    for h in pc.HYP_COUNTS:
        h = min(h, len(case["samples"]))
        got = run(orbx, m, [problem(orbx, case, case["samples"][:h])])
        against_host(orbx, got[0], case, h, "single")
    if name == "n33_s4_coplanar":                                                # its first sample lies in the world plane z = 0
        assert (case["p3d"][case["samples"][0], 2] == 0).all()
    if case["N"] == 4:
        assert sorted(case["samples"][0]) == [0, 1, 2, 3]
    if name == "n64_s6":                                                         # the planted pose, by hand: exact points, 6 right matches
        k = next(k for k, sm in enumerate(case["samples"]) if (sm >= case["wrong"]).all())
        cnt, Rt, mk = run(orbx, m, [problem(orbx, case, case["samples"][k:k + 1])])[0]
        assert np.abs(Rt[0, :9].reshape(3, 3) - case["R"]).max() < 1e-4 and np.abs(Rt[0, 9:] - case["t"]).max() < 1e-2
        bits = np.unpackbits(mk.view(np.uint8), bitorder="little")[:case["N"]].astype(bool)
        assert not bits[:case["wrong"]].any() and bits[case["wrong"]:].all() and cnt[0] == case["N"] - case["wrong"]


def mixed(orbx):
    return [problem(orbx, pc.BY_NAME[name], pc.BY_NAME[name]["samples"][:h]) for name, h in pc.MIXED]


def test_mixed_batch_equals_the_host_problem_by_problem(m, orbx):
    problems = mixed(orbx)
    assert len({pr[4] for pr in problems}) >= 4 and len({tuple(pr[3]) for pr in problems}) == 3 and len(problems[2][5]) == 0
    got = run(orbx, m, problems)
    for g, (name, h) in zip(got, pc.MIXED):
        against_host(orbx, g, pc.BY_NAME[name], h, "mixed")


def test_a_result_depends_on_its_problem_and_sample_alone(m, orbx):
    problems = mixed(orbx)
    batch = run(orbx, m, problems)
    for g, pr in zip(batch, problems):
        assert same(g, run(orbx, m, [pr])[0])                                    # the batch equals the single-problem calls
    assert all(same(a, b) for a, b in zip(batch, run(orbx, m, problems)))         # a second run
    assert all(same(a, b) for a, b in zip(batch, run(orbx, m, problems[::-1])[::-1]))
    # the same hypothesis at another position of its problem
    p2d, p3d, e, K, ms, sm = problems[0]
    rev = run(orbx, m, [(p2d, p3d, e, K, ms, sm[::-1])])[0]
    assert same(tuple(a[::-1] for a in rev), batch[0])
    via_python = m.pnp_hypotheses(problems)                                      # the unguarded wrapper
    assert all(same(a, b) for a, b in zip(batch, via_python))


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_pointer_form_gives_the_same_bytes(m, orbx, own_stream):
    import torch
    problems = mixed(orbx)
    want = run(orbx, m, problems)
    off, p2d, p3d, e, cams, hyp_off, sm, mask_off = orbx.ORBmatcher.pack_pnp_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    dev = torch.device("cuda")
    host_in = [off, p2d, p3d, e, np.ascontiguousarray(cams.view(np.uint8).reshape(B, 20)), hyp_off, sm, mask_off]
    d_in = [torch.from_numpy(a).to(dev) for a in host_in]
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_Rt = torch.full((12 * H + 2 * PAD,), -77.0, dtype=torch.float64, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if own_stream else None
    m.pnp_hypotheses_device(B, H, *d_in, d_cnt[PAD:PAD + H], d_Rt[PAD:PAD + 12 * H], d_masks[PAD:PAD + MW], stream=stream)
    torch.cuda.synchronize()
    cnt, Rt, masks = d_cnt.cpu().numpy(), d_Rt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((cnt, H), (Rt, 12 * H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    for k in range(B):
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        got = (cnt[PAD + h0:PAD + h1], Rt[PAD + 12 * h0:PAD + 12 * h1].reshape(-1, 12),
               masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].view(np.uint32).reshape(want[k][2].shape))
        assert same(got, want[k]), pc.MIXED[k]
    for d, h in zip(d_in, host_in):                                              # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), h)
    m.pnp_hypotheses_device(0, 0, *([None] * 11))                               # nothing to do: nothing is read
    with pytest.raises(orbx.OrbxError) as e:
        m.pnp_hypotheses_device(B, H, *d_in[:4], None, *d_in[5:], d_cnt[PAD:PAD + H], d_Rt[PAD:PAD + 12 * H], d_masks[PAD:PAD + MW])
    assert e.value.code == orbx.ORBX_E_INVALID


def test_the_frame_steps_over_empty_problems_and_zero_fills_a_problem_without_correspondences(m, orbx):
    """What the kernels' shared frame (csrc/orbm_hyp.h) decides, on the device form: a problem without hypotheses first and last,
    n = 33 with 3 hypotheses, n = 0 with 2 hypotheses (the host form refuses it; the kernel gives count 0, a zero row and no mask
    word), n = 65 with 2 hypotheses: H = 7 leaves a partial last workgroup."""
    import torch
    c33, c65 = pc.BY_NAME["n33_s8"], pc.BY_NAME["n65_s6"]
    nothing = problem(orbx, pc.BY_NAME["n64_s5"], [])
    no_points = (np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), c33["K"], 4, np.zeros((2, 4), np.int32))
    problems = [nothing, problem(orbx, c33, c33["samples"][:3]), no_points, problem(orbx, c65, c65["samples"][:2]), nothing]
    want = {1: tuple(a[:3] for a in host(orbx, c33)), 3: tuple(a[:2] for a in host(orbx, c65))}     # the host path
    off, p2d, p3d, e, cams, hyp_off, sm, mask_off = orbx.ORBmatcher.pack_pnp_problems(problems)
    B, H, MW = len(problems), int(hyp_off[-1]), int(mask_off[-1])
    assert (B, H, MW) == (5, 7, 3 * 2 + 2 * 3) and list(np.diff(off)) == [64, 33, 0, 65, 64] and list(np.diff(hyp_off)) == [0, 3, 2, 2, 0]
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (off, p2d, p3d, e, np.ascontiguousarray(cams.view(np.uint8).reshape(B, 20)), hyp_off, sm,
                                                  mask_off)]
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_Rt = torch.full((12 * H + 2 * PAD,), -77.0, dtype=torch.float64, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.pnp_hypotheses_device(B, H, *d_in, d_cnt[PAD:PAD + H], d_Rt[PAD:PAD + 12 * H], d_masks[PAD:PAD + MW])
    torch.cuda.synchronize()
    cnt, Rt, masks = d_cnt.cpu().numpy(), d_Rt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((cnt, H), (Rt, 12 * H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    for k, w in want.items():                                                    # every mask word belongs to one of the two
        h0, h1 = int(hyp_off[k]), int(hyp_off[k + 1])
        got = (cnt[PAD + h0:PAD + h1], Rt[PAD + 12 * h0:PAD + 12 * h1].reshape(-1, 12),
               masks[PAD + mask_off[k]:PAD + mask_off[k + 1]].view(np.uint32).reshape(w[2].shape))
        assert same(got, w), k
    assert mask_off[2] == mask_off[3] and (cnt[PAD + 3:PAD + 5] == 0).all()
    assert Rt[PAD + 12 * 3:PAD + 12 * 5].tobytes() == bytes(8 * 12 * 2)


def test_a_small_handle_grows_and_keeps_its_grid(orbx):
    """a batch larger than the workspace grows the handle; a windowed search gives the same answer before and after"""
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=8192, max_pairs=64)
    try:
        scene = F.suite_scene(0)
        fr = F.make_frame(np.random.default_rng(31), scene)
        bounds = tuple(float(b) for b in scene.view["bounds"])
        h.grid_build(fr.kps, *bounds)
        rng = np.random.default_rng(5)
        qx, qy = rng.uniform(0, bounds[1], 60).astype(np.float32), rng.uniform(0, bounds[3], 60).astype(np.float32)
        before = h.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        assert len(before[1]) > 0
        problems = mixed(orbx)                                                   # 21 hypotheses: 25 words each + masks, against 192
        got = run(orbx, h, problems)
        for g, (name, k) in zip(got, pc.MIXED):
            against_host(orbx, g, pc.BY_NAME[name], k, "grown handle")
        assert h.grid_count() == len(fr.kps)
        after = h.GetFeaturesInArea(qx, qy, 25.0, 0, 3)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(before, after))
        assert all(same(a, b) for a, b in zip(got, run(orbx, h, problems)))
    finally:
        h.close()


def _relocalization_loop(solvers):
    """the while loop of Tracking::Relocalization (:1403-1418) without its early exit: iterate(5) round-robin until every solver
    says bNoMore; the trace of every call"""
    trace, alive = [], [s is not None for s in solvers]
    while any(alive):
        for i, s in enumerate(solvers):
            if not alive[i]:
                continue
            T, no_more, flags, n = s.iterate(5)
            if no_more:
                alive[i] = False
            trace.append((i, None if T is None else T.tobytes(), no_more, None if flags is None else flags.tobytes(), n,
                          s.ransac_state()["iterations"]))
    return trace


def test_evaluate_all_then_replay_equals_the_all_host_run(m, orbx):
    keys = ("never", "early", "set6", "late")
    want = _relocalization_loop([solver(orbx, pc.ransac_case(k)) for k in keys])
    first = next(t for t in want if t[1] is not None)
    assert first[0] == 1 and first[5] < 35 and not first[2]                        # "early" returns a pose before its queue is used up
    solvers = [solver(orbx, pc.ransac_case(k)) for k in keys]
    orbx.PnPsolver.EvaluateAll(solvers[:2] + [None] + solvers[2:], m)             # a NULL entry of vpPnPsolvers is skipped
    assert [len(s.queued()) for s in solvers] == [max(s.ransac_state()["max_its"], 5) for s in solvers]
    got = _relocalization_loop(solvers)
    assert got == want


def test_degenerate_samples_stay_in_their_slots(m, orbx):
    """a sample with a repeated 3-D point and one of four collinear points: ORBX_OK, flags 0/1 with count = popcount (run() checks
    both and the guards), and the neighbours' bytes are those of a batch without the degenerate samples.  Values are not compared."""
    case = dict(pc.BY_NAME["n65_s4"])
    p3d, p2d = case["p3d"].copy(), case["p2d"].copy()
    d = np.array([0.25, -0.125, 0.5], np.float32)                                # exact in float32: 10 .. 13 are collinear
    for k in (1, 2, 3):
        p3d[10 + k] = p3d[10] + k * d
    p3d[21], p2d[21] = p3d[20], p2d[20]                                          # 20 and 21 are one point
    case["p3d"], case["p2d"], case["name"] = p3d, p2d, "n65_s4_degenerate"
    s = case["samples"]
    other = problem(orbx, pc.BY_NAME["n64_s5"], pc.BY_NAME["n64_s5"]["samples"][:5])
    keep = [k for k in range(len(s)) if not set(s[k]) & {10, 11, 12, 13, 20, 21}][:3]
    assert len(keep) == 3
    a, b, c = (s[k] for k in keep)
    with_deg = run(orbx, m, [problem(orbx, case, [a, [10, 11, 12, 13], b, [20, 21, 30, 31], c]), other])
    without = run(orbx, m, [problem(orbx, case, [a, b, c]), other])
    assert same(tuple(x[[0, 2, 4]] for x in with_deg[0]), without[0]) and same(with_deg[1], without[1])
