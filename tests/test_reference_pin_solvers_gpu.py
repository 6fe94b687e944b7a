"""The three hypothesis kernels (k_sim3_hypotheses, k_pnp_hypotheses, k_init_hypotheses) and k_init_check_rt against the records of
the reference's own src/Sim3Solver.cc, src/PnPsolver.cc and src/Initializer.cc (oracle/ref/ref_sim3.cc, ref_pnp.cc, ref_init.cc),
directly: tests/ref_solvers.py runs the library on the reference's request with every hypothesis taken from the GPU call
(Sim3Solver / PnPsolver EvaluateAll-then-replay, Initializer.Initialize with a matcher) and ref_solvers.check() applies the rules of
tests/test_reference_pin_solvers_cpu.py: flags, counts, draws, winners and transcripts exactly, values within 4 x the spread of the
reference's own two arithmetic variants.  It reads nothing of the reference but the binaries under oracle/_ref/ and the recorded
fixtures under tests/golden/solvers/.

Four-point EPnP is the library's documented own definition; ref_solvers.basis_decided_fields leaves the fields it
decides out of the comparison for requests with minSet = 4, as in the CPU module, which also shows the two side by side.

Beyond the per-case runs: one mixed batch per hypothesis kernel (Sim3, PnP, Initializer), every `_device` entry point on padded
device buffers (sim3, pnp, init hypotheses, init CheckRT), and k_init_check_rt given the motions and inlier flags the REFERENCE
recorded, its per-match outputs reduced as CheckRT reduces its loop (ref_solvers.reduce_check_rt) and compared motion by motion, in
the reference's order: nGood and vbGood exactly, points and parallax within tolerance."""
import numpy as np
import pytest

import ref_solvers as rs
import sim3_cases as sc

pytestmark = pytest.mark.gpu
FIXTURES = rs.load_fixtures()
NAMES = [(k, n) for k, n, _ in rs.pinned_requests()]
IDS = ["%s-%s" % kn for kn in NAMES]
PAD = 16


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


def expected(kind, records):
    return rs.sim3_reference_as_library(records.by) if kind == "sim3" else records.by


@pytest.mark.parametrize("kind,name", NAMES, ids=IDS)
def test_gpu_hypotheses_and_replays_equal_the_recorded_reference(m, orbx, kind, name):
    """from the fixtures alone: single problems, the EvaluateAll-then-replay transcripts, the whole GPU Initialize"""
    req, rsp = FIXTURES[(kind, name)]
    got = getattr(rs, "lib_" + kind)(orbx, rs.Records(req), m)
    rs.check(kind, got, expected(kind, rs.Records(rsp)), rs.basis_decided_fields(kind, rs.Records(req)))


def test_gpu_equals_the_reference_binaries(m, orbx):
    if not rs.ensure(allow_build=False):
        pytest.skip("no reference binaries under oracle/_ref: the fixtures stand in")
    reqs = rs.pinned_requests()
    failures = []
    for (kind, name, req), (rc, data, err) in zip(reqs, rs.run_many([(k, r, "") for k, _, r in reqs])):
        assert rc == 0 and data == FIXTURES[(kind, name)][1], (kind, name, rc, err)
        try:
            rs.check(kind, getattr(rs, "lib_" + kind)(orbx, rs.Records(req), m), expected(kind, rs.Records(data)),
                     rs.basis_decided_fields(kind, rs.Records(req)))
        except AssertionError as e:
            failures.append((kind, name, str(e)[:300]))
    assert not failures, failures


def _sim3_solver(orbx, req):
    r = rs.Records(req)
    fix, seed, min_inliers, max_its = [int(v) for v in r.one("ipar").reshape(-1)[:4]]
    s = orbx.Sim3Solver(r.one("x1"), r.one("x2"), r.one("sig1").reshape(-1), r.one("sig2").reshape(-1), r.one("K1").reshape(-1),
                        r.one("K2").reshape(-1), bool(fix), rand=sc.Lcg(seed), rand_max=sc.RAND_MAX)
    s.SetRansacParameters(float(r.one("prob")[0, 0]), min_inliers, max_its)
    return s


def _check_sim3_hypotheses(name, triples, cnt, sRt, masks, ref, N):
    """the rows of one problem of an orbm_sim3_hypotheses call against the reference's per-hypothesis records"""
    ran = [k for k in range(len(ref["ran"])) if int(ref["ran"][k][0, 0])]
    assert len(triples) == len(ran) > 0, name
    for row, k in enumerate(ran):
        bits = np.unpackbits(np.ascontiguousarray(masks[row]).view(np.uint8), bitorder="little")
        assert np.array_equal(triples[row], ref["tri"][k].reshape(-1)), (name, k)
        assert int(cnt[row]) == int(ref["ninl"][k][0, 0]) and np.array_equal(bits[:N], ref["inl"][k].reshape(-1)) and not bits[N:].any(), (name, k)
        want = np.concatenate([ref["s"][k].reshape(-1), ref["R"][k].reshape(-1), ref["t"][k].reshape(-1)])
        assert rs.deviation(sRt[row], want) <= rs.tol("sim3_srt"), (name, k)


MIXED = ("hyp_n129_fix", "hyp_n3_fix", "hyp_n64_fix", "hyp_n65_free", "hyp_thresholds")


def test_sim3_mixed_batch_in_one_call(m, orbx):
    """all N classes (one mask word, two, three; N = 3) in ONE orbm_sim3_hypotheses call, each problem against its reference records"""
    solvers = [_sim3_solver(orbx, FIXTURES[("sim3", n)][0]) for n in MIXED]
    triples = [s.draw(s.ransac_state()["max_its"]) for s in solvers]
    for name, s, tri, (cnt, sRt, masks) in zip(MIXED, solvers, triples, m.sim3_hypotheses(solvers)):
        _check_sim3_hypotheses(name, tri, cnt, sRt, masks, rs.Records(FIXTURES[("sim3", name)][1]).by, s.N)


def test_sim3_device_pointer_form(m, orbx):
    import torch
    name = "hyp_n65_free"
    s = _sim3_solver(orbx, FIXTURES[("sim3", name)][0])
    tri = s.draw(s.ransac_state()["max_its"])
    off, x1, x2, e1, e2, cams, hyp_off, triples, mask_off = orbx.ORBmatcher.pack_sim3_problems([s.problem()])
    H, MW = int(hyp_off[-1]), int(mask_off[-1])
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (off, x1, x2, e1, e2, np.ascontiguousarray(cams.view(np.uint8).reshape(1, 36)), hyp_off, triples, mask_off)]
    d_cnt = torch.full((H + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    d_sRt = torch.full((13 * H + 2 * PAD,), -77.0, dtype=torch.float32, device=dev)
    d_masks = torch.full((MW + 2 * PAD,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.sim3_hypotheses_device(1, H, *d_in, d_cnt[PAD:PAD + H], d_sRt[PAD:PAD + 13 * H], d_masks[PAD:PAD + MW])
    torch.cuda.synchronize()
    cnt, sRt, masks = d_cnt.cpu().numpy(), d_sRt.cpu().numpy(), d_masks.cpu().numpy()
    for a, n in ((cnt, H), (sRt, 13 * H), (masks, MW)):
        assert (a[:PAD] == -77).all() and (a[PAD + n:] == -77).all()
    _check_sim3_hypotheses(name, tri, cnt[PAD:PAD + H], sRt[PAD:PAD + 13 * H].reshape(H, 13), masks[PAD:PAD + MW].view(np.uint32).reshape(H, -1),
                           rs.Records(FIXTURES[("sim3", name)][1]).by, s.N)


def test_pnp_mixed_batch_in_one_call(m, orbx):
    """samples of 5, 6 and 8 points over one, two and three mask words in ONE orbm_pnp_hypotheses call"""
    names = ("hyp_p129_s8", "hyp_p5_s5", "hyp_p65_s6", "hyp_p64_s5")
    solvers, samples = [], []
    for n in names:
        r = rs.Records(FIXTURES[("pnp", n)][0])
        seed, _, _, min_set, _, _, calls = [int(x) for x in r.one("ipar").reshape(-1)]
        eps, th2 = [float(x) for x in r.one("fpar").reshape(-1)]
        s = orbx.PnPsolver(r.one("p2d"), r.one("sig2").reshape(-1), r.one("p3d"), *[float(x) for x in r.one("K").reshape(-1)],
                           rand=sc.Lcg(seed), rand_max=sc.RAND_MAX)
        s.SetRansacParameters(float(r.one("prob")[0, 0]), s.N, calls, min_set, eps, th2)     # minInliers = N: max_its = 1, and the `||` loop
        sm = s.draw(calls)                                                                # makes a coming iterate(calls) consume `calls` draws
        assert len(sm) == calls
        solvers.append(s)
        samples.append(sm)
    for n, s, sm, (cnt, Rt, masks) in zip(names, solvers, samples, m.pnp_hypotheses(solvers)):
        ref = rs.Records(FIXTURES[("pnp", n)][1]).by
        for k in range(len(sm)):
            bits = np.unpackbits(np.ascontiguousarray(masks[k]).view(np.uint8), bitorder="little")
            assert np.array_equal(sm[k], ref["sample"][k].reshape(-1)), (n, k)
            assert int(cnt[k]) == int(ref["ninl"][k][0, 0]) and np.array_equal(bits[:s.N], ref["inl"][k].reshape(-1)), (n, k)
            want = np.concatenate([ref["R"][k].reshape(-1), ref["t"][k].reshape(-1)])
            assert rs.deviation(Rt[k], want) <= rs.tol("pnp_rt"), (n, k)


def _padded(torch, n, dtype, fill=-77):
    return torch.full((n + 2 * PAD,), fill, dtype=dtype, device=torch.device("cuda"))


def _guards_intact(a, n, fill=-77):
    return (a[:PAD] == fill).all() and (a[PAD + n:] == fill).all()


def test_pnp_device_pointer_form(m, orbx):
    """orbm_pnp_hypotheses_device on padded device buffers against the reference's per-hypothesis records"""
    import torch
    name = "hyp_p65_s6"
    r = rs.Records(FIXTURES[("pnp", name)][0])
    seed, _, _, min_set, _, _, calls = [int(x) for x in r.one("ipar").reshape(-1)]
    eps, th2 = [float(x) for x in r.one("fpar").reshape(-1)]
    s = orbx.PnPsolver(r.one("p2d"), r.one("sig2").reshape(-1), r.one("p3d"), *[float(x) for x in r.one("K").reshape(-1)],
                       rand=sc.Lcg(seed), rand_max=sc.RAND_MAX)
    s.SetRansacParameters(float(r.one("prob")[0, 0]), s.N, calls, min_set, eps, th2)
    sm = s.draw(calls)
    off, p2d, p3d, e, cams, hyp_off, samples, mask_off = orbx.ORBmatcher.pack_pnp_problems([s])
    H, MW = int(hyp_off[-1]), int(mask_off[-1])
    assert H == calls == len(sm)
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (off, p2d, p3d, e, np.ascontiguousarray(cams.view(np.uint8).reshape(1, -1)), hyp_off, samples, mask_off)]
    d_cnt, d_Rt, d_masks = _padded(torch, H, torch.int32), _padded(torch, 12 * H, torch.float64, -77.0), _padded(torch, MW, torch.int32)
    torch.cuda.synchronize()
    m.pnp_hypotheses_device(1, H, *d_in, d_cnt[PAD:PAD + H], d_Rt[PAD:PAD + 12 * H], d_masks[PAD:PAD + MW])
    torch.cuda.synchronize()
    cnt, Rt, masks = d_cnt.cpu().numpy(), d_Rt.cpu().numpy(), d_masks.cpu().numpy()
    assert _guards_intact(cnt, H) and _guards_intact(Rt, 12 * H) and _guards_intact(masks, MW)
    cnt, Rt, masks = cnt[PAD:PAD + H], Rt[PAD:PAD + 12 * H].reshape(H, 12), masks[PAD:PAD + MW].view(np.uint32).reshape(H, -1)
    ref = rs.Records(FIXTURES[("pnp", name)][1]).by
    for k in range(H):
        bits = np.unpackbits(np.ascontiguousarray(masks[k]).view(np.uint8), bitorder="little")
        assert np.array_equal(sm[k], ref["sample"][k].reshape(-1)), k
        assert int(cnt[k]) == int(ref["ninl"][k][0, 0]) and np.array_equal(bits[:s.N], ref["inl"][k].reshape(-1)) and not bits[s.N:].any(), k
        assert rs.deviation(Rt[k], np.concatenate([ref["R"][k].reshape(-1), ref["t"][k].reshape(-1)])) <= rs.tol("pnp_rt"), k


def _initializer(orbx, req):
    """the library's Initializer on a ref_init request, its current frame set and its sets drawn -> (it, iterations, n_per)"""
    r = rs.Records(req)
    seed, iterations, n_per = [int(x) for x in r.one("ipar").reshape(-1)]
    it = orbx.Initializer(r.one("keys1"), r.one("K").reshape(-1), float(r.one("sigma")[0, 0]), iterations, rand=sc.Lcg(seed), rand_max=sc.RAND_MAX)
    it.set_current(r.one("keys2"), r.one("m12").reshape(-1))
    it.draw()
    return it, iterations, min(n_per, iterations)


def _check_init_rows(name, score_M, cnt, masks, ref, N, iterations, n_per):
    """the rows of one problem of an orbm_init_hypotheses call (the H of every set, then the F) against the reference's per-set records"""
    assert len(score_M) == 2 * iterations and n_per > 0, name
    assert np.array_equal(ref["sets"][0].shape, (iterations, 8))
    for px, model in (("H", 0), ("F", 1)):
        rows = slice(model * iterations, model * iterations + n_per)
        bits = np.unpackbits(np.ascontiguousarray(masks[rows]).view(np.uint8).reshape(n_per, -1), axis=1, bitorder="little")
        want = np.unpackbits(ref[px + "inl"][0], axis=1, bitorder="little")[:, :N]
        assert np.array_equal(bits[:, :N], want) and not bits[:, N:].any(), (name, px)
        assert np.array_equal(cnt[rows], want.sum(1)), (name, px)
        assert rs.value_deviation("init_matrix", score_M[rows, 1:], ref[px + "s"][0]) <= rs.tol("init_matrix"), (name, px)
        assert rs.deviation(score_M[rows, 0], ref[px + "sc"][0]) <= rs.tol("init_score"), (name, px)


def test_init_mixed_batch_in_one_call(m, orbx):
    """N = 129, 8, 64, 63 and 8 again (five, one, two and two 32-bit mask words; both routes) in ONE orbm_init_hypotheses call"""
    names = ("general129", "plane8", "plane64", "few63", "general8")
    its = [_initializer(orbx, FIXTURES[("init", n)][0]) for n in names]
    for n, (it, iterations, n_per), (sm, cnt, masks) in zip(names, its, m.init_hypotheses([i[0] for i in its])):
        ref = rs.Records(FIXTURES[("init", n)][1]).by
        assert np.array_equal(it._get()[3], ref["sets"][0]), n
        _check_init_rows(n, sm, cnt, masks, ref, it.N, iterations, n_per)


def test_init_hypotheses_device_pointer_form(m, orbx):
    import torch
    name = "general65"
    it, iterations, n_per = _initializer(orbx, FIXTURES[("init", name)][0])
    off, uv, pn, params, hyp_off, sets, models, mask_off = orbx.ORBmatcher.pack_init_problems([it])
    H, MW = int(hyp_off[-1]), int(mask_off[-1])
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (off, uv, pn, np.ascontiguousarray(params.view(np.uint8).reshape(1, -1)), hyp_off, sets, models, mask_off)]
    d_sm, d_cnt, d_masks = _padded(torch, 10 * H, torch.float32, -77.0), _padded(torch, H, torch.int32), _padded(torch, MW, torch.int32)
    torch.cuda.synchronize()
    m.init_hypotheses_device(1, H, *d_in, d_sm[PAD:PAD + 10 * H], d_cnt[PAD:PAD + H], d_masks[PAD:PAD + MW])
    torch.cuda.synchronize()
    sm, cnt, masks = d_sm.cpu().numpy(), d_cnt.cpu().numpy(), d_masks.cpu().numpy()
    assert _guards_intact(sm, 10 * H) and _guards_intact(cnt, H) and _guards_intact(masks, MW)
    _check_init_rows(name, sm[PAD:PAD + 10 * H].reshape(H, 10), cnt[PAD:PAD + H], masks[PAD:PAD + MW].view(np.uint32).reshape(H, -1),
                     rs.Records(FIXTURES[("init", name)][1]).by, it.N, iterations, n_per)


def _route(ref):
    sh, sf = np.float32(ref["fHsc"][0].reshape(-1)[0]), np.float32(ref["fFsc"][0].reshape(-1)[0])
    return "H" if sh / (sh + sf) > 0.40 else "F"


def _check_rt_against_reference(name, ref, px, status, cosp, p3d, first, n1):
    """k_init_check_rt's outputs for the REFERENCE's own motions and inlier flags, reduced as CheckRT reduces its loop, against the
    reference's per-motion records: nGood and vbGood exactly, motion by motion in the reference's order"""
    good, vb, pts, par = rs.reduce_check_rt(status, cosp, p3d, first, n1)
    assert np.array_equal(good, ref[px + "good"][0].reshape(-1)), (name, good, ref[px + "good"][0])
    want_vb = ref[px + "vb"][0].astype(bool)
    assert np.array_equal(vb.astype(bool), want_vb), name
    k = len(good)
    got_p, want_p = pts.reshape(k, n1, 3), ref[px + "p3d"][0].reshape(k, n1, 3)
    assert rs.deviation(got_p[want_vb], want_p[want_vb]) <= rs.tol("init_p3d"), name
    assert rs.deviation(rs._cos_parallax(par), rs._cos_parallax(ref[px + "par"][0].reshape(-1))) <= rs.tol("init_parallax"), name


@pytest.mark.parametrize("name", ["plane65", "general129", "plane8", "few63"])
def test_check_rt_kernel_on_the_reference_motions(m, orbx, name):
    """8 motions (plane) and 4 (general): the kernel is given the motions and the inlier flags the reference recorded"""
    it, _, _ = _initializer(orbx, FIXTURES[("init", name)][0])
    ref = rs.Records(FIXTURES[("init", name)][1]).by
    px = _route(ref)
    Rt, inl = ref[px + "mot"][0], ref["f%sinl" % px][0].reshape(-1)
    assert len(Rt) == (8 if px == "H" else 4) and len(inl) == it.N
    uv, K4, th2 = it.check_rt_inputs()
    _check_rt_against_reference(name, ref, px, *m.init_check_rt(uv, inl, K4, th2, Rt), it.matches()[0], it.n1)


def test_init_check_rt_device_pointer_form(m, orbx):
    import torch
    name = "plane129"
    it, _, _ = _initializer(orbx, FIXTURES[("init", name)][0])
    ref = rs.Records(FIXTURES[("init", name)][1]).by
    px = _route(ref)
    Rt, inl = np.ascontiguousarray(ref[px + "mot"][0], np.float32), np.ascontiguousarray(ref["f%sinl" % px][0].reshape(-1), np.uint8)
    uv, K4, th2 = it.check_rt_inputs()
    n, k = it.N, len(Rt)
    dev = torch.device("cuda")
    d_uv, d_inl, d_Rt = (torch.from_numpy(np.array(a)).to(dev) for a in (uv, inl, Rt))
    d_st, d_cos, d_p3d = _padded(torch, k * n, torch.uint8, 77), _padded(torch, k * n, torch.float32, -77.0), _padded(torch, 3 * k * n, torch.float32, -77.0)
    torch.cuda.synchronize()
    m.init_check_rt_device(n, d_uv, d_inl, K4, th2, k, d_Rt, d_st[PAD:PAD + k * n], d_cos[PAD:PAD + k * n], d_p3d[PAD:PAD + 3 * k * n])
    torch.cuda.synchronize()
    st, cosp, p3d = d_st.cpu().numpy(), d_cos.cpu().numpy(), d_p3d.cpu().numpy()
    assert _guards_intact(st, k * n, 77) and _guards_intact(cosp, k * n) and _guards_intact(p3d, 3 * k * n)
    _check_rt_against_reference(name, ref, px, st[PAD:PAD + k * n].reshape(k, n), cosp[PAD:PAD + k * n].reshape(k, n),
                                p3d[PAD:PAD + 3 * k * n].reshape(k, n, 3), it.matches()[0], it.n1)
