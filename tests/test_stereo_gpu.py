"""N3: Frame::ComputeStereoMatches on the GPU == oracle restatement (src/Frame.cc:466-640),
mvuRight / mvDepth compared as bit patterns."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _stereo_pair(synth, W, H, seed, disp):
    """Rectified pair: the right image sees the scene shifted left by `disp(x)` px (depth varies along x)."""
    canvas = synth.texture(seed, W + 128, H)
    left = canvas[:, 32:32 + W].copy()
    right = np.empty_like(left)
    for x0 in range(0, W, 160):          # piecewise-constant disparity: 6, 11, 16, ... px (capped at 36)
        d = min(disp + 5 * (x0 // 160), 36)
        wseg = min(160, W - x0)
        right[:, x0:x0 + wseg] = canvas[:, 32 + x0 + d:32 + x0 + d + wseg]
    noise = (synth.splitmix64(seed + 7, W * H) % np.uint64(5)).astype(np.int16).reshape(H, W) - 2
    right = np.clip(right.astype(np.int16) + noise, 0, 255).astype(np.uint8)
    return left, right


@pytest.mark.parametrize("W,H,n", [(640, 480, 1000), (1241, 376, 2000)])
def test_stereo_matches_equal_oracle(orbx, synth, W, H, n):
    left, right = _stereo_pair(synth, W, H, 31, 6)
    exL = orbx.ORBextractor(n, max_width=W, max_height=H)
    exR = orbx.ORBextractor(n, max_width=W, max_height=H)
    kl, dl = exL(left)
    kr, dr = exR(right)
    fx, bf = 500.0, 40.0 * 500.0 / 100.0      # mbf = baseline * fx; mb = mbf / fx
    mb = np.float32(bf) / np.float32(fx)
    u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, float(mb), float(bf))
    oex = O.Extractor(n)
    ou, od = O.stereo_matches(oex, kl, dl, kr, dr, oex.pyramid(left), oex.pyramid(right), float(mb), float(bf))
    assert np.array_equal(u.view(np.uint32), ou.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32))
    matched = u >= 0
    assert matched.sum() > 0.3 * len(kl)                       # the rig really matches
    disp = kl["x"][matched] - u[matched]
    assert (disp > 2).mean() > 0.9 and (disp < 40).all()


def test_stereo_no_right_keypoints(orbx, synth):
    left, right = _stereo_pair(synth, 320, 240, 5, 6)
    exL = orbx.ORBextractor(300, max_width=320, max_height=240)
    exR = orbx.ORBextractor(300, max_width=320, max_height=240)
    kl, dl = exL(left)
    exR(np.full((240, 320), 77, np.uint8))
    u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kl[:0], dl[:0], 0.08, 40.0)
    assert (u == -1).all() and (d == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# the edges: every hand-built case of tests/stereo_cases.py through the kernel (GPU == oracle, and the case's expectation)

import threading                                      # noqa: E402

import ref_pin as R                                   # noqa: E402  (level_dims / undefined_levels only: no reference is read)
import stereo_cases as S                              # noqa: E402
from stereo_cases import ACC_CASES, accuracy_scene, assert_bits, check_accuracy, oracle_run   # noqa: E402

HAND = S.hand_cases()
_handles = {}


def _pair_handles(orbx, sf, nl, W, H, nf=500):
    key = (sf, nl, W, H, nf)
    if key not in _handles:
        _handles[key] = (orbx.ORBextractor(nf, sf, nl, max_width=W, max_height=H),
                         orbx.ORBextractor(nf, sf, nl, max_width=W, max_height=H))
    return _handles[key]


def _oracle_scene(sf, nl, left, right, kl, dl, kr, dr, mb, mbf):
    ex = O.Extractor(500, sf, nl)
    return O.stereo_matches(ex, kl, dl, kr, dr, ex.pyramid(left), ex.pyramid(right), mb, mbf)


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_hand_case_gpu(orbx, case):
    H, W = case.left.shape
    exL, exR = _pair_handles(orbx, case.sf, case.nl, W, H)
    exL(case.left)
    exR(case.right)
    u, d = orbx.ComputeStereoMatches(exL, exR, case.kl, case.dl, case.kr, case.dr, case.mb, case.mbf)
    ou, od = oracle_run(case)
    assert_bits(u, ou, "mvuRight")
    assert_bits(d, od, "mvDepth")
    S.check_expectations(case, u, d)


# ---------------------------------------------------------------------------------------------------------------------
# randomised scenes over sizes, pyramids, feature counts and rigs

SIZES = [(640, 480), (1241, 376), (322, 241), (1920, 1080)]
SFS, NLS, NFS, FXS = [1.2, 1.5, 2.0], [1, 4, 8], [300, 1000, 4000], [500.0, 40.0, 2000.0]


def _fit(nf, sf, nl, most=1600):
    """nfeatures lowered until the largest level quota fits the library's LDS quadtree (orbx_create refuses more)."""
    while O.Extractor(nf, sf, nl).e.quota[0] > most:
        nf = nf * 3 // 4
    return nf


def _sweep_params():
    """sizes x scale factors x nlevels; nfeatures and rig cycle so that, for every size, each (nfeatures, fx) pair occurs;
    odd cases give the right handle other nfeatures / FAST thresholds.  nlevels is lowered where the reference's
    extractor is undefined (a level without a 30-px cell), nfeatures where one level's quota exceeds what a handle
    supports."""
    out = []
    for a, (W, H) in enumerate(SIZES):
        for b, sf in enumerate(SFS):
            for c, nl in enumerate(NLS):
                while nl > 1 and R.undefined_levels(W, H, sf, nl):
                    nl -= 1
                nf, fx = _fit(NFS[(a + b + c) % 3], sf, nl), FXS[(a + 2 * b + c) % 3]
                mixed = (a + b + c) % 2 == 1
                out.append(pytest.param(W, H, sf, nl, nf, fx, mixed,
                                        id="%dx%d-sf%g-nl%d-n%d-fx%g%s" % (W, H, sf, nl, nf, fx, "-mixed" if mixed else "")))
    return out


@pytest.mark.parametrize("W,H,sf,nl,nf,fx,mixed", _sweep_params())
def test_stereo_sweep(orbx, W, H, sf, nl, nf, fx, mixed):
    left, right, _ = S.stereo_scene(W * 31 + H + int(sf * 10) + nl, W, H)
    nfR, ini, mn = (_fit(nf * 2, sf, nl) if nf < 4000 else nf // 2, 12, 5) if mixed else (nf, 20, 7)
    if mixed and nfR == nf:
        nfR = nf // 2
    exL = orbx.ORBextractor(nf, sf, nl, max_width=W, max_height=H)
    exR = orbx.ORBextractor(nfR, sf, nl, ini, mn, max_width=W, max_height=H)
    kl, dl = exL(left)
    kr, dr = exR(right)
    mb, mbf = S.rig(fx)
    u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    ou, od = _oracle_scene(sf, nl, left, right, kl, dl, kr, dr, mb, mbf)
    assert_bits(u, ou, "mvuRight")
    assert_bits(d, od, "mvDepth")
    assert (u >= 0).sum() > 0.1 * len(kl)


def test_subset_and_permutation_of_right_keypoints(orbx):
    """The candidate scan is dense and ties go to the lowest index: a subset or a reordering of the right keypoints
    changes the result exactly as it changes the oracle's."""
    W, H = 640, 480
    left, right, _ = S.stereo_scene(77, W, H)
    exL, exR = _pair_handles(orbx, 1.2, 8, W, H, 1000)
    kl, dl = exL(left)
    kr, dr = exR(right)
    mb, mbf = S.rig(500.0)
    rng = np.random.default_rng(5)
    dr_tied = dr.copy()
    dr_tied[1::2] = dr[0::2][:len(dr[1::2])]         # many exact descriptor ties
    base = None
    for name, sel, desc in [("all", np.arange(len(kr)), dr), ("perm", rng.permutation(len(kr)), dr),
                            ("subset", np.sort(rng.choice(len(kr), len(kr) // 2, replace=False)), dr),
                            ("subset_perm", rng.choice(len(kr), len(kr) // 3, replace=False), dr),
                            ("reversed", np.arange(len(kr))[::-1], dr),
                            ("ties", np.arange(len(kr)), dr_tied), ("ties_reversed", np.arange(len(kr))[::-1], dr_tied)]:
        u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr[sel], desc[sel], mb, mbf)
        ou, od = _oracle_scene(1.2, 8, left, right, kl, dl, kr[sel], desc[sel], mb, mbf)
        assert_bits(u, ou, "mvuRight (%s)" % name)
        assert_bits(d, od, "mvDepth (%s)" % name)
        if name == "all":
            base = u
        elif name == "subset":
            assert not np.array_equal(u, base)


# ---------------------------------------------------------------------------------------------------------------------
# which pyramid a handle exposes, argument checks, threads, capacity

def _scene_kps(orbx, img, nf=1000, W=640, H=480):
    ex = orbx.ORBextractor(nf, max_width=W, max_height=H)
    return ex(img)


def test_extract_batch_exposes_frame0(orbx):
    W, H = 640, 480
    A, Ar, _ = S.stereo_scene(101, W, H)
    X, Y = S.stereo_scene(102, W, H)[0], S.stereo_scene(103, W, H)[1]
    exL = orbx.ORBextractor(1000, max_width=W, max_height=H, max_batch=3)
    exR = orbx.ORBextractor(1000, max_width=W, max_height=H)
    kl, dl = exL.extract_batch(np.stack([A, X, Y]))[0]
    kr, dr = exR(Ar)
    mb, mbf = S.rig(500.0)
    u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    ou, od = _oracle_scene(1.2, 8, A, Ar, kl, dl, kr, dr, mb, mbf)
    assert_bits(u, ou, "mvuRight")
    assert_bits(d, od, "mvDepth")
    assert (u >= 0).sum() > 0.3 * len(kl)


def test_extract_batch_device_exposes_frame0(orbx):
    import torch
    W, H, B = 640, 480, 2
    A, Ar, _ = S.stereo_scene(111, W, H)
    X = S.stereo_scene(112, W, H)[0]
    fr = torch.from_numpy(np.stack([A, X])).cuda()     # level 0 is read from this buffer: it stays alive and unchanged
    exL = orbx.ORBextractor(1000, max_width=W, max_height=H, max_batch=B)
    exR = orbx.ORBextractor(1000, max_width=W, max_height=H)
    cap = exL.cap
    k = torch.zeros((B, cap, 7), device="cuda"); dd = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    c = torch.zeros(B, dtype=torch.int32, device="cuda"); s = torch.zeros(B, dtype=torch.int32, device="cuda")
    exL.extract_batch_device(fr.data_ptr(), B, W, H, fr.stride(1), fr.stride(0), k.data_ptr(), dd.data_ptr(), c.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    n = int(c[0])
    kl = np.frombuffer(k[0, :n].cpu().numpy().tobytes(), O.KP_DTYPE).copy()
    dl = dd[0, :n].cpu().numpy()
    kr, dr = exR(Ar)
    mb, mbf = S.rig(500.0)
    u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    ou, od = _oracle_scene(1.2, 8, A, Ar, kl, dl, kr, dr, mb, mbf)
    assert_bits(u, ou, "mvuRight")
    assert_bits(d, od, "mvDepth")
    assert (u >= 0).sum() > 0.3 * len(kl)


def test_begin_end_equals_plain_call(orbx):
    W, H = 640, 480
    left, right, _ = S.stereo_scene(121, W, H)
    exL, exR = _pair_handles(orbx, 1.2, 8, W, H, 1000)
    mb, mbf = S.rig(500.0)
    kl, dl = exL(left)
    kr, dr = exR(right)
    u0, d0 = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    exL(right)                                          # something else in between
    exL.extract_begin(left)
    exR.extract_begin(right)
    kl1, dl1 = exL.extract_end()
    kr1, dr1 = exR.extract_end()
    assert kl1.tobytes() == kl.tobytes() and kr1.tobytes() == kr.tobytes()
    u1, d1 = orbx.ComputeStereoMatches(exL, exR, kl1, dl1, kr1, dr1, mb, mbf)
    assert_bits(u1, u0, "mvuRight")
    assert_bits(d1, d0, "mvDepth")


def test_shape_change_uses_the_new_shape(orbx):
    exL = orbx.ORBextractor(1000, max_width=640, max_height=480)
    exR = orbx.ORBextractor(1000, max_width=640, max_height=480)
    mb, mbf = S.rig(500.0)
    for (W, H), seed in [((640, 480), 131), ((322, 241), 132), ((640, 480), 133)]:
        left, right, _ = S.stereo_scene(seed, W, H)
        kl, dl = exL(left)
        kr, dr = exR(right)
        u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
        ou, od = _oracle_scene(1.2, 8, left, right, kl, dl, kr, dr, mb, mbf)
        assert_bits(u, ou, "mvuRight %dx%d" % (W, H))
        assert_bits(d, od, "mvDepth %dx%d" % (W, H))


def test_mismatched_handles_are_refused(orbx):
    left, right, _ = S.stereo_scene(141, 640, 480)
    exL = orbx.ORBextractor(1000, max_width=640, max_height=480)
    exR = orbx.ORBextractor(1000, max_width=640, max_height=480)
    kl, dl = exL(left)
    kr, dr = exR(right[:240, :320].copy())
    with pytest.raises(orbx.OrbxError) as e:
        orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, 0.08, 40.0)
    assert e.value.code == orbx.ORBX_E_SHAPE
    ex4 = orbx.ORBextractor(1000, 1.2, 4, max_width=640, max_height=480)
    kr, dr = ex4(right)
    with pytest.raises(orbx.OrbxError) as e:
        orbx.ComputeStereoMatches(exL, ex4, kl, dl, kr, dr, 0.08, 40.0)
    assert e.value.code == orbx.ORBX_E_INVALID


def test_empty_and_single_keypoint_sides(orbx):
    W, H = 640, 480
    left, right, _ = S.stereo_scene(151, W, H)
    exL, exR = _pair_handles(orbx, 1.2, 8, W, H, 1000)
    kl, dl = exL(left)
    kr, dr = exR(right)
    mb, mbf = S.rig(500.0)
    u, d = orbx.ComputeStereoMatches(exL, exR, kl[:0], dl[:0], kr, dr, mb, mbf)
    assert len(u) == 0 and len(d) == 0
    full, _ = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    i = int(np.nonzero(full >= 0)[0][0])                 # a left keypoint that matches
    for name, a, b in [("nr=0", (kl, dl), (kr[:0], dr[:0])), ("nl=1", (kl[i:i + 1], dl[i:i + 1]), (kr, dr)),
                       ("nr=1", (kl, dl), (kr[:1], dr[:1])), ("nl=nr=1", (kl[i:i + 1], dl[i:i + 1]), (kr[:1], dr[:1]))]:
        u, d = orbx.ComputeStereoMatches(exL, exR, a[0], a[1], b[0], b[1], mb, mbf)
        ou, od = _oracle_scene(1.2, 8, left, right, a[0], a[1], b[0], b[1], mb, mbf)
        assert_bits(u, ou, "mvuRight (%s)" % name)
        assert_bits(d, od, "mvDepth (%s)" % name)
        if name == "nr=0":
            assert (u == -1).all()
    u, d = orbx.ComputeStereoMatches(exL, exR, kl[i:i + 1], dl[i:i + 1], kr, dr, mb, mbf)
    assert u[0] >= 0                                      # a lone match is its own median and survives the cull


def test_two_rigs_on_two_threads(orbx):
    """Each thread extracts its own pair and matches it 20 times; both share the per-device stereo scratch."""
    rigs = [(640, 480, 161, 500.0), (1241, 376, 162, 40.0)]
    data = []
    for W, H, seed, fx in rigs:
        left, right, _ = S.stereo_scene(seed, W, H)
        data.append((left, right, S.rig(fx)))
    errors = []

    def work(t):
        try:
            left, right, (mb, mbf) = data[t]
            H, W = left.shape
            exL = orbx.ORBextractor(1000, max_width=W, max_height=H)
            exR = orbx.ORBextractor(1000, max_width=W, max_height=H)
            kl, dl = exL(left)
            kr, dr = exR(right)
            ou, od = want[t]
            for _ in range(20):
                u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
                if u.tobytes() != ou.tobytes() or d.tobytes() != od.tobytes():
                    errors.append("thread %d: result differs from the oracle" % t)
                    return
        except Exception as e:          # noqa: BLE001
            errors.append("thread %d: %r" % (t, e))

    want = []
    for left, right, (mb, mbf) in data:
        H, W = left.shape
        kl, dl = _scene_kps(orbx, left, W=W, H=H)
        kr, dr = _scene_kps(orbx, right, W=W, H=H)
        want.append(_oracle_scene(1.2, 8, left, right, kl, dl, kr, dr, mb, mbf))
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_right_keypoint_count_limit(orbx):
    """k_stereo packs dist << 22 | iR into 32 bits: 2^22 right keypoints are refused before anything runs, 2^22 - 1
    are matched (all of them candidates of one left keypoint, all at distance 0: the lowest index must win)."""
    W, H = 640, 480
    left, right, _ = S.stereo_scene(171, W, H)
    exL, exR = _pair_handles(orbx, 1.2, 8, W, H, 1000)
    exL(left)
    exR(right)
    kl = S.kps([(300.0, 240.0, 0)])
    dl = np.zeros((1, 32), np.uint8)
    n = 1 << 22
    kr = np.zeros(n, O.KP_DTYPE)
    kr["y"], kr["size"], kr["class_id"] = 240.0, 31.0, -1
    kr["x"] = (290.0 - (np.arange(n) % 40)).astype(np.float32)
    dr = np.zeros((n, 32), np.uint8)
    with pytest.raises(orbx.OrbxError) as e:
        orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, 0.08, 40.0)
    assert e.value.code == orbx.ORBX_E_CAPACITY
    u, d = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr[:n - 1], dr[:n - 1], 0.08, 40.0)
    ou, od = _oracle_scene(1.2, 8, left, right, kl, dl, kr[:n - 1], dr[:n - 1], 0.08, 40.0)
    assert_bits(u, ou, "mvuRight")
    assert_bits(d, od, "mvDepth")


@pytest.mark.parametrize("d,seed", ACC_CASES)
def test_accuracy_known_disparity_gpu(orbx, d, seed):
    ex, left, right, kl, dl, kr, dr = accuracy_scene(d, seed)
    exL, exR = _pair_handles(orbx, 1.2, 8, 640, 480, 1000)
    gkl, gdl = exL(left)
    gkr, gdr = exR(right)
    assert gkl.tobytes() == kl.tobytes() and gkr.tobytes() == kr.tobytes()
    mb, mbf = S.rig(500.0)
    u, depth = orbx.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    ou, od = O.stereo_matches(ex, kl, dl, kr, dr, ex.pyramid(left), ex.pyramid(right), mb, mbf)
    assert_bits(u, ou, "mvuRight")
    assert_bits(depth, od, "mvDepth")
    check_accuracy(ex, kl, u, depth, d, mbf)
