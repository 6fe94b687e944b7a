"""GPU parity against the reference's own code: the HIP library (through the C ABI) == oracle/_ref/ref_orbx, the
reference's src/ORBextractor.cc compiled unmodified on the OpenCV shim, with no step through the oracle.  ref_orbx is
a CPU program that build() leaves under oracle/_ref/; these tests read nothing else of the reference."""
import os

import numpy as np
import pytest

import ref_pin as R

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


@pytest.fixture(scope="module", autouse=True)
def ref():
    if not (os.path.exists(R.EXE) and os.access(R.EXE, os.X_OK)):
        pytest.skip("oracle/_ref/ref_orbx was not built (build() compiles it where the reference tree is present)")
    return R.EXE


def _bits(a):
    return a.view(np.uint32) if a.dtype.kind == "f" else a


def _compare(kps, desc, rk, rd, tag):
    assert len(kps) == len(rk), "%s: count %d vs reference %d" % (tag, len(kps), len(rk))
    for f in FIELDS:
        bad = np.nonzero(_bits(kps[f]) != _bits(rk[f]))[0]
        assert bad.size == 0, "%s: field %s differs at %s: %s vs reference %s" % (tag, f, bad[:5], kps[f][bad[:5]], rk[f][bad[:5]])
    assert np.array_equal(desc, rd), "%s: descriptors differ in %d rows" % (tag, int((desc != rd).any(axis=1).sum()))


def _ref(img, nf=1000, sf=1.2, nl=8, ini=20, mn=7, blur=0):
    (out,) = R.run([R.Case(R.EXTRACT, (nf, sf, nl, ini, mn, blur), img)])
    return out


@pytest.mark.parametrize("W,H,n", [(640, 480, 1000), (1241, 376, 2000), (322, 241, 500)])
def test_extract_matches_reference(orbx, synth, W, H, n):
    img = synth.texture(1, W, H)
    ex = orbx.ORBextractor(n, 1.2, 8, 20, 7, max_width=W, max_height=H)
    kps, desc = ex(img)
    _compare(kps, desc, *_ref(img, n), tag="%dx%d" % (W, H))


def test_1080p_n4000(orbx, synth):
    f0, f1 = synth.frame_pair(2, 1920, 1080)
    ex = orbx.ORBextractor(4000, max_width=1920, max_height=1080)
    for tag, f in (("f0", f0), ("f1", f1)):
        kps, desc = ex(f)
        _compare(kps, desc, *_ref(f, 4000), tag="1080p " + tag)


@pytest.mark.parametrize("blur", [0, 1])
def test_1241x376_n2000_blur_modes(orbx, synth, blur):
    img = synth.texture(5, 1241, 376)
    ex = orbx.ORBextractor(2000, max_width=1241, max_height=376)
    ex.set_blur_rounding(blur)
    kps, desc = ex(img)
    _compare(kps, desc, *_ref(img, 2000, blur=blur), tag="blur %d" % blur)


@pytest.mark.parametrize("params", [
    dict(nfeatures=50, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7),
    dict(nfeatures=700, scaleFactor=1.5, nlevels=4, iniThFAST=30, minThFAST=10),
    dict(nfeatures=300, scaleFactor=2.0, nlevels=3, iniThFAST=20, minThFAST=7),
    dict(nfeatures=2000, scaleFactor=1.2, nlevels=8, iniThFAST=7, minThFAST=7),
    dict(nfeatures=500, scaleFactor=1.1, nlevels=12, iniThFAST=12, minThFAST=20),
    dict(nfeatures=1, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7),
])
def test_parameter_sweep_vs_reference(orbx, synth, params):
    W, H = 512, 384
    img = synth.texture(21, W, H)
    ex = orbx.ORBextractor(max_width=W, max_height=H, **params)
    kps, desc = ex(img)
    p = params
    assert not R.undefined_levels(W, H, p["scaleFactor"], p["nlevels"])
    _compare(kps, desc, *_ref(img, p["nfeatures"], p["scaleFactor"], p["nlevels"], p["iniThFAST"], p["minThFAST"]), tag=str(p))
    (t,) = R.run([R.Case(R.TABLES, (p["nfeatures"], p["scaleFactor"], p["nlevels"], 20, 7, 0))])
    assert np.array_equal(np.asarray(ex.GetScaleFactors(), np.float32).view(np.uint32), t["scale"].view(np.uint32))
    assert np.array_equal(np.asarray(ex.GetInverseScaleSigmaSquares(), np.float32).view(np.uint32), t["inv_sigma2"].view(np.uint32))


def test_saturated_noise_lattice(orbx):
    rng = np.random.default_rng(3)
    dots = np.full((240, 320), 255, np.uint8)
    dots[rng.integers(25, 215, 300), rng.integers(25, 295, 300)] = 0
    noise = rng.integers(0, 256, (240, 320), dtype=np.uint8)
    lattice = np.zeros((240, 320), np.uint8)
    lattice[::2, ::2] = rng.integers(60, 256, (120, 160), dtype=np.uint8)
    ex = orbx.ORBextractor(500, max_width=320, max_height=240)
    for tag, img in (("dots", dots), ("noise", noise), ("lattice", lattice)):
        kps, desc = ex(img)
        _compare(kps, desc, *_ref(img, 500), tag=tag)


def test_strided_input_is_an_isolated_image(orbx, synth):
    """An ROI (row stride > width) is processed as an image of its own; the reference is given the contiguous copy
    (its level-0 copyMakeBorder would read the parent's pixels around an ROI; its callers pass whole images)."""
    big = synth.texture(5, 700, 480)
    roi = big[:, 30:670]
    assert roi.strides[0] == 700
    ex = orbx.ORBextractor(500, max_width=640, max_height=480)
    kps, desc = ex(roi)
    _compare(kps, desc, *_ref(np.ascontiguousarray(roi), 500), tag="roi")


def test_batch64_vs_reference(orbx, synth):
    frames = synth.stream(4, 640, 480, 64)
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480, max_batch=64)
    res = ex.extract_batch(frames)
    refs = R.run_parallel([R.Case(R.EXTRACT, (1000, 1.2, 8, 20, 7, 0), f) for f in frames])
    for k in range(64):
        _compare(res[k][0], res[k][1], *refs[k], tag="frame %d" % k)


def test_bordered_pyramid_vs_reference(orbx, synth):
    W, H = 321, 243
    img = synth.texture(8, W, H)
    ex = orbx.ORBextractor(300, max_width=W, max_height=H)
    ex(img)
    (rp,) = R.run([R.Case(R.PYRAMID, (300, 1.2, 8, 20, 7, 0), img)])
    pyr = ex.image_pyramid_all(border=19)
    for l in range(8):
        assert pyr[l].shape == rp[l].shape, "level %d: %s vs reference %s" % (l, pyr[l].shape, rp[l].shape)
        assert np.array_equal(pyr[l], rp[l]), "level %d bytes differ" % l
