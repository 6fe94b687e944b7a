"""The oracle's oro_stereo_matches against the reference's own Frame::ComputeStereoMatches (src/Frame.cc:466-640): the
function's text is sliced out of Frame.cc at build time and compiled on the OpenCV shim inside a minimal Frame
(oracle/ref/ref_stereo.cc -> oracle/_ref/ref_stereo).  Both sides get the same pyramids (the oracle's, pinned to the
reference's ComputePyramid by tests/test_reference_pin_cpu.py), scale tables, keypoints and descriptors; mvuRight and
mvDepth are compared as bit patterns: every hand-built case of tests/stereo_cases.py, a sweep of randomised rigs and
scenes, and the same cases once more through the UBSan build."""
import os
import struct
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import ref_pin as R
import stereo_cases as S

EXE = os.path.join(R.REF_OUT, "ref_stereo")
EXE_UBSAN = os.path.join(R.REF_OUT, "ref_stereo_ubsan")
SWEEP_CASES = 280


@pytest.fixture(scope="module", autouse=True)
def ref():
    if not (os.path.exists(EXE) and os.path.exists(EXE_UBSAN)):
        if not os.path.exists(os.path.join(R.reference_dir(), "src", "Frame.cc")):
            pytest.skip("oracle/_ref/ref_stereo is not built and the reference tree is not present to build it from")
        subprocess.check_call(["make", "-s", "-C", os.path.join(R.ROOT, "oracle", "ref"), "stereo"])
    return EXE


class Pin:
    """One ref_stereo request (format in oracle/ref/ref_stereo.cc) and the oracle's answer to the same input."""

    def __init__(self, tag, sf, nl, left, right, kl, dl, kr, dr, mb, mbf):
        ex = O.Extractor(500, sf, nl)
        pl, pr = ex.pyramid(left), ex.pyramid(right)
        kl, kr = np.ascontiguousarray(kl, O.KP_DTYPE), np.ascontiguousarray(kr, O.KP_DTYPE)
        dl, dr = np.ascontiguousarray(dl, np.uint8), np.ascontiguousarray(dr, np.uint8)
        assert len(kl) > 0
        sc = np.array(list(ex.e.scale)[:nl], np.float32)
        isc = np.array(list(ex.e.inv_scale)[:nl], np.float32)
        b = [struct.pack("<iff", nl, mb, mbf), sc.tobytes(), isc.tobytes()]
        for lv in pl + pr:
            b += [struct.pack("<ii", lv.shape[1], lv.shape[0]), np.ascontiguousarray(lv).tobytes()]
        b += [struct.pack("<i", len(kl)), kl.tobytes(), dl.tobytes(), struct.pack("<i", len(kr)), kr.tobytes(), dr.tobytes()]
        self.tag, self.n, self.blob = tag, len(kl), b"".join(b)
        self.oracle = O.stereo_matches(ex, kl, dl, kr, dr, pl, pr, mb, mbf)


def run(pins, exe=EXE):
    with tempfile.TemporaryDirectory(prefix="ref_stereo_") as d:
        req, resp = os.path.join(d, "req.bin"), os.path.join(d, "resp.bin")
        with open(req, "wb") as f:
            f.write(struct.pack("<ii", 0x51525453, len(pins)))
            for p in pins:
                f.write(p.blob)
        p = subprocess.run([exe, req, resp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise subprocess.CalledProcessError(p.returncode, [exe], p.stdout, p.stderr)
        data = open(resp, "rb").read()
    assert struct.unpack("<i", data[:4])[0] == 0x52525453
    out, o = [], 4
    for p in pins:
        u = np.frombuffer(data[o:o + 4 * p.n], np.float32).copy(); o += 4 * p.n
        d = np.frombuffer(data[o:o + 4 * p.n], np.float32).copy(); o += 4 * p.n
        out.append((u, d))
    assert o == len(data), "trailing bytes in the ref_stereo response"
    return out


def run_parallel(pins, exe=EXE, procs=None):
    procs = procs or max(1, min(R.MAX_PROCS, os.cpu_count() or 1, len(pins)))
    parts = [pins[i::procs] for i in range(procs)]
    with ThreadPoolExecutor(procs) as pool:
        res = list(pool.map(lambda ps: run(ps, exe), parts))
    out = [None] * len(pins)
    for i in range(procs):
        out[i::procs] = res[i]
    return out


def assert_same(pin, got):
    (u, d), (ou, od) = got, pin.oracle
    for name, a, b in (("mvuRight", u, ou), ("mvDepth", d, od)):
        bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
        assert bad.size == 0, "%s: %s differs at %s: %s (reference) vs %s (oracle)" % (pin.tag, name, bad[:8], a[bad[:8]], b[bad[:8]])


@pytest.fixture(scope="module")
def hand():
    return [Pin(c.name, c.sf, c.nl, c.left, c.right, c.kl, c.dl, c.kr, c.dr, c.mb, c.mbf) for c in S.hand_cases()]


def _sweep_pin(i):
    """Randomised rig and scene: size, pyramid, feature counts and FAST thresholds of both sides, baseline and fx (maxD
    from 20 px to 2000 px), the scene's disparity range, and sometimes a shuffled subset of the right keypoints."""
    rng = np.random.default_rng(7000 + i)
    W, H = int(rng.integers(120, 720)), int(rng.integers(100, 520))
    sf = float(rng.choice([1.1, 1.2, 1.2, 1.5, 2.0]))
    nl = int(rng.integers(1, 9))
    while nl > 1 and R.undefined_levels(W, H, sf, nl):
        nl -= 1
    if R.undefined_levels(W, H, sf, nl):
        return None
    left, right, _ = S.stereo_scene(int(rng.integers(1, 1 << 30)), W, H, max_disp=int(rng.integers(4, 60)),
                                    noise=int(rng.integers(0, 4)))
    nfL, nfR = int(rng.choice([50, 300, 1000, 2000])), int(rng.choice([50, 300, 1000, 2000]))
    kl, dl, _ = O.Extractor(nfL, sf, nl).extract(left)
    kr, dr, _ = O.Extractor(nfR, sf, nl, int(rng.integers(8, 30)), int(rng.integers(3, 8))).extract(right)
    if len(kl) == 0:
        return None
    if len(kr) and rng.random() < 0.3:
        sel = rng.choice(len(kr), int(rng.integers(1, len(kr) + 1)), replace=False)
        kr, dr = kr[sel], dr[sel]
    mb, mbf = S.rig(float(rng.choice([20.0, 40.0, 300.0, 500.0, 718.0, 2000.0])), float(rng.uniform(0.05, 0.6)))
    pin = Pin("sweep %d: %dx%d sf=%g nl=%d n=%d/%d" % (i, W, H, sf, nl, len(kl), len(kr)), sf, nl, left, right,
              kl, dl, kr, dr, mb, mbf)
    # the reference reads the median of vDistIdx unchecked (:627): a scene where nothing passes the disparity test is outside
    # its domain.  A match that survives the cull proves one passed.
    return pin if (pin.oracle[0] >= 0).any() else None


@pytest.fixture(scope="module")
def sweep():
    with ThreadPoolExecutor(min(R.MAX_PROCS, os.cpu_count() or 1)) as pool:
        pins = [p for p in pool.map(_sweep_pin, range(SWEEP_CASES)) if p is not None]
    return pins


def test_hand_cases_equal_the_reference(hand):
    for pin, got in zip(hand, run(hand)):
        assert_same(pin, got)


def test_random_sweep_equals_the_reference(sweep):
    print("\n%d of %d random rigs inside the reference's domain" % (len(sweep), SWEEP_CASES))
    assert len(sweep) >= 200
    matched = 0
    for pin, got in zip(sweep, run_parallel(sweep)):
        assert_same(pin, got)
        matched += int((got[0] >= 0).sum())
    assert matched > 10000


def test_compared_cases_are_defined_behaviour_under_ubsan(hand, sweep):
    """The compared cases once through the UBSan build (-fno-sanitize-recover: the first undefined operation ends the
    process with an error), which must also give the same answers."""
    pins = hand + sweep
    try:
        out = run_parallel(pins, exe=EXE_UBSAN)
    except subprocess.CalledProcessError as e:
        pytest.fail("ref_stereo_ubsan exit %s:\n%s" % (e.returncode, e.stderr[-2000:]))
    for pin, got in zip(pins, out):
        assert_same(pin, got)
