"""The batched MapPoint::ComputeDistinctiveDescriptors on the MI355X (orbm_distinctive_descriptors, include/orbm.h) against
the restatement tests/mappoint_oracle.py.  Integer arithmetic only, so every comparison is exact: == on both int32 outputs.
Every test here needs the symbol, so all of them fail on a library built without my-slam_amd/csrc/orbm_mappoint.hip."""
import os
import subprocess

import numpy as np
import pytest

import mappoint_oracle as MO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# size-class boundaries of my-slam_amd/csrc/orbm_mappoint.hip (DD_SMALL_MAX, DD_WAVE_MAX, DD_WG_MAX); 2 is the last N answered
# without arithmetic
NO_ARITHMETIC_MAX = 2
SMALL_MAX = 16
WAVE_MAX = 64
WG_MAX = 256
BOUNDARIES = (NO_ARITHMETIC_MAX, SMALL_MAX, WAVE_MAX, WG_MAX)


def test_boundaries_mirror_the_kernel_file():
    text = open(os.path.join(ROOT, "my-slam_amd", "csrc", "orbm_mappoint.hip")).read()
    for name, v in (("DD_SMALL_MAX", SMALL_MAX), ("DD_WAVE_MAX", WAVE_MAX), ("DD_WG_MAX", WG_MAX)):
        assert "#define %s %d\n" % (name, v) in text


def check(m, off, desc):
    best, med = m.distinctive_descriptors(off, desc)
    eb, em = MO.distinctive_descriptors(off, desc)
    assert best.dtype == np.int32 and med.dtype == np.int32
    bad = np.nonzero((best != eb) | (med != em))[0]
    assert len(bad) == 0, "points %s (N = %s): got %s / %s, expected %s / %s" % (
        bad[:8], np.diff(off)[bad[:8]], best[bad[:8]], med[bad[:8]], eb[bad[:8]], em[bad[:8]])
    assert np.array_equal(best, eb) and np.array_equal(med, em)
    return best, med


@pytest.fixture()
def matcher(orbx):
    m = orbx.ORBmatcher()
    yield m
    m.close()


@pytest.mark.parametrize("flips", [6, None], ids=["bit-flips", "uniform"])
def test_key_frame_shaped_batch(matcher, flips):
    rng = np.random.default_rng(11 if flips else 12)
    lengths = MO.run_lengths_keyframe(rng, 2000)
    assert lengths.max() > WAVE_MAX and np.median(lengths) < SMALL_MAX
    off, desc = MO.batch_from_lengths(rng, lengths, flips=flips)
    best, med = check(matcher, off, desc)
    if flips:
        assert med.max() <= 2 * flips and (best > 0).sum() > 200      # small distances, and the first row is not the usual answer
    else:
        assert med[lengths > 8].min() > 80


@pytest.mark.parametrize("B", BOUNDARIES)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tier_edge_alone(matcher, B, delta):
    rng = np.random.default_rng(100 * B + delta + 1)
    for flips in (4, None):
        off, desc = MO.batch_from_lengths(rng, np.array([B + delta]), flips=flips)
        check(matcher, off, desc)


def test_tier_edges_mixed_into_one_batch(matcher):
    rng = np.random.default_rng(21)
    edges = [B + d for B in BOUNDARIES for d in (-1, 0, 1)]
    lengths = np.array(edges + [0] + list(rng.integers(0, 20, 40)) + edges[::-1] + [700, 5, 300])
    rng.shuffle(lengths)
    for flips in (5, None):
        off, desc = MO.batch_from_lengths(rng, lengths, flips=flips)
        check(matcher, off, desc)


def test_large_runs_beyond_the_tiers(matcher):
    """The reference's float Distances[N][N] on the stack dies near N = 1400; the library must not care."""
    rng = np.random.default_rng(31)
    lengths = np.array([3, 1600, 0, 257, 9, 513, 2])             # 1600: rows blocks shared with both neighbours' rows
    off, desc = MO.batch_from_lengths(rng, lengths, flips=8)
    check(matcher, off, desc)
    off, desc = MO.batch_from_lengths(rng, np.array([1500]), flips=None)
    check(matcher, off, desc)
    # a tie across row blocks: rows 0..299 and 300..599 are two copies of the same rows, so the first copy must win
    half = MO.batch_from_lengths(rng, np.array([300]), flips=3)[1]
    off = np.array([0, 600], np.int32)
    best, med = check(matcher, off, np.concatenate([half, half]))
    assert best[0] < 300


def test_empty_runs_and_tiny_batches(matcher):
    rng = np.random.default_rng(41)
    off, desc = MO.batch_from_lengths(rng, np.array([0, 5, 0, 0, 33, 0]))
    best, med = check(matcher, off, desc)
    assert list(best[[0, 2, 3, 5]]) == [-1] * 4 and list(med[[0, 2, 3, 5]]) == [-1] * 4
    off, desc = MO.batch_from_lengths(rng, np.array([7]))         # M = 1
    check(matcher, off, desc)
    off, desc = MO.batch_from_lengths(rng, np.zeros(9, np.int64))  # only empty runs
    best, med = check(matcher, off, desc)
    assert (best == -1).all() and (med == -1).all()
    best, med = matcher.distinctive_descriptors(np.zeros(1, np.int32), np.zeros((0, 32), np.uint8))   # M = 0
    assert len(best) == 0 and len(med) == 0


def test_handle_state_small_large_small(orbx, synth):
    """One handle: a grid search, then small -> large (the call's scratch grows) -> small batches, then the same grid search.
    The search must give what it gave before unless orbm_grid_count() reports that the grid was dropped."""
    rng = np.random.default_rng(51)
    n = 1500
    kps = np.zeros(n, orbx.KP_DTYPE)
    kps["x"] = rng.uniform(0, 640, n).astype(np.float32); kps["y"] = rng.uniform(0, 480, n).astype(np.float32)
    kps["octave"] = rng.integers(0, 8, n)
    train = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q = train[rng.integers(0, n, 300)].copy()
    x = rng.uniform(0, 640, 300).astype(np.float32); y = rng.uniform(0, 480, 300).astype(np.float32)
    m = orbx.ORBmatcher(max_queries=2048, max_train=2048, max_pairs=1 << 16)
    m.grid_build(kps, 0.0, 640.0, 0.0, 480.0)
    assert m.grid_count() == n
    before = m.search_area_best2(q, x, y, 60.0, 0, 7, train)
    assert (before[0] >= 0).sum() > 100
    small = MO.batch_from_lengths(rng, rng.integers(0, 12, 50))
    large = MO.batch_from_lengths(rng, MO.run_lengths_keyframe(rng, 6000))       # ~60 000 rows: far beyond the handle's 2048
    small2 = MO.batch_from_lengths(rng, rng.integers(0, 30, 80), flips=None)
    for off, desc in (small, large, small2, small):
        check(m, off, desc)
        if m.grid_count() == -1:
            m.grid_build(kps, 0.0, 640.0, 0.0, 480.0)
        else:
            assert m.grid_count() == n
        after = m.search_area_best2(q, x, y, 60.0, 0, 7, train)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
    m.close()


def test_device_entry_point_on_a_callers_stream(orbx):
    import torch
    rng = np.random.default_rng(61)
    lengths = np.concatenate([MO.run_lengths_keyframe(rng, 1500), [0, 300, 1, 700, 2, 64, 65]])
    off, desc = MO.batch_from_lengths(rng, lengths)
    m = orbx.ORBmatcher()
    hb, hm = m.distinctive_descriptors(off, desc)
    d_off, d_desc = torch.from_numpy(off).cuda(), torch.from_numpy(desc).cuda()
    d_best = torch.full((len(lengths),), -7, dtype=torch.int32, device="cuda")
    d_med = torch.full((len(lengths),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        m.distinctive_descriptors_device(len(lengths), d_off.data_ptr(), d_desc.data_ptr(), int(off[-1]), int(lengths.max()),
                                         d_best.data_ptr(), d_med.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_best.cpu().numpy(), hb) and np.array_equal(d_med.cpu().numpy(), hm)
    # best_median may be NULL, the handle's own stream serves when none is given
    d_best.fill_(-7)
    torch.cuda.synchronize()
    m.distinctive_descriptors_device(len(lengths), d_off.data_ptr(), d_desc.data_ptr(), int(off[-1]), int(lengths.max()), d_best.data_ptr())
    m.distinctive_descriptors(off[:2], desc[:off[1]])            # a host call on the same handle synchronises its stream
    torch.cuda.synchronize()
    assert np.array_equal(d_best.cpu().numpy(), hb)
    eb, em = MO.distinctive_descriptors(off, desc)
    assert np.array_equal(hb, eb) and np.array_equal(hm, em)
    m.close()


def _hex(rows):
    return np.ascontiguousarray(rows, np.uint8).tobytes().hex()


def test_cxx_caller_sets_the_row_the_restatement_picks(orbx, tmp_path):
    """tests/cxx/mappoint_callsites.cc: after the batched call every point's GetDescriptor() is the row the restatement picks
    from its observations in map order; NULL, bad and unobserved points and points whose key frames are all bad keep theirs."""
    exe = str(tmp_path / "mappoint_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "mappoint_shims"),
           "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [os.path.join(ROOT, "tests", "cxx", "mappoint_callsites.cc"), "-o", exe, "-L" + libdir, "-lorbx",
                           "-Wl,-rpath," + libdir])
    rng = np.random.default_rng(71)
    K, rows = 120, 400
    bad_kf = rng.random(K) < 0.1
    bad_kf[:3] = [True, True, False]
    base = rng.integers(0, 256, (rows, 32), dtype=np.uint8)       # feature idx of every key frame = a noisy copy of base[idx]
    kf_desc = np.repeat(base[None], K, axis=0)
    noise = rng.integers(0, 256 * 32 * 8, (K, rows, 5))
    for f in range(5):
        byte, bit = (noise[:, :, f] >> 3) % 32, noise[:, :, f] & 7
        np.bitwise_xor.at(kf_desc, (np.arange(K)[:, None], np.arange(rows)[None, :], byte), (1 << bit).astype(np.uint8))
    script = ["kfs %d" % K] + ["kf %d %d %s" % (bad_kf[k], rows, _hex(kf_desc[k])) for k in range(K)]
    slots = []                                                    # per slot: None, or (old descriptor, expected descriptor)
    lengths = list(MO.run_lengths_keyframe(rng, 300, tail=(17, K))) + [0, 0, 1, 2, K]
    for i, n_obs in enumerate(lengths):
        if i % 37 == 5:
            script.append("null"); slots.append(None)
        old = rng.integers(0, 256, 32, dtype=np.uint8)
        kfs = np.sort(rng.choice(K, int(n_obs), replace=False))   # map order = ascending KeyFrame* = ascending id (one array)
        if i == 7:
            kfs = np.array([0, 1])                                # only bad key frames
        idx = int(rng.integers(0, rows))
        bad = i % 29 == 3
        script.append("mp %d %s %d %s" % (bad, _hex(old), len(kfs), " ".join("%d %d" % (k, idx) for k in rng.permutation(kfs))))
        D = np.array([kf_desc[k, idx] for k in kfs if not bad_kf[k]], np.uint8).reshape(-1, 32)
        b, _ = MO.distinctive_descriptor(D)
        slots.append((old, old if (bad or b < 0) else D[b]))
    script += ["batch", "dump"]
    p = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = p.stdout.split("\n")
    changed = sum(1 for s in slots if s is not None and not np.array_equal(s[0], s[1]))
    assert out[0] == "set %d" % changed and changed > 250
    kept = 0
    for s, line in zip(slots, out[1:]):
        if s is None:
            assert line == "null"
        else:
            assert line == _hex(s[1])
            kept += np.array_equal(s[0], s[1])
    assert kept >= 10                                             # bad, unobserved and all-bad-key-frame points were in the list
    # the rewritten single-point method gives the same descriptor as the batch did
    first = next(i for i, s in enumerate(slots) if s is not None and not np.array_equal(s[0], s[1]))
    p = subprocess.run([exe], input="\n".join(script[:-2] + ["single %d" % first, "dump"]) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.split("\n")
    assert lines[first] == _hex(slots[first][1])
    assert sum(1 for s, line in zip(slots, lines) if s is not None and line != _hex(s[0])) == 1
