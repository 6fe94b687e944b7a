"""No-GPU checks of the batched MapPoint::ComputeDistinctiveDescriptors (include/orbm.h, orbm_distinctive_descriptors):
hand-worked cases of the restatement tests/mappoint_oracle.py with the expected index AND median written out; both exports;
the argument checks made before any device work; the all-N<=2 batch that needs no device; the loud failure of everything
else without a GPU; and the C++ adapter compiling the reference's call expressions.

The hand-worked descriptors lie on a line: L(x) has its first x bits set, so DescriptorDistance(L(x), L(y)) = |x - y|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mappoint_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def L(x):
    bits = np.zeros(256, np.uint8)
    bits[:x] = 1
    return np.packbits(bits)


def line(*xs):
    return np.stack([L(x) for x in xs])


def test_line_descriptors_have_the_distances_the_cases_assume():
    assert MO.descriptor_distance(L(0), L(256)) == 256
    assert MO.descriptor_distance(L(7), L(40)) == 33
    assert MO.descriptor_distance(L(13), L(13)) == 0


# ---- the restatement, one case per point of the contract

def test_empty_run_keeps_the_descriptor():
    assert MO.distinctive_descriptor(np.zeros((0, 32), np.uint8)) == (-1, -1)


def test_one_observation():
    assert MO.distinctive_descriptor(line(5)) == (0, 0)


def test_two_observations_always_take_the_first():
    # k = int(0.5 * 1) = 0: both rows' element 0 is the own 0, and 0 < 0 is false for the second
    assert MO.distinctive_descriptor(line(0, 100)) == (0, 0)
    assert MO.distinctive_descriptor(line(100, 0)) == (0, 0)


def test_three_observations_take_the_row_whose_nearer_neighbour_is_nearest():
    # rows sorted: [0 10 13], [0 3 10], [0 3 13]; k = 1: medians 10, 3, 3 -> the first 3 is row 1
    assert MO.distinctive_descriptor(line(0, 10, 13)) == (1, 3)
    # [0 20 25], [0 20 45], [0 25 45]: medians 20, 20, 25
    assert MO.distinctive_descriptor(line(20, 0, 45)) == (0, 20)


def test_four_observations_take_the_lower_middle():
    # rows sorted: [0 4 10 11], [0 4 6 7], [0 1 6 10], [0 1 7 11]; k = int(1.5) = 1: medians 4, 4, 1, 1 -> (2, 1).
    # The upper middle (k = 2) would give 10, 6, 6, 7 -> (1, 6)
    assert MO.distinctive_descriptor(line(0, 4, 10, 11)) == (2, 1)


def test_five_observations():
    # rows sorted: [0 2 5 9 20], [0 2 3 7 18], [0 3 4 5 15], [0 4 7 9 11], [0 11 15 18 20]; k = 2: medians 5, 3, 4, 7, 15
    assert MO.distinctive_descriptor(line(0, 2, 5, 9, 20)) == (1, 3)


def test_a_tie_goes_to_the_first_row():
    # rows sorted: [0 5 10 15], [0 5 5 10], [0 5 5 10], [0 5 10 15]; k = 1: every median is 5
    assert MO.distinctive_descriptor(line(0, 5, 10, 15)) == (0, 5)
    # medians 33, 0, 0: the tie is between rows 1 and 2
    assert MO.distinctive_descriptor(line(40, 7, 7)) == (1, 0)


def test_duplicate_descriptors_give_zero_entries():
    # rows sorted: [0 0 0 33] x 3, [0 33 33 33]; k = 1: medians 0, 0, 0, 33
    assert MO.distinctive_descriptor(line(7, 7, 7, 40)) == (0, 0)


def test_reversing_the_input_changes_the_answer():
    D = line(0, 5, 10, 15)
    i, m = MO.distinctive_descriptor(D)
    j, n = MO.distinctive_descriptor(D[::-1])
    assert (i, m) == (0, 5) and (j, n) == (0, 5)
    assert not np.array_equal(D[i], D[::-1][j])                 # the same index is another observation's descriptor


def test_batch_form_matches_the_single_point_form():
    rng = np.random.default_rng(5)
    lengths = np.array([0, 1, 2, 3, 7, 0, 20])
    off, desc = MO.batch_from_lengths(rng, lengths)
    best, med = MO.distinctive_descriptors(off, desc)
    assert best.dtype == np.int32 and med.dtype == np.int32
    for p in range(len(lengths)):
        assert (best[p], med[p]) == MO.distinctive_descriptor(desc[off[p]:off[p + 1]])
    assert list(best[:3]) == [-1, 0, 0] and list(med[:3]) == [-1, 0, 0] and best[5] == -1


def test_generators_give_the_shapes_the_gpu_tests_ask_for():
    rng = np.random.default_rng(1)
    n = MO.run_lengths_keyframe(rng, 2000)
    assert ((n >= 2) & (n <= 15)).mean() > 0.9 and n.max() > 100 and n.max() <= 400
    off, desc = MO.batch_from_lengths(rng, n)
    assert off[-1] == len(desc) == n.sum()
    d = [MO.descriptor_distance(desc[off[p]], desc[off[p] + 1]) for p in range(50)]
    assert max(d) <= 12                                         # at most 6 flips per row
    off, desc = MO.batch_from_lengths(rng, n, flips=None)
    d = [MO.descriptor_distance(desc[off[p]], desc[off[p] + 1]) for p in range(50)]
    assert 90 < np.mean(d) < 166


# ---- the library without a GPU

@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_both_symbols_are_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    assert hasattr(lib, "orbm_distinctive_descriptors") and hasattr(lib, "orbm_distinctive_descriptors_device")
    assert hasattr(built.ORBmatcher, "distinctive_descriptors") and hasattr(built.ORBmatcher, "distinctive_descriptors_device")


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument still gets ORBX_E_INVALID and a text: the
    checks run before the handle or the device is looked at."""
    Lb = built.lib()
    E = built.ORBX_E_INVALID
    f = Lb.orbm_distinctive_descriptors
    off = np.array([0, 3], np.int32); desc = np.zeros((3, 32), np.uint8); best = np.zeros(1, np.int32); med = np.zeros(1, np.int32)
    assert f(None, -1, p(off), p(desc), p(best), p(med)) == E and b"n_points" in Lb.orbm_last_error()
    assert f(None, 1, None, p(desc), p(best), p(med)) == E and b"NULL" in Lb.orbm_last_error()
    assert f(None, 1, p(off), p(desc), None, p(med)) == E
    assert f(None, 1, p(off), None, p(best), p(med)) == E and b"desc" in Lb.orbm_last_error()
    bad0 = np.array([1, 3], np.int32)
    assert f(None, 1, p(bad0), p(desc), p(best), p(med)) == E and b"off[0]" in Lb.orbm_last_error()
    down = np.array([0, 3, 2], np.int32)
    assert f(None, 2, p(down), p(desc), p(best), p(med)) == E and b"monotone" in Lb.orbm_last_error()
    assert f(None, 0, None, None, None, None) == built.ORBX_OK
    g = Lb.orbm_distinctive_descriptors_device
    assert g(None, -1, None, None, 0, 0, None, None, None) == E
    assert g(None, 1, None, None, 3, 3, None, None, None) == E
    assert g(None, 1, p(off), p(desc), 3, 4, p(best), None, None) == E          # max_run > total_rows
    assert g(None, 0, None, None, 0, 0, None, None, None) == built.ORBX_OK


def test_a_batch_of_short_runs_needs_no_device(built):
    """Freshly made points (N <= 2, and an empty run): answered on the host, wherever the library runs."""
    Lb = built.lib()
    rng = np.random.default_rng(2)
    lengths = np.array([2, 1, 0, 2, 2, 1, 0])
    off, desc = MO.batch_from_lengths(rng, lengths)
    best = np.full(len(lengths), 77, np.int32); med = np.full(len(lengths), 77, np.int32)
    assert Lb.orbm_distinctive_descriptors(None, len(lengths), p(off), p(desc), p(best), p(med)) == built.ORBX_OK
    eb, em = MO.distinctive_descriptors(off, desc)
    assert np.array_equal(best, eb) and np.array_equal(med, em)
    assert list(best) == [0, 0, -1, 0, 0, 0, -1]
    best[:] = 77
    assert Lb.orbm_distinctive_descriptors(None, len(lengths), p(off), p(desc), p(best), None) == built.ORBX_OK    # best_median may be NULL
    assert np.array_equal(best, eb)


def test_one_run_of_three_fails_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    rng = np.random.default_rng(3)
    off, desc = MO.batch_from_lengths(rng, np.array([2, 3, 1]))
    best = np.full(3, 77, np.int32); med = np.full(3, 77, np.int32)
    assert Lb.orbm_distinctive_descriptors(None, 3, p(off), p(desc), p(best), p(med)) == built.ORBX_E_HIP
    assert b"no CPU path" in Lb.orbm_last_error()
    assert list(best) == [77, 77, 77]                           # no half answer
    d = np.zeros(4, np.int32)
    assert Lb.orbm_distinctive_descriptors_device(None, 3, p(off), p(desc), 6, 3, p(d), None, None) == built.ORBX_E_HIP
    with pytest.raises(built.OrbxError) as ei:
        built.ORBmatcher()
    assert ei.value.code == built.ORBX_E_HIP


def test_adapter_compiles_the_reference_call_expressions(built, tmp_path):
    exe = str(tmp_path / "mappoint_callsites")
    libdir = os.path.dirname(built.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "mappoint_shims"),
           "-I" + os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "cxx", "mappoint_callsites.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [src, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    text = open(src).read()
    for expr in ("const vector<MapPoint*> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();", "if(!pMP->isBad())",
                 "pMP->ComputeDistinctiveDescriptors();", "ComputeDistinctiveDescriptors(vpMapPointMatches"):
        assert expr in text
    assert subprocess.run([exe, "compile-only"]).returncode == 0
