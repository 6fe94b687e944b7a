"""No-GPU checks of the keyframe database (include/orbk.h): hand-worked cases of the restatement tests/kfdb_oracle.py, one per
point of the reference's behaviour, with the expected lists written out; the orbk_ exports; the argument checks made before
any device work; the loud failure without a GPU; and the C++ adapter compiling the reference's call expressions.

Values are dyadic, so every L1 score is exact: for positive values the term of a common word is -2 * min(v, w) and the score
is the sum of min(v, w) over the common words."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kfdb_oracle as K
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bow(d):
    ks = sorted(d)
    return np.array(ks, np.int32), np.array([d[k] for k in ks], np.float64)


def db_with(kfs, nwords=100):
    db = K.KeyFrameDatabase(nwords)
    for kid, d in kfs:
        db.add(kid, bow(d))
    return db


# ---- the restatement, one case per point of the contract

def test_encounter_order_is_first_shared_query_word_then_add_order():
    db = db_with([(1, {5: 0.5}), (2, {3: 0.5}), (3, {3: 0.5, 5: 0.25})])
    scored, mc = db.query_begin(False, 10, bow({3: 0.5, 5: 0.5}))
    # word 3's list: 2, 3; word 5's list: 1, 3 -> 2, 3, 1.  Counts 1, 2, 1: max 2, min int(1.6f) = 1, so only 3 is scored
    assert [k for _, k in scored] == [3] and mc == 1
    db = db_with([(1, {5: 0.5}), (2, {3: 0.5}), (3, {3: 0.25})])
    scored, _ = db.query_begin(False, 10, bow({3: 0.5, 5: 0.5}))
    assert [(float(s), k) for s, k in scored] == [(0.5, 2), (0.25, 3), (0.5, 1)]


def test_erase_then_add_moves_a_keyframe_to_the_back():
    db = db_with([(1, {5: 0.5}), (2, {3: 0.5}), (3, {3: 0.25})])
    db.erase(2)
    db.add(2, bow({3: 0.5}))
    scored, _ = db.query_begin(False, 10, bow({3: 0.5, 5: 0.5}))
    assert [k for _, k in scored] == [3, 2, 1]
    db.erase(77)                                              # not in the database: a no-op
    scored, _ = db.query_begin(False, 11, bow({3: 0.5, 5: 0.5}))
    assert [k for _, k in scored] == [3, 2, 1]


def test_min_common_words_truncates_and_is_strict():
    # max 6 -> 6 * 0.8f = 4.8 -> 4: five shared words are scored (rounding would give 5 and drop it), four are not
    q = {w: 0.0625 for w in range(10)}
    db = db_with([(1, {w: 0.0625 for w in range(6)}), (2, {w: 0.0625 for w in range(5)}), (3, {w: 0.0625 for w in range(4)})])
    scored, mc = db.query_begin(False, 1, bow(q))
    assert mc == 4 and [k for _, k in scored] == [1, 2]
    # max 5 -> 5 * 0.8f = 4.0000001 -> 4: four shared words are not > 4
    db = db_with([(1, {w: 0.0625 for w in range(5)}), (2, {w: 0.0625 for w in range(4)})])
    scored, mc = db.query_begin(False, 1, bow(q))
    assert mc == 4 and [k for _, k in scored] == [1]
    assert int(F32(5) * F32(0.8)) == 4 and int(F32(6) * F32(0.8)) == 4


def test_loop_min_score_is_inclusive():
    db = db_with([(1, {1: 0.5}), (2, {2: 0.25}), (3, {3: 0.5})])
    scored, _ = db.query_begin(True, 50, bow({1: 0.5, 2: 0.5, 3: 0.5}), connected=(), min_score=0.5)
    assert [(float(s), k) for s, k in scored] == [(0.5, 1), (0.5, 3)]     # 0.5 >= 0.5 kept, 0.25 dropped
    assert db.kfs[2].mLoopScore == F32(0.25)                              # scored all the same


def test_best_keyframe_tie_keeps_the_first_and_duplicates_keep_the_first():
    # scores: 1 -> 0.25, 2 -> 0.5, 3 -> 0.5 (all scored: one shared word each)
    db = db_with([(1, {1: 0.25}), (2, {2: 0.5}), (3, {3: 0.5})])
    covis = {1: [3, 2], 2: [3], 3: [2]}
    scored, mc = db.query_begin(False, 9, bow({1: 0.5, 2: 0.5, 3: 0.5}))
    assert [k for _, k in scored] == [1, 2, 3]
    # 1: acc 0.25+0.5+0.5 = 1.25, best 3 (3 and 2 tie at 0.5; the first wins); 2: acc 1.0, best 2 (3's 0.5 is not > 0.5);
    # 3: acc 1.0, best 3.  min retain 0.75 * 1.25 = 0.9375: all three pass; 3 is output once, at its first place
    assert db.query_end(False, 9, scored, mc, covis) == [3, 2]


def test_relocalisation_neighbour_contributes_a_stale_score():
    db = db_with([(1, {2: 0.25, 3: 0.25}), (2, {1: 0.75}), (4, {4: 0.125, 5: 0.125})])
    assert db.DetectRelocalizationCandidates(10, bow({1: 0.75, 2: 0.25}), {}) == [2]   # 2 scores 0.75
    covis = {1: [2]}
    scored, mc = db.query_begin(False, 11, bow({1: 0.5, 2: 0.5, 3: 0.5, 4: 0.5, 5: 0.5}))
    # counts 2 -> 1, 1 -> 2, 4 -> 2: min 1, so 2 is pushed (mnRelocQuery = 11) but not scored
    assert [(float(s), k) for s, k in scored] == [(0.5, 1), (0.25, 4)]
    # 1's neighbour 2 brings query 10's 0.75 > 0.5: the best of 1's group is 2, which this query never scored
    assert db.query_end(False, 11, scored, mc, covis) == [2]


def test_query_id_zero_pushes_no_fresh_keyframe():
    db = db_with([(1, {1: 0.5}), (2, {2: 0.5})])
    assert db.query_begin(False, 0, bow({1: 0.5, 2: 0.5})) == ([], 0)
    assert db.DetectRelocalizationCandidates(5, bow({1: 0.5, 2: 0.5}), {}) == [1, 2]
    scored, _ = db.query_begin(False, 0, bow({1: 0.5, 2: 0.5}))
    assert [k for _, k in scored] == [1, 2]
    # the loop variant's mnLoopQuery starts at 0 too
    db = db_with([(1, {1: 0.5})])
    assert db.DetectLoopCandidates(0, bow({1: 0.5}), (), 0.0, {}) == []


def test_repeated_query_id_accumulates_counts():
    db = db_with([(1, {1: 1.0}), (2, {2: 0.25, 3: 0.25})])
    assert db.DetectLoopCandidates(7, bow({1: 1.0}), (), 0.0, {}) == [1]                 # 1 scores 1.0
    scored, mc = db.query_begin(True, 7, bow({1: 0.5, 2: 0.5, 3: 0.5}))
    # 1 is not pushed again (mnLoopQuery == 7) and its count goes 1 -> 2; 2 counts 2: min int(1.6f) = 1
    assert [(float(s), k) for s, k in scored] == [(0.5, 2)] and db.kfs[1].mnLoopWords == 2
    # 2's neighbour 1 passes mnLoopWords 2 > 1 and brings 1.0: the best is 1
    assert db.query_end(True, 7, scored, mc, {2: [1]}) == [1]
    # relocalisation: a repeated id pushes nothing already tagged with it
    db = db_with([(1, {1: 0.5})])
    assert db.DetectRelocalizationCandidates(3, bow({1: 0.5}), {}) == [1]
    assert db.DetectRelocalizationCandidates(3, bow({1: 0.5}), {}) == []
    assert db.kfs[1].mnRelocWords == 2


def test_loop_excludes_connected_keyframes_from_push_and_max():
    db = db_with([(1, {1: 0.5, 2: 0.5, 3: 0.5}), (2, {1: 0.25, 2: 0.25})])
    scored, mc = db.query_begin(True, 20, bow({1: 0.5, 2: 0.5, 3: 0.5}), connected=[1])
    # 1 shares three words but is connected: never pushed, its count reset at every encounter (ends at 1), and the max is 2's 2
    assert mc == 1 and [(float(s), k) for s, k in scored] == [(0.5, 2)]
    assert db.kfs[1].mnLoopQuery == 0 and db.kfs[1].mnLoopWords == 1
    # as a neighbour it does not count (mnLoopQuery != 20)
    assert db.query_end(True, 20, scored, mc, {2: [1]}) == [2]


def test_state_outlives_membership_and_clear():
    db = db_with([(1, {1: 0.5}), (2, {2: 0.5})])
    assert db.DetectRelocalizationCandidates(4, bow({1: 0.5, 2: 0.5}), {}) == [1, 2]
    db.clear()
    db.add(2, bow({2: 0.5}))
    # 2 keeps mnRelocQuery == 4 through clear() and re-add: the same id pushes nothing
    assert db.DetectRelocalizationCandidates(4, bow({2: 0.5}), {}) == []
    assert db.DetectRelocalizationCandidates(6, bow({2: 0.5}), {}) == [2]


def test_empty_bow_vectors_give_empty_results():
    db = db_with([(1, {}), (2, {1: 0.5})])
    assert db.DetectRelocalizationCandidates(1, bow({}), {}) == []
    assert db.DetectRelocalizationCandidates(2, bow({9: 0.5}), {}) == []
    assert db.DetectLoopCandidates(3, bow({}), (), 0.0, {}) == []
    assert db.DetectRelocalizationCandidates(4, bow({1: 0.5}), {}) == [2]


def test_score_matches_the_oracle_library():
    L = O.lib()
    L.oro_voc_score_l1.restype = C.c_double
    rng = np.random.default_rng(3)
    for _ in range(50):
        a = np.unique(rng.integers(0, 300, rng.integers(0, 120))).astype(np.int32)
        b = np.unique(rng.integers(0, 300, rng.integers(0, 120))).astype(np.int32)
        va, vb = rng.random(len(a)), rng.random(len(b))
        va /= max(va.sum(), 1e-300); vb /= max(vb.sum(), 1e-300)
        ref = L.oro_voc_score_l1(a.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), len(a),
                                 b.ctypes.data_as(C.c_void_p), vb.ctypes.data_as(C.c_void_p), len(b))
        got = K.score_l1((a, va), (b, vb))
        assert np.float64(got).tobytes() == np.float64(ref).tobytes()


# ---- the library without a GPU

@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def test_every_orbk_symbol_is_exported(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbk.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(orbk_[a-z0-9_]+)\s*\(", text))
    assert len(names) == 10
    lib = C.CDLL(built.LIB_PATH)
    assert [n for n in sorted(names) if not hasattr(lib, n)] == []


def test_invalid_arguments_return_a_status(built):
    L = built.lib()
    h = C.c_void_p()
    E = built.ORBX_E_INVALID
    assert L.orbk_create(None, 0, 100, 0, 4, 100) == E
    assert L.orbk_create(C.byref(h), 0, 100, 1, 4, 100) == E            # L2: ORB-SLAM2's vocabulary is L1
    assert L.orbk_create(C.byref(h), 0, 0, 0, 4, 100) == E
    assert L.orbk_create(C.byref(h), 0, 100, 0, -1, 100) == E
    assert not h
    ids = np.array([1, 2], np.int32); vals = np.array([0.5, 0.5])
    n = C.c_int()
    buf = np.zeros(4, np.uint64); fb = np.zeros(4, np.float32); off = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.orbk_add(None, 1, p(ids), p(vals), 2) == E
    assert L.orbk_erase(None, 1) == E
    assert L.orbk_clear(None) == E
    assert L.orbk_size(None) == E
    assert L.orbk_score(None, p(ids), p(vals), 2, p(buf), 1, C.byref(n)) == E
    assert L.orbk_query_begin(None, 0, 1, p(ids), p(vals), 2, None, 0, 0.0, p(buf), p(fb), 4, C.byref(n)) == E
    assert L.orbk_query_end(None, 0, p(off), p(buf), p(buf), 4, C.byref(n)) == E
    L.orbk_destroy(None)
    assert "NULL handle" in L.orbk_last_error().decode()


def test_no_gpu_fails_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(built.OrbxError) as ei:
        built.KeyFrameDatabase(1000)
    assert ei.value.code == built.ORBX_E_HIP and "no CPU path" in str(ei.value)


def test_adapter_compiles_the_reference_call_expressions(built, tmp_path):
    exe = str(tmp_path / "kfdb_callsites")
    libdir = os.path.dirname(built.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "kfdb_shims"),
           "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [os.path.join(ROOT, "tests", "cxx", "kfdb_callsites.cc"),
                           os.path.join(ROOT, "my-slam_amd", "host", "KeyFrameDatabase.cc"), "-o", exe, "-L" + libdir, "-lorbx",
                           "-Wl,-rpath," + libdir])
    src = open(os.path.join(ROOT, "tests", "cxx", "kfdb_callsites.cc")).read()
    for expr in ("mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame)", "mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore)",
                 "mpKeyFrameDB->add(pKF)", "mpKeyFrameDB->erase(pKF)", "mpKeyFrameDB->clear()"):
        assert expr in src
    assert subprocess.run([exe, "compile-only"]).returncode == 0


@pytest.mark.parametrize("first", ["FIRST_KEYFRAME", "FIRST_FRAME", "FIRST_MAPPOINT"])
def test_adapter_header_survives_the_reference_include_cycle(first):
    """KeyFrame.h includes Frame.h and KeyFrameDatabase.h before it defines KeyFrame, and Frame.h / MapPoint.h include
    KeyFrame.h (the shims keep that order): the adapter header must compile whichever of them a translation unit includes
    first, so it may only declare."""
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "kfdb_shims"),
           "-I" + os.path.join(ROOT, "include")]
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-D" + first] + inc +
                       [os.path.join(ROOT, "tests", "cxx", "kfdb_include_order.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
