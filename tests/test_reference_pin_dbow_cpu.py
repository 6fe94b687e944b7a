"""The oracle's vocabulary functions (oro_voc_* of oracle/orb_oracle.c) and the Python L1 score (tests/kfdb_oracle.py) against
the reference's own Thirdparty/DBoW2, compiled unmodified on the OpenCV shim into oracle/_ref/ref_dbow.  Both restatements
were written from one reading of DBoW2; these tests replace that reading with DBoW2 itself.  Ints must be equal, doubles are
compared as bit patterns.  The case list (tests/ref_dbow.py) proves what it planted with a numpy walk of the node table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kfdb_oracle as K
import oracle_lib as O
import ref_dbow as D
from test_vocabulary import oracle_transform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_score(a, b):
    L = O.lib()
    L.oro_voc_score_l1.restype = C.c_double
    a = (np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.float64))
    b = (np.ascontiguousarray(b[0], np.int32), np.ascontiguousarray(b[1], np.float64))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    return L.oro_voc_score_l1(p(a[0]), p(a[1]), len(a[0]), p(b[0]), p(b[1]), len(b[0]))


@pytest.fixture(scope="module")
def pinned(tmp_path_factory):
    """(cases, {name: (LOAD result, [TRANSFORM result per run])}): every case through one ref_dbow process."""
    out = D.pinned_cases(str(tmp_path_factory.mktemp("dbow_cases")), build=True)
    if out is None:
        pytest.skip("oracle/_ref/ref_dbow is not built and the reference tree is not present to build it from")
    return out


def test_case_tables_equal_reference_load(pinned):
    """The node table each case hands the oracle is what loadFromTextFile builds from the case's file."""
    cases, ref = pinned
    for c in cases:
        D.check_load(c.name, c.voc, ref[c.name][0])


def test_oracle_transform_equals_reference(pinned):
    cases, ref = pinned
    for c in cases:
        for r, (feat, levelsup) in enumerate(c.runs):
            D.check_run("%s, n=%d, levelsup=%d" % (c.name, len(feat), levelsup), c.voc, feat, levelsup,
                        oracle_transform(c.voc, feat, levelsup), ref[c.name][1][r])


def test_stopped_and_unnormalised_cases_are_what_they_claim(pinned):
    """With every word stopped both vectors are empty; DOT_PRODUCT alone leaves the BowVector unnormalised, every other
    scoring type gives norm 1 (L2 in the 2-norm, the rest in the 1-norm)."""
    cases, ref = pinned
    seen = set()
    for c in cases:
        for res in ref[c.name][1]:
            ids, vals = res["bow"]
            if c.name.startswith("stop_all"):
                assert len(ids) == 0 and len(res["fv"]) == 0 and len(res["word"]) > 0
            elif len(ids):
                s = c.voc["scoring"]
                seen.add(s)
                norm = np.sqrt((vals * vals).sum()) if s == 1 else np.abs(vals).sum()
                assert (abs(norm - 1.0) < 1e-12) == (s != 5), (c.name, norm)
    assert seen == {0, 1, 2, 3, 4, 5}


def test_planted_cases_prove_themselves(pinned):
    """Counted with numpy from the node table and the features alone: features that meet an exact tie for the minimum at some
    level, features whose winner sits at child position >= 64, and features whose leaf is deep enough for a node id."""
    cases, _ = pinned
    planted = 0
    for c in cases:
        ties = late = total = 0
        for feat, levelsup in c.runs:
            depth, tie, lt = D.descend(c.voc, feat)
            ties += int(tie.sum()); late += int(lt.sum()); total += len(feat)
            assert tie[:c.n_planted].all(), "%s: a planted feature meets no tie" % c.name
            planted += c.n_planted
            if c.min_deep and levelsup in c.min_deep:
                share = float((depth >= c.voc["L"] - levelsup).mean())
                assert c.min_deep[levelsup] <= share <= 0.9, "%s, levelsup %d: %.3f of the features have a node id" % (c.name, levelsup, share)
        assert ties >= c.min_ties, "%s: %d ties, %d planted" % (c.name, ties, c.min_ties)
        assert late >= c.min_late * total, "%s: %d of %d winners at position >= 64" % (c.name, late, total)
    assert planted >= 60
    kids = {int(n) for c in cases for n in np.diff(c.voc["child_off"])}
    assert {1, 2, 20, 64, 65, 130} <= kids
    depths = {(c.voc["L"]) for c in cases}
    assert {1, 10} <= depths


def test_l1_scores_equal_reference(pinned):
    """oro_voc_score_l1 and kfdb_oracle.score_l1 == L1Scoring::score bit for bit: consecutive BowVectors of each L1 case, one
    against itself, two without a common word, empty against full and empty against empty."""
    cases, ref = pinned
    l1 = [c for c in cases if c.voc["scoring"] == 0]
    pairs = {c.name: D.score_pairs(ref[c.name][1]) for c in l1}
    out = D.run([r for c in l1 for r in (D.req_load(c.path), D.req_score(pairs[c.name]))])[1::2]
    n = between = 0
    for c, scores in zip(l1, out):
        for (a, b), s in zip(pairs[c.name], scores):
            for name, got in (("oro_voc_score_l1", oracle_score(a, b)), ("kfdb_oracle.score_l1", K.score_l1(a, b))):
                assert D.u64(got) == D.u64(s), "%s, %s: %r vs reference %r" % (c.name, name, got, s)
            n += 1
        assert all(D.u64(x) == D.u64(-0.0) for x in scores[-4:])                             # no common word: -0 / 2
        if not c.name.startswith("stop_all"):
            assert abs(scores[-5] - 1.0) < 1e-12                                             # identical: 1 up to rounding
            between += int(((scores[:-5] > 0.0) & (scores[:-5] < 1.0)).sum())
    assert n > 100 and between > 20


def test_ubsan_build_runs_the_whole_case_list(pinned):
    cases, ref = pinned
    l1 = [c for c in cases if c.voc["scoring"] == 0][:3]
    reqs = [r for c in cases for r in c.requests()]
    reqs += [r for c in l1 for r in (D.req_load(c.path), D.req_score(D.score_pairs(ref[c.name][1])))]
    D.run(reqs, D.EXE_UBSAN)          # raises on a non-zero exit


def test_driver_refuses_what_the_reference_cannot_load(pinned, tmp_path):
    """A missing file (loadFromTextFile would never return) and more nodes than it reserves (its word pointers would dangle)."""
    cases, _ = pinned
    with pytest.raises(subprocess.CalledProcessError) as e:
        D.run([D.req_load(str(tmp_path / "absent.txt"))])
    assert e.value.returncode == 2 and "cannot open" in e.value.stderr
    big = str(tmp_path / "big.txt")
    with open(cases[0].path) as f, open(big, "w") as g:
        g.write(f.read().replace("10 3 ", "10 2 ", 1))          # 1110 node lines under a header that reserves 111
    with pytest.raises(subprocess.CalledProcessError) as e:
        D.run([D.req_load(big)])
    assert e.value.returncode == 2 and "reserves" in e.value.stderr


def test_final_newline_makes_no_difference_to_the_driver(pinned, tmp_path):
    cases, ref = pinned
    c = next(c for c in cases if c.name == "no_final_newline")
    p = str(tmp_path / "with_newline.txt")
    D.write_vocabulary(p, c.voc, trailing_newline=True)
    (ld,) = D.run([D.req_load(p)])
    D.check_load("with the final newline", c.voc, ld)


# ---- the vocabulary the reference trained itself (tests/golden/make_golden_dbow.py); needs neither the binary nor the reference

def test_oracle_equals_golden_reference_vocabulary():
    path, runs, load, scores = D.golden_fixture()
    voc = D.parse_vocabulary_text(path)
    D.check_load("golden", voc, load)
    assert voc["nnodes"] < (6 ** 4 - 1) // 5 and len(set(np.diff(voc["child_off"]).tolist())) > 2     # k-means left it unbalanced
    shallow = 0
    for r, (feat, levelsup, res) in enumerate(runs):
        deep = D.check_run("golden run %d" % r, voc, feat, levelsup, oracle_transform(voc, feat, levelsup), res)
        shallow += int((~deep).sum())
    assert shallow > 0
    for a, b, s in scores:
        pa, pb = runs[a][2]["bow"], runs[b][2]["bow"]
        assert D.u64(oracle_score(pa, pb)) == D.u64(s) and D.u64(K.score_l1(pa, pb)) == D.u64(s)
