"""The restatement of the key-frame database (tests/kfdb_oracle.py) against the reference's own src/KeyFrameDatabase.cc,
compiled unmodified into oracle/_ref/ref_kfdb behind a stand-in KeyFrame / Frame (oracle/ref/kfdb_standin.h).  The
restatement, the hand-worked cases of tests/test_kfdb_cpu.py and the library were written from one reading of that file;
these tests replace the reading with the file itself.  Everything is exact: ids equal, floats as bit patterns.  The case
list (tests/ref_kfdb.py) proves what it planted from its inputs or from the reference's output.  The last test needs no
reference program: it runs from the recorded outputs under tests/golden/kfdb/."""
import os

import numpy as np
import pytest

import ref_kfdb as R


@pytest.fixture(scope="module")
def pinned():
    """(control cases, edge cases, {name: reference events}): every case through ref_kfdb, every proof checked."""
    out = R.pinned_cases(build=True)
    if out is None:
        pytest.skip("oracle/_ref/ref_kfdb is not built and the reference tree is not present to build it from")
    return out


def check_events(name, ref, got):
    """Candidates, lScoreAndMatch (ids and score bits) and every dumped field, event by event."""
    assert [e[0] for e in got] == [e[0] for e in ref], name
    nq = 0
    for i, (a, b) in enumerate(zip(ref, got)):
        if a[0] == "q":
            assert b[1] == a[1], "%s: candidates of query %d" % (name, nq)
            assert b[2] == a[2], "%s: lScoreAndMatch of query %d" % (name, nq)
            nq += 1
        else:
            assert b[1] == a[1], "%s: key-frame fields at dump %d (event %d)" % (name, i - nq, i)
    return nq


def test_restatement_equals_reference(pinned):
    """Every case: the candidate lists, the reference's lScoreAndMatch against query_begin, and all six fields of every
    key frame wherever the script dumps them (after every operation in the control-flow cases)."""
    cc, ec, ref = pinned
    nq = sum(check_events(c.name, ref[c.name], R.run_oracle(c.ops)) for c in cc + ec)
    assert nq == sum(c.nqueries for c in cc + ec) and nq > 500
    assert sum(len(R.queries(ref[c.name])) for c in cc + ec) == nq


def test_min_common_words_equals_what_the_dumps_show(pinned):
    """minCommonWords is a local of the reference.  The dumps around a query bound it: a key frame the query pushed (its
    query id became the query's) that is in lScoreAndMatch had more words, a pushed one outside it had at most that many.
    That holds where the list has every scored key frame: relocalisation, and loop queries with minScore 0.  The
    restatement's value must lie in the bounds; where they pin one integer it is read exactly."""
    cc, _, ref = pinned
    exact = checked = 0
    for c in cc:
        ev, ov = ref[c.name], R.run_oracle(c.ops)
        qops = [op for op in c.ops if op[0] in ("reloc", "loop")]
        qi, before = 0, {}
        for i, e in enumerate(ev):
            if e[0] == "d":
                before = e[1]
                continue
            op = qops[qi]
            qi += 1
            loop = op[0] == "loop"
            if (loop and float(op[2]) > 0.0) or not e[2] or i + 1 >= len(ev) or ev[i + 1][0] != "d":
                continue
            lo, hi = R.min_common_bounds(before, ev[i + 1][1], e, loop, op[1])
            mc = ov[i][3]
            assert lo <= mc < hi, (c.name, qi - 1, lo, mc, hi)
            checked += 1
            exact += hi - lo == 1
    assert checked > 200 and exact > 50


def test_hand_worked_expectations_hold_on_the_reference(pinned):
    """The expected lists written out in tests/test_kfdb_cpu.py, replayed through ref_kfdb."""
    bits = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])
    cases = R.hand_worked()
    assert len(cases) >= 15
    for name, s, expected in cases:
        ev = R.run_ref(s.ops)
        qs = R.queries(ev)
        assert len(qs) == len(expected), name
        for q, (cand, scored) in zip(qs, expected):
            if cand is not None:
                assert q[1] == cand, name
            if scored is not None:
                assert q[2] == [(k, bits(v)) for v, k in scored], name
        check_events(name, ev, R.run_oracle(s.ops))
    # the counts the hand-worked cases assert, read from the reference's dumps
    last = {name: R.run_ref(s.ops)[-1][1] for name, s, _ in cases}          # every hand-worked script ends with a dump
    assert last["repeated_loop_id"][1][:2] == (7, 2)                   # mnLoopWords went 1 -> 2 under the repeated id
    assert last["repeated_reloc_id"][1][3:5] == (3, 2)
    assert last["connected_excluded"][1][:2] == (0, 1)                 # connected: never tagged, count left at 1
    assert last["min_score_inclusive"][2][:3] == (50, 1, bits(0.25))   # below minScore, scored all the same


def test_reference_runs_clean_under_ubsan(pinned):
    """Every compared case once through ref_kfdb_ubsan (a stand-alone program, nothing preloaded): it exits at the first
    undefined operation, and its output equals the plain build's."""
    cc, ec, ref = pinned
    for c in cc + ec:
        assert R.parse_output(R.run_ref_text(c.text, R.EXE_UBSAN)) == ref[c.name], c.name
    for name, s, _ in R.hand_worked():
        R.run_ref_text(R.text(s.ops), R.EXE_UBSAN)


def test_driver_refuses_what_the_reference_leaves_undefined(pinned):
    """A word id >= the vocabulary size would index past mvInvertedFile: the driver stops with status 2, so no case can
    hold one unnoticed."""
    import subprocess
    for script in ("words 10\nkf 1 1 10 0.5\n", "words 10\nreloc 1 1 12 0.5\n", "kf 1 0\n", "words 10\nfrobnicate\n"):
        with pytest.raises(subprocess.CalledProcessError) as ei:
            R.run_ref_text(script)
        assert ei.value.returncode == 2


def test_case_list_is_what_it_claims():
    """The conditions that make the kernel-edge cases meaningful, from their inputs alone (no reference, no library)."""
    by = {c.name: c for c in R.edge_cases()}
    f = by["chunks"].facts
    assert [n for n, _ in f["second_chunk"]] == [65, 128, 129] and all(64 <= p[0] < 128 for _, p in f["second_chunk"])
    assert {n for g in f.values() for n, _ in g} == set(R.CHUNK_LENGTHS) - {0}
    assert by["long_queries"].facts["query_lengths"] == [1, R.LDS_QUERY, R.LDS_QUERY + 1]
    slots = by["slots"].facts["slots"]
    assert slots[::2] == list(R.SLOT_COUNTS) and slots[4] > R.WAVES and slots[6] > 2 * R.WAVES
    na, nb, _ = by["second_download"].facts["records"]
    assert na < 10 and nb > 300 and nb > max(R.REC_GUESS, na + na // 4)
    comp = next(c for c in R.control_cases() if c.name == "compaction_order")
    assert comp.facts["compactions"] == [0, 1, 2, 3]


def test_golden_scripts_equal_their_recorded_reference_output():
    """tests/golden/kfdb/: one control-flow script and one kernel-edge script with ref_kfdb's recorded output (data only;
    tests/golden/make_golden_kfdb.py regenerates them).  The restatement must reproduce both without the reference."""
    n = 0
    for name in ("control", "edges"):
        script = open(os.path.join(R.GOLDEN, name + ".script")).read()
        ref = R.parse_output(open(os.path.join(R.GOLDEN, name + ".out")).read())
        ops = R.parse(script)
        assert R.text(ops) == script
        n += check_events(name, ref, R.run_oracle(ops))
    assert n == 61
