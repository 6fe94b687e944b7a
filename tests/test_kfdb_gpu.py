"""The keyframe database on the GPU (include/orbk.h) against the restatement of src/KeyFrameDatabase.cc (tests/kfdb_oracle.py)
and DBoW2's L1 score (oro_voc_score_l1): the scoring kernel's records bit for bit, long mixed call sequences on one handle,
arena growth, capacity retries, an end-to-end run from synthetic frames, the C++ adapter and concurrent callers."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import kfdb_oracle as K
import oracle_lib as O
from test_vocabulary import make_vocabulary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_QUERY = 8192              # K_LDS_QUERY of orbk.hip: longer queries take the global-memory search


def _score_ref(a, b):
    L = O.lib()
    L.oro_voc_score_l1.restype = C.c_double
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    return L.oro_voc_score_l1(p(a[0]), p(a[1]), len(a[0]), p(b[0]), p(b[1]), len(b[0]))


def zipf_bow(rng, perm, n):
    """About n distinct words, Zipf-distributed ranks over the vocabulary, L1-normalised random values."""
    nwords = len(perm)
    ids = np.zeros(0, np.int64)
    while len(ids) < n:
        r = rng.zipf(1.1, 4 * n) - 1
        ids = np.unique(np.concatenate([ids, perm[r[r < nwords]]]))
    ids = np.sort(rng.choice(ids, n, replace=False)).astype(np.int32)
    v = rng.random(n) + 1e-3
    return ids, v / v.sum()


def expected_records(kfs, q):
    out = []
    for kid, b in kfs:
        _, iq, _ = np.intersect1d(q[0], b[0], assume_unique=True, return_indices=True)
        if len(iq):
            out.append((kid, len(iq), int(iq.min()), _score_ref(q, b)))
    return out


def check_records(db, kfs, q):
    got = db.score(q)
    exp = expected_records(kfs, q)
    assert len(got) == len(exp)
    assert [int(x) for x in got["id"]] == [e[0] for e in exp]
    assert got["words"].tolist() == [e[1] for e in exp]
    assert got["first"].tolist() == [e[2] for e in exp]
    assert got["score"].view(np.uint64).tolist() == np.array([e[3] for e in exp], np.float64).view(np.uint64).tolist()
    return len(got)


def test_score_records_equal_direct_computation(orbx):
    rng = np.random.default_rng(1)
    nwords = 1_000_000
    perm = rng.permutation(nwords)
    db = orbx.KeyFrameDatabase(nwords, max_keyframes=64, max_entries=1 << 16)
    kfs = [(7, (np.zeros(0, np.int32), np.zeros(0))), (8, (np.array([int(perm[0])], np.int32), np.array([1.0])))]
    for kid, b in kfs:
        db.add(kid, b)
    for i in range(5000):
        b = zipf_bow(rng, perm, int(rng.integers(200, 1200)))
        db.add(100 + i, b)
        kfs.append((100 + i, b))
    assert len(db) == 5002
    sizes = [2000, 1, 50, LDS_QUERY, LDS_QUERY + 1, 12000]
    for n in sizes:
        q = zipf_bow(rng, perm, n)
        assert check_records(db, kfs, q) > 0
    # a query sharing no word, an empty query, a one-entry query on the one-entry keyframe
    used = np.unique(np.concatenate([b[0] for _, b in kfs]))
    free = np.setdiff1d(np.arange(nwords, dtype=np.int32), used)[:3000]
    assert check_records(db, kfs, (free[:300], np.full(300, 1 / 300))) == 0
    assert check_records(db, kfs, (free[:LDS_QUERY + 100], np.full(LDS_QUERY + 100, 0.5))) == 0
    assert len(db.score((np.zeros(0, np.int32), np.zeros(0)))) == 0
    assert check_records(db, kfs, (np.array([int(perm[0])], np.int32), np.array([0.25]))) >= 1


# ---- mixed call sequences

VALS = (0.125, 0.25, 0.5, 1.0)


def small_bow(rng, nw=40):
    n = int(rng.integers(0, 9))
    ids = np.sort(rng.choice(nw, n, replace=False)).astype(np.int32)
    return ids, np.array([VALS[i] for i in rng.integers(0, 4, n)], np.float64)


def run_sequence(orbx, seed, nops, ctx):
    """nops random calls on ctx's handle and restatement; ctx carries both, the present ids and their BowVectors."""
    rng = np.random.default_rng(seed)
    nw = 40
    db, oracle, present, bows = ctx["db"], ctx["oracle"], ctx["present"], ctx["bows"]
    nq = 0
    for _ in range(nops):
        op = rng.random()
        if op < 0.35:
            kid = int(rng.integers(1, 31))
            if kid in present:
                with pytest.raises(orbx.OrbxError) as ei:
                    db.add(kid, bows[kid])
                assert ei.value.code == orbx.ORBX_E_INVALID
                continue
            bows[kid] = small_bow(rng, nw)
            db.add(kid, bows[kid]); oracle.add(kid, bows[kid])
            present.append(kid)
        elif op < 0.5:
            kid = int(rng.integers(1, 36))
            db.erase(kid); oracle.erase(kid)
            if kid in present:
                present.remove(kid)
        elif op < 0.52:
            db.clear(); oracle.clear()
            present.clear()
        else:
            loop = op >= 0.76
            kind = orbx.ORBK_LOOP if loop else orbx.ORBK_RELOC
            qid = int(rng.integers(0, 7))
            q = small_bow(rng, nw)
            conn = [int(x) for x in rng.choice(36, int(rng.integers(0, 5)), replace=False)] if loop else []
            min_score = float(rng.choice([0.0, 0.125, 0.25, 0.5, 0.75])) if loop else 0.0
            ids, si = db.query_begin(kind, qid, q, conn, min_score)
            exp, mc = oracle.query_begin(loop, qid, q, conn, min_score)
            assert [int(x) for x in ids] == [k for _, k in exp], (seed, nq)
            assert si.view(np.uint32).tolist() == np.array([s for s, _ in exp], np.float32).view(np.uint32).tolist()
            covis = {int(k): [int(x) for x in rng.integers(0, 36, int(rng.integers(0, 11)))] for k in ids}
            got = db.query_end(kind, ids, covis)
            assert got == oracle.query_end(loop, qid, exp, mc, covis, min_score), (seed, nq)
            nq += 1
        assert len(db) == len(present)
    return nq


def test_mixed_sequences_equal_the_restatement(orbx):
    nw = 40
    ctx = dict(db=orbx.KeyFrameDatabase(nw, max_keyframes=4, max_entries=16), oracle=K.KeyFrameDatabase(nw), present=[], bows={})
    total = sum(run_sequence(orbx, 100 + seed, 300, ctx) for seed in range(6))      # one long-lived handle
    assert total > 500


def test_growth_from_a_tiny_handle(orbx):
    rng = np.random.default_rng(5)
    nw = 5000
    perm = rng.permutation(nw)
    db = orbx.KeyFrameDatabase(nw, max_keyframes=4, max_entries=100)
    oracle = K.KeyFrameDatabase(nw)
    live = []
    for i in range(2000):
        b = zipf_bow(rng, perm, int(rng.integers(1, 60)))
        db.add(i + 1, b); oracle.add(i + 1, b)
        live.append(i + 1)
        if i % 7 == 3:
            k = live.pop(int(rng.integers(0, len(live))))
            db.erase(k); oracle.erase(k)
        if i % 250 == 249:
            q = zipf_bow(rng, perm, 200)
            covis = {k: [int(x) for x in rng.integers(1, i + 2, 10)] for k in live}
            assert db.DetectRelocalizationCandidates(10_000 + i, q, covis) == oracle.DetectRelocalizationCandidates(10_000 + i, q, covis)
            assert db.DetectLoopCandidates(20_000 + i, q, live[:5], 0.01, covis) == oracle.DetectLoopCandidates(20_000 + i, q, live[:5], 0.01, covis)
    assert len(db) == len(live)
    kfs = [(k, oracle.kfs[k].bow) for k in live]
    check_records(db, kfs, zipf_bow(rng, perm, 300))


def test_capacity_error_commits_no_state(orbx):
    rng = np.random.default_rng(9)
    nw = 40
    db = orbx.KeyFrameDatabase(nw)
    oracle = K.KeyFrameDatabase(nw)
    for k in range(1, 21):
        b = small_bow(rng, nw)
        db.add(k, b); oracle.add(k, b)
    q = (np.arange(0, 40, 2, dtype=np.int32), np.full(20, 0.25))
    for loop, kind in ((False, orbx.ORBK_RELOC), (True, orbx.ORBK_LOOP)):
        with pytest.raises(orbx.OrbxError) as ei:
            db.query_begin(kind, 3, q, [1, 2], 0.0, cap=1)
        assert ei.value.code == orbx.ORBX_E_CAPACITY
        with pytest.raises(orbx.OrbxError) as ei:
            db.query_end(kind, [], {})                         # nothing pending after the refused begin
        assert ei.value.code == orbx.ORBX_E_INVALID
        ids, si = db.query_begin(kind, 3, q, [1, 2], 0.0)
        exp, mc = oracle.query_begin(loop, 3, q, [1, 2], 0.0)
        assert len(exp) > 1
        assert [int(x) for x in ids] == [k for _, k in exp]
        assert si.view(np.uint32).tolist() == np.array([s for s, _ in exp], np.float32).view(np.uint32).tolist()
        covis = {int(k): [int(k) % 20 + 1] for k in ids}
        assert db.query_end(kind, ids, covis) == oracle.query_end(loop, 3, exp, mc, covis)


def test_invalid_bow_vectors_are_refused(orbx):
    db = orbx.KeyFrameDatabase(100)
    for ids in ([3, 3], [5, 4], [-1], [100]):
        b = (np.array(ids, np.int32), np.full(len(ids), 0.5))
        for call in (lambda: db.add(1, b), lambda: db.score(b), lambda: db.query_begin(orbx.ORBK_RELOC, 1, b)):
            with pytest.raises(orbx.OrbxError) as ei:
                call()
            assert ei.value.code == orbx.ORBX_E_INVALID
    assert len(db) == 0
    with pytest.raises(orbx.OrbxError) as ei:
        orbx.KeyFrameDatabase(100, scoring=1)
    assert ei.value.code == orbx.ORBX_E_INVALID


def test_end_to_end_from_synthetic_frames(orbx, synth, tmp_path):
    path = str(tmp_path / "voc.txt")
    make_vocabulary(path, k=10, depth=4, seed=11)
    voc = orbx.ORBVocabulary(path)
    ex = orbx.ORBextractor(1000, max_width=640, max_height=480)
    frames = synth.stream(21, 640, 480, 60, step=(40, 20))        # keyframes 240 px apart, the query 40 px from its keyframe
    db = orbx.KeyFrameDatabase(voc.nwords)
    oracle = K.KeyFrameDatabase(voc.nwords)
    bows = {}
    for j in range(0, 60, 6):
        bows[j] = voc.transform(ex(frames[j])[1])[0]
        db.add(j + 1, bows[j]); oracle.add(j + 1, bows[j])
    covis = {j + 1: [i + 1 for i in range(0, 60, 6) if 0 < abs(i - j) <= 12] for j in range(0, 60, 6)}
    for j in (12, 30, 48):
        q = voc.transform(ex(frames[j + 1])[1])[0]
        got = db.DetectRelocalizationCandidates(1000 + j, q, covis)
        assert got == oracle.DetectRelocalizationCandidates(1000 + j, q, covis)
        assert j + 1 in got
        conn = [k for k in covis[j + 1] if abs(k - j - 1) <= 6]
        got = db.DetectLoopCandidates(j + 1, bows[j], conn, 0.0, covis)
        assert got == oracle.DetectLoopCandidates(j + 1, bows[j], conn, 0.0, covis)


def _script_and_expected(seed, nops):
    rng = np.random.default_rng(seed)
    nw = 40
    oracle = K.KeyFrameDatabase(nw)
    lines, expected = ["words %d" % nw], []
    fmt = lambda b: "%d %s" % (len(b[0]), " ".join("%d %.17g" % (w, v) for w, v in zip(b[0], b[1])))
    covis, conn, bows, present = {}, {}, {}, set()
    for k in range(1, 36):
        covis[k] = [int(x) for x in rng.integers(1, 36, int(rng.integers(0, 13)))]
        conn[k] = [int(x) for x in rng.choice(np.arange(1, 36), int(rng.integers(0, 4)), replace=False)]
        bows[k] = small_bow(rng, nw)
        lines += ["kf %d %s" % (k, fmt(bows[k])), "covis %d %d %s" % (k, len(covis[k]), " ".join(map(str, covis[k]))),
                  "conn %d %d %s" % (k, len(conn[k]), " ".join(map(str, conn[k])))]
    covis10 = {k: v[:10] for k, v in covis.items()}
    for _ in range(nops):
        op = rng.random()
        if op < 0.3:
            k = int(rng.integers(1, 31))
            if k not in present:
                lines.append("add %d" % k); oracle.add(k, bows[k]); present.add(k)
        elif op < 0.45:
            k = int(rng.integers(1, 36))
            lines.append("erase %d" % k); oracle.erase(k); present.discard(k)
        elif op < 0.47:
            lines.append("clear"); oracle.clear(); present = set()
        elif op < 0.75:
            qid = int(rng.integers(0, 7))
            q = small_bow(rng, nw)
            lines.append("reloc %d %s" % (qid, fmt(q)))
            expected.append(oracle.DetectRelocalizationCandidates(qid, q, covis10))
        else:
            k = int(rng.integers(1, 36))
            ms = np.float32(rng.choice([0.0, 0.125, 0.25, 0.5]))
            lines.append("loop %d %.9g" % (k, ms))
            expected.append(oracle.DetectLoopCandidates(k, bows[k], conn[k], ms, covis10))
    return "\n".join(lines) + "\n", expected


def test_cxx_adapter_equals_the_restatement(orbx, tmp_path):
    orbx.build()
    exe = str(tmp_path / "kfdb_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "kfdb_shims"),
           "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + inc + [os.path.join(ROOT, "tests", "cxx", "kfdb_callsites.cc"),
                                                              os.path.join(ROOT, "my-slam_amd", "host", "KeyFrameDatabase.cc"), "-o", exe,
                                                              "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    for seed in (1, 2, 3):
        script, expected = _script_and_expected(seed, 250)
        r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = [[int(x) for x in l.split()] for l in r.stdout.split("\n")[:-1]]
        assert got == expected
        assert sum(len(e) > 0 for e in expected) > 20


def test_concurrent_callers(orbx):
    rng = np.random.default_rng(17)
    nw = 2000
    perm = rng.permutation(nw)
    db = orbx.KeyFrameDatabase(nw, max_keyframes=8, max_entries=256)
    initial = list(range(1, 201))
    bows = {k: zipf_bow(rng, perm, int(rng.integers(20, 120))) for k in range(1, 401)}
    for k in initial:
        db.add(k, bows[k])
    erased = [int(x) for x in rng.choice(initial, 80, replace=False)]
    added = list(range(201, 401))
    queries = [zipf_bow(rng, perm, 150) for _ in range(40)]
    covis = {k: [int(x) for x in rng.integers(1, 401, 10)] for k in range(1, 401)}
    errors = []

    def guard(fn):
        def run():
            try:
                fn()
            except Exception as e:          # noqa: BLE001 -- reported after join
                errors.append(repr(e))
        return run

    def reloc():
        for i in range(120):
            db.DetectRelocalizationCandidates(5000 + i, queries[i % 40], covis)

    def adder():
        for i, k in enumerate(added):
            db.add(k, bows[k])
            if i % 4 == 0:
                db.DetectLoopCandidates(k, bows[k], covis[k][:3], 0.0, covis)

    def eraser():
        for k in erased:
            db.erase(k)

    ts = [threading.Thread(target=guard(f)) for f in (reloc, adder, eraser)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errors == []
    final = [k for k in initial if k not in set(erased)] + added
    assert len(db) == len(final)
    oracle = K.KeyFrameDatabase(nw)
    for k in final:
        oracle.add(k, bows[k])
    q = queries[0]
    got = db.DetectLoopCandidates(99_999, q, [1, 2, 3], 0.0, covis)
    assert got == oracle.DetectLoopCandidates(99_999, q, [1, 2, 3], 0.0, covis)
    ids, si = db.query_begin(orbx.ORBK_LOOP, 99_998, q, [1, 2, 3], 0.0)
    exp, _ = oracle.query_begin(True, 99_998, q, [1, 2, 3], 0.0)
    assert [int(x) for x in ids] == [k for _, k in exp] and len(exp) > 0
    db.query_end(orbx.ORBK_LOOP, ids, covis)
