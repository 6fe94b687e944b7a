"""GPU parity against the reference's own DBoW2: the HIP library's vocabulary loader, tree descent, BowVector, FeatureVector
and L1 score (include/orbv.h) and the key-frame database's scores (include/orbk.h) == oracle/_ref/ref_dbow, the reference's
Thirdparty/DBoW2 compiled unmodified, with no step through the oracle.  Everything is bit-exact.  ref_dbow is a CPU program
that build() leaves under oracle/_ref/; apart from it these tests read nothing of the reference, and the last one (a
vocabulary the reference trained, stored under tests/golden/) does not need it either."""
import numpy as np
import pytest

import ref_dbow as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned(tmp_path_factory):
    out = D.pinned_cases(str(tmp_path_factory.mktemp("dbow_cases")))
    if out is None:
        pytest.skip("oracle/_ref/ref_dbow was not built (build() compiles it where the reference tree is present)")
    return out


def product(v, feat, levelsup):
    return v.transform_features(feat, levelsup), *v.transform(feat, levelsup)


def info(v):
    return dict(k=v.k, L=v.depth, nnodes=v.nnodes, nwords=v.nwords, scoring=v.scoring, weighting=v.weighting)


def as_bytes(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for part in got for a in part)


def test_loader_and_descent_equal_reference(orbx, pinned):
    """Every case vocabulary: orbv_info == LOAD, and every run == TRANSFORM.  The cases cover n at the 4-waves-per-block
    edges, depth 1 and depth 10, unbalanced trees, nodes of 1 to 130 children, planted ties (the first child wins, also across
    the 64-child trips), distance 0 and 256, levelsup from 0 to L + 1, stopped words, and all weightings and scorings."""
    cases, ref = pinned
    for c in cases:
        v = orbx.ORBVocabulary(c.path)
        load, results = ref[c.name]
        assert info(v) == {k: load[k] for k in info(v)}, c.name
        for (feat, levelsup), res in zip(c.runs, results):
            D.check_run("%s, n=%d, levelsup=%d" % (c.name, len(feat), levelsup), c.voc, feat, levelsup, product(v, feat, levelsup), res)
        v.close()


def test_final_newline_is_ignored(orbx, pinned, tmp_path):
    """include/orbv.h: the loader ignores the empty line that saveToTextFile's final newline leaves, where the reference
    appends a node; both spellings of one file give the same vocabulary and the same results."""
    cases, ref = pinned
    c = next(c for c in cases if c.name == "no_final_newline")
    other = str(tmp_path / "with_newline.txt")
    D.write_vocabulary(other, c.voc, trailing_newline=True)
    assert open(other).read() == open(c.path).read() + "\n"
    a, b = orbx.ORBVocabulary(c.path), orbx.ORBVocabulary(other)
    assert info(a) == info(b) == {k: ref[c.name][0][k] for k in info(a)}
    feat, levelsup = c.runs[0]
    assert as_bytes(product(a, feat, levelsup)) == as_bytes(product(b, feat, levelsup))
    D.check_run("with the final newline", c.voc, feat, levelsup, product(b, feat, levelsup), ref[c.name][1][0])


def test_staging_growth_on_a_live_handle(orbx, pinned):
    """One handle called with n = 1, then 3000, then 5: the call after each growth of the staging buffers equals the
    reference's and a fresh handle's; the same features twice give the same bytes."""
    cases, ref = pinned
    c = cases[0]
    by_n = {len(f): (f, l, r) for (f, l), r in zip(c.runs, ref[c.name][1])}
    live = orbx.ORBVocabulary(c.path)
    for n in (1, 3000, 5):
        feat, levelsup, res = by_n[n]
        got = product(live, feat, levelsup)
        D.check_run("live handle, n=%d" % n, c.voc, feat, levelsup, got, res)
        fresh = orbx.ORBVocabulary(c.path)
        assert as_bytes(got) == as_bytes(product(fresh, feat, levelsup)), n
        fresh.close()
    feat, levelsup, _ = by_n[257]
    assert as_bytes(product(live, feat, levelsup)) == as_bytes(product(live, feat, levelsup))


def test_vocabulary_score_equals_reference(orbx, pinned):
    """ORBVocabulary.score == L1Scoring::score bit for bit on the L1 cases' BowVectors: consecutive ones, one against itself,
    two without a common word, and empty ones."""
    cases, ref = pinned
    l1 = [c for c in cases if c.voc["scoring"] == 0]
    pairs = {c.name: D.score_pairs(ref[c.name][1]) for c in l1}
    out = D.run([r for c in l1 for r in (D.req_load(c.path), D.req_score(pairs[c.name]))])[1::2]
    n = 0
    for c, scores in zip(l1, out):
        v = orbx.ORBVocabulary(c.path)
        for (a, b), s in zip(pairs[c.name], scores):
            a = (np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.float64))
            b = (np.ascontiguousarray(b[0], np.int32), np.ascontiguousarray(b[1], np.float64))
            got = v.score(a, b)
            assert D.u64(got) == D.u64(s), "%s: %r vs reference %r" % (c.name, got, s)
            n += 1
        v.close()
    assert n > 100


def test_keyframe_database_scores_equal_reference(orbx, pinned):
    """KeyFrameDatabase.score(bow) per key frame == voc.score(query, key frame) of the reference, over 50 key frames built
    from features: one identical to the query, five that share no word with it (no record; the reference scores them -0),
    the rest random.  The vocabulary has all its 20 words under the root, so a feature three bits from a word's descriptor is
    that word and the word sets are the test's to choose."""
    cases, ref = pinned
    c = next(c for c in cases if c.name == "depth1_k20")
    rng = np.random.default_rng(77)
    leaves = D.children(c.voc, 0)

    def features(words):
        return np.array([D.flip(c.voc["desc"][leaves[w]], rng.choice(256, 3, replace=False)) for w in words], np.uint8)

    query = features(rng.integers(0, 10, 40))
    kfs = [query] + [features(rng.integers(10, 20, int(rng.integers(5, 60)))) for _ in range(5)]
    kfs += [features(rng.integers(0, 20, int(rng.integers(1, 60)))) for _ in range(44)]
    res = D.run([D.req_load(c.path)] + [D.req_transform(f, 0) for f in kfs])[1:]
    qbow = res[0]["bow"]
    scores = D.run([D.req_load(c.path), D.req_score([(qbow, r["bow"]) for r in res])])[1]
    v = orbx.ORBVocabulary(c.path)
    db = orbx.KeyFrameDatabase(v.nwords, max_keyframes=64, max_entries=1 << 12)
    expected = []
    for i, (f, r) in enumerate(zip(kfs, res)):
        bow, _ = v.transform(f, 0)
        assert np.array_equal(bow[0], r["bow"][0]) and np.array_equal(D.u64(bow[1]), D.u64(r["bow"][1])), i
        db.add(100 + i, bow)
        _, iq, _ = np.intersect1d(qbow[0], r["bow"][0], assume_unique=True, return_indices=True)
        if len(iq):
            expected.append((100 + i, len(iq), int(iq.min()), scores[i]))
        else:
            assert D.u64(scores[i]) == D.u64(-0.0)
    assert 35 <= len(expected) <= 45 and expected[0][0] == 100 and not set(range(101, 106)) & {e[0] for e in expected}
    assert abs(scores[0] - 1.0) < 1e-12
    qb, _ = v.transform(query, 0)
    got = db.score(qb)
    assert [int(x) for x in got["id"]] == [e[0] for e in expected]
    assert got["words"].tolist() == [e[1] for e in expected] and got["first"].tolist() == [e[2] for e in expected]
    assert D.u64(got["score"]).tolist() == D.u64(np.array([e[3] for e in expected])).tolist()
    for i, r in enumerate(res):
        assert D.u64(v.score(qb, (r["bow"][0], r["bow"][1]))) == D.u64(scores[i])


def test_product_equals_golden_reference_vocabulary(orbx):
    """The vocabulary the reference's create() trained and saveToTextFile wrote (tests/golden/dbow/k6_L3.txt, unbalanced as
    k-means leaves it, final newline included) and the reference's results on it: loader, descent, vectors and scores."""
    path, runs, load, scores = D.golden_fixture()
    v = orbx.ORBVocabulary(path)
    assert info(v) == {k: load[k] for k in info(v)}
    voc = D.parse_vocabulary_text(path)
    shallow = 0
    for r, (feat, levelsup, res) in enumerate(runs):
        shallow += int((~D.check_run("golden run %d" % r, voc, feat, levelsup, product(v, feat, levelsup), res)).sum())
    assert shallow > 0
    for a, b, s in scores:
        pa, pb = runs[a][2]["bow"], runs[b][2]["bow"]
        assert D.u64(v.score((np.ascontiguousarray(pa[0], np.int32), pa[1]), (np.ascontiguousarray(pb[0], np.int32), pb[1]))) == D.u64(s)
