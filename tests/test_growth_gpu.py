"""Growth of the matcher-side handles from their smallest size: every call below finds the handle too small, grows it and must
return what the oracle (or a handle created with ample capacity) returns; the same call again allocates nothing and must return
the same.  Random descriptors and keypoints, fixed seeds."""
import numpy as np
import pytest

import frustum_oracle as F
import kfdb_oracle as K
import mappoint_oracle as MP
import oracle_lib as O
from test_vocabulary import make_vocabulary, oracle_transform

pytestmark = pytest.mark.gpu
W, H = 640.0, 480.0


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes(), "%s: output %d differs" % (what, i)


def _twice(call, want, what):
    first = call()
    _same(first, want, what)
    _same(call(), first, what + " (second call)")
    return first


def _keypoints(orbx, rng, n):
    k = np.zeros(n, orbx.KP_DTYPE)
    k["x"] = rng.uniform(0, W, n).astype(np.float32); k["y"] = rng.uniform(0, H, n).astype(np.float32)
    k["octave"] = rng.integers(0, 8, n)
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    return k


def _windows(rng, n):
    x = rng.uniform(-20, W + 20, n).astype(np.float32); y = rng.uniform(-20, H + 20, n).astype(np.float32)
    r = rng.uniform(5, 120, n).astype(np.float32)
    mn = rng.integers(-1, 4, n).astype(np.int32); mx = np.where(rng.random(n) < 0.5, -1, mn + 3).astype(np.int32)
    return x, y, r, mn, mx


def _area(grid, win):
    off, idx = [0], []
    for x, y, r, mn, mx in zip(*win):
        idx.extend(grid.features_in_area(float(x), float(y), float(r), int(mn), int(mx)).tolist())
        off.append(len(idx))
    return np.array(off, np.int32), np.array(idx, np.int32)


def test_matcher_grows_from_the_smallest_handle(orbx):
    rng = np.random.default_rng(2024)
    m = orbx.ORBmatcher(max_queries=1, max_train=1, max_pairs=0)
    big = orbx.ORBmatcher()
    desc = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)

    # dense best2: d_q, d_t, d_out and the partials
    q, t = desc(40), desc(48)
    _twice(lambda: m.best2(q, t), O.best2(q, t), "dense best2")

    # CSR best2 / distances, three candidates per query: d_off, d_idx
    off = np.arange(0, 3 * 40 + 1, 3, dtype=np.int32)
    idx = rng.integers(0, 48, 3 * 40).astype(np.int32)
    _twice(lambda: m.best2(q, t, off, idx), O.best2(q, t, off, idx), "CSR best2")
    _twice(lambda: (m.distances(q, t, off, idx),), (big.distances(q, t, off, idx),), "CSR distances")

    # grid of 200 keypoints: 200 x 28 bytes do not fit d_out, the keypoints go through the temporary staging block
    kps, tdesc = _keypoints(orbx, rng, 200), desc(200)
    m.grid_build(kps, 0.0, W, 0.0, H)
    assert m.grid_count() == 200
    grid = O.FrameGrid(kps, 0.0, W, 0.0, H)
    win, qd = _windows(rng, 16), desc(16)
    _twice(lambda: m.GetFeaturesInArea(*win), _area(grid, win), "GetFeaturesInArea")
    _twice(lambda: m.search_area_best2(qd, *win, tdesc), grid.search_area_best2(qd, *win, tdesc), "search_area_best2")
    assert m.grid_count() == 200

    # MapPoint scratch; the run of 70 rows reaches the wave kernel
    doff, ddesc = MP.batch_from_lengths(rng, [1, 2, 3, 9, 70])
    _twice(lambda: m.distinctive_descriptors(doff, ddesc), MP.distinctive_descriptors(doff, ddesc), "distinctive_descriptors")

    sc = F.make_scene(rng, 64)
    want = F.frustum(*sc.args(), 0.5)
    got = _twice(lambda: m.frustum(*sc.args(), 0.5)[:6], want[:6], "frustum")
    assert len(got) == 6 and m.frustum(*sc.args(), 0.5)[6] == want[6]
    assert m.grid_count() == 200                        # none of these grew max_train

    # 500 keypoints: max_train grows inside the call, both grid slots are dropped and slot 1 is rebuilt
    kps, tdesc = _keypoints(orbx, rng, 500), desc(500)
    m.grid_build(kps, 0.0, W, 0.0, H)
    assert m.grid_count() == 500
    grid = O.FrameGrid(kps, 0.0, W, 0.0, H)
    _twice(lambda: m.search_area_best2(qd, *win, tdesc), grid.search_area_best2(qd, *win, tdesc), "search_area_best2 after the growth")
    _same(m.best2(q, t), O.best2(q, t), "dense best2 after everything")
    m.close(); big.close()


def test_vocabulary_staging_grows_once(orbx, tmp_path):
    path = str(tmp_path / "voc.txt")
    voc = make_vocabulary(path, k=6, depth=3, seed=7)
    v = orbx.ORBVocabulary(path)
    rng = np.random.default_rng(7)
    for n in (10, 300, 10):
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        _same(v.transform_features(d, 2), oracle_transform(voc, d, 2)[0], "transform_features(%d)" % n)
    v.close()


def test_keyframe_database_compacts_and_moves_from_the_minimum(orbx):
    rng = np.random.default_rng(11)
    nw = 400
    db, oracle = orbx.KeyFrameDatabase(nw, max_keyframes=0, max_entries=0), K.KeyFrameDatabase(nw)
    for k in range(1, 13):                              # 4 slots / 256 entries at creation: the fifth add compacts and moves
        ids = np.sort(rng.choice(nw, 30, replace=False)).astype(np.int32)
        v = rng.random(30) + 1e-3
        db.add(k, (ids, v / v.sum())); oracle.add(k, (ids, v / v.sum()))
    for k in (2, 7, 12):
        db.erase(k); oracle.erase(k)
    assert len(db) == 9
    live = [k for k in range(1, 13) if k not in (2, 7, 12)]
    covis = {k: [j for j in live if j != k][:10] for k in live}
    for i in range(3):
        ids = np.sort(rng.choice(nw, 60, replace=False)).astype(np.int32)
        q = (ids, np.full(60, 1.0 / 60))
        ids_got, si = db.query_begin(orbx.ORBK_RELOC, 100 + i, q)
        exp, mc = oracle.query_begin(False, 100 + i, q)
        assert len(exp) > 0 and [int(x) for x in ids_got] == [k for _, k in exp]
        assert si.view(np.uint32).tolist() == np.array([s for s, _ in exp], np.float32).view(np.uint32).tolist()     # scores, bit for bit
        assert db.query_end(orbx.ORBK_RELOC, ids_got, covis) == oracle.query_end(False, 100 + i, exp, mc, covis)
        assert db.DetectLoopCandidates(200 + i, q, live[:2], 0.0, covis) == oracle.DetectLoopCandidates(200 + i, q, live[:2], 0.0, covis)
    db.close()
