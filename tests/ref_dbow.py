"""Client of oracle/_ref/ref_dbow (the reference's own Thirdparty/DBoW2, compiled unmodified on the OpenCV shim; request and
response formats in oracle/ref/ref_dbow.cc), and the case list of tests/test_reference_pin_dbow_cpu.py and _gpu.py.

Every planted case proves itself: descend() is a plain numpy walk of the node table that counts, per feature, exact ties for
the minimum, winners in the second or third 64-child trip and the leaf depth.  It is used only for those counts and for the
"leaf deep enough for a node id" mask, never as an expected result."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from test_vocabulary import make_vocabulary, make_vocabulary_tree, write_vocabulary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(REF_OUT, "ref_dbow")
EXE_UBSAN = os.path.join(REF_OUT, "ref_dbow_ubsan")
TIMEOUT = 120          # seconds; the reference's loader can spin forever on a bad file, so no run goes without one

LOAD, TRANSFORM, SCORE, CREATE = range(4)
NID_UNSET = 0xFFFFFFFF


def ensure(allow_build=True):
    """Path to ref_dbow, building it when it is missing and the reference exists; None when neither exists."""
    if os.path.exists(EXE) and os.path.exists(EXE_UBSAN):
        return EXE
    import ref_pin
    if allow_build and os.path.exists(os.path.join(ref_pin.reference_dir(), "Thirdparty", "DBoW2", "DBoW2", "TemplatedVocabulary.h")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref"), "dbow"])
        return EXE
    return None


# ---- requests

def req_load(path):
    p = os.fsencode(path)
    return LOAD, struct.pack("<ii", LOAD, len(p)) + p


def req_transform(feat, levelsup):
    feat = np.ascontiguousarray(feat, np.uint8).reshape(-1, 32)
    return (TRANSFORM, len(feat)), struct.pack("<iii", TRANSFORM, levelsup, len(feat)) + feat.tobytes()


def _bow_bytes(b):
    ids, vals = np.ascontiguousarray(b[0], "<u4"), np.ascontiguousarray(b[1], "<f8")
    assert len(ids) == len(vals)
    return struct.pack("<i", len(ids)) + ids.tobytes() + vals.tobytes()


def req_score(pairs):
    return (SCORE, len(pairs)), struct.pack("<ii", SCORE, len(pairs)) + b"".join(_bow_bytes(a) + _bow_bytes(b) for a, b in pairs)


def req_create(seed, k, L, weighting, scoring, images, out_path):
    b = struct.pack("<iiiiiii", CREATE, seed, k, L, weighting, scoring, len(images))
    for im in images:
        im = np.ascontiguousarray(im, np.uint8).reshape(-1, 32)
        b += struct.pack("<i", len(im)) + im.tobytes()
    p = os.fsencode(out_path)
    return CREATE, b + struct.pack("<i", len(p)) + p


class _Reader:
    def __init__(self, data):
        self.d, self.o = data, 0

    def arr(self, dtype, n):
        dt = np.dtype(dtype)
        assert self.o + dt.itemsize * n <= len(self.d), "truncated ref_dbow response"
        v = np.frombuffer(self.d, dt, n, self.o).copy()
        self.o += dt.itemsize * n
        return v

    def i32(self):
        return int(self.arr("<i4", 1)[0])


def _parse(what, r):
    mode = what if isinstance(what, int) else what[0]
    assert r.i32() == mode, "response out of step"
    if mode == LOAD:
        k, L, scoring, weighting, nn, nwords = (r.i32() for _ in range(6))
        out = dict(k=k, L=L, scoring=scoring, weighting=weighting, nnodes=nn, nwords=nwords)
        out["parent"] = r.arr("<i4", nn); out["leaf"] = r.arr("<i4", nn).astype(bool); out["word_of"] = r.arr("<i4", nn)
        out["weight"] = r.arr("<f8", nn); out["desc"] = r.arr(np.uint8, nn * 32).reshape(nn, 32)
        nch = r.arr("<i4", nn)
        out["child_off"] = np.concatenate([[0], np.cumsum(nch)]).astype(np.int32)
        out["child_ids"] = r.arr("<u4", int(nch.sum())).astype(np.int32)
        return out
    if mode == TRANSFORM:
        n = what[1]
        out = dict(word=r.arr("<u4", n), weight=r.arr("<f8", n), node=r.arr("<u4", n))
        nb = r.i32()
        out["bow"] = (r.arr("<u4", nb).astype(np.int32), r.arr("<f8", nb))
        fv = []
        for _ in range(r.i32()):
            nid = int(r.arr("<u4", 1)[0])
            fv.append((nid, r.arr("<u4", r.i32()).astype(np.int32)))
        out["fv"] = fv
        return out
    if mode == SCORE:
        return r.arr("<f8", what[1])
    return r.arr(np.uint8, r.i32()).tobytes()


def run(requests, exe=None):
    """One ref_dbow process for a list of requests; returns one parsed result per request.  A non-zero exit raises
    CalledProcessError (status 2: the driver refused the request; the UBSan build exits at the first undefined operation)."""
    exe = exe or EXE
    with tempfile.TemporaryDirectory(prefix="ref_dbow_") as d:
        req, resp = os.path.join(d, "req.bin"), os.path.join(d, "resp.bin")
        with open(req, "wb") as f:
            f.write(struct.pack("<ii", 0x51574244, len(requests)))
            for _, blob in requests:
                f.write(blob)
        p = subprocess.run([exe, req, resp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
        if p.returncode != 0:
            raise subprocess.CalledProcessError(p.returncode, [exe], p.stdout, p.stderr)
        with open(resp, "rb") as f:
            r = _Reader(f.read())
    assert r.i32() == 0x52574244
    out = [_parse(what, r) for what, _ in requests]
    assert r.o == len(r.d), "trailing bytes in the ref_dbow response"
    return out


# ---- the numpy walk behind the self-proofs

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(f, D):
    return _POP[np.bitwise_xor(D, f)].sum(axis=-1)


def descend(voc, feat):
    """Per feature: leaf depth, whether some level of its descent had two or more children at exactly the minimum distance,
    and whether some level's winner was a child of position >= 64 (found only in a later trip of a 64-lane loop)."""
    off, ids, D = voc["child_off"], voc["child_ids"], voc["desc"]
    n = len(feat)
    depth = np.zeros(n, np.int32); tie = np.zeros(n, bool); late = np.zeros(n, bool)
    for i in range(n):
        node = 0
        while off[node + 1] > off[node]:
            ch = ids[off[node]:off[node + 1]]
            d = hamming(feat[i], D[ch])
            m = d.min()
            tie[i] |= int((d == m).sum()) > 1
            first = int(np.argmax(d == m))
            late[i] |= first >= 64
            node = int(ch[first])
            depth[i] += 1
    return depth, tie, late


# ---- planting

def flip(d, bits):
    d = np.array(d, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def children(voc, node):
    return voc["child_ids"][voc["child_off"][node]:voc["child_off"][node + 1]]


def path_to(voc, node):
    p = []
    while node != 0:
        p.append(node)
        node = int(voc["parent"][node])
    return p[::-1]


def pin_path(voc, node, rng):
    """Makes `node` reachable: every node on the way from the root takes its parent's descriptor with 6 bits flipped (the
    root's children keep theirs), so a feature near `node` is ~12 bits from each of them and ~128 from their siblings.  A
    descriptor that an earlier plant settled (voc["fixed"]) is never rewritten."""
    fixed = voc.setdefault("fixed", set())
    p = path_to(voc, node)
    fixed.add(p[0])
    for a, b in zip(p, p[1:]):
        if b not in fixed:
            voc["desc"][b] = flip(voc["desc"][a], rng.choice(256, 6, replace=False))
            fixed.add(b)


def plant_tie(voc, parent, i, j, t, rng, identical=False):
    """Children number i < j of `parent` end up at exactly distance t from the returned feature, every other child far away.
    identical: the two are the same descriptor; otherwise they differ in two bits (t >= 1)."""
    ch = children(voc, parent)
    assert i < j < len(ch)
    ci, cj = int(ch[i]), int(ch[j])
    pin_path(voc, ci, rng)
    assert cj not in voc["fixed"], "child %d of node %d is already planted" % (j, parent)
    bits = rng.choice(256, t + 1, replace=False)
    A, x = bits[:t], bits[t]
    f = flip(voc["desc"][ci], A)
    voc["desc"][cj] = voc["desc"][ci] if identical else flip(voc["desc"][ci], [A[0], x])
    voc["fixed"].add(cj)
    return f


# ---- cases

class Case:
    """One vocabulary file and the (features, levelsup) runs on it.  min_ties / min_late / min_deep are what the case
    planted: lower bounds on what descend() must count over the features of all runs (ties as a count, winners of position
    >= 64 as a share; min_deep maps a levelsup to the share of a run's features whose leaf is deep enough for a node id)."""

    def __init__(self, name, voc, runs, min_ties=0, min_late=0.0, min_deep=None, trailing_newline=True, n_planted=0):
        self.name, self.voc, self.runs = name, voc, [(np.ascontiguousarray(f, np.uint8).reshape(-1, 32), int(l)) for f, l in runs]
        self.min_ties, self.min_late, self.min_deep, self.trailing_newline = min_ties, min_late, min_deep, trailing_newline
        self.n_planted = n_planted          # the first n_planted features of every run each meet a planted tie
        self.path = None

    def write(self, d):
        self.path = os.path.join(d, self.name + ".txt")
        write_vocabulary(self.path, self.voc, self.trailing_newline)
        return self

    def requests(self):
        return [req_load(self.path)] + [req_transform(f, l) for f, l in self.runs]

    def deep_mask(self, run):
        """Features of run whose leaf is at least as deep as the level the node id is taken at (all, when that is the root)."""
        f, l = self.runs[run]
        depth, _, _ = descend(self.voc, f)
        return depth >= self.voc["L"] - l


def noisy_leaves(voc, rng, n, flips=12):
    """n features: half random bytes, half copies of random nodes with a few bits flipped (they spread over the tree)."""
    f = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pick = rng.integers(1, voc["nnodes"], n)
    for i in range(0, n, 2):
        f[i] = flip(voc["desc"][pick[i]], rng.choice(256, flips, replace=False))
    return f


SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 3000)     # a block is 4 waves, one wave per feature


def _wide_children(level, o):
    if level == 0:
        return 130
    if level == 1:
        return (130, 64, 20, 2, 1, 65, 0)[o % 7] if o < 21 else 0
    return (2, 0, 1)[o % 3] if o < 60 else 0


def _unbalanced_children(seed):
    r = np.random.default_rng(seed)

    def f(level, o):
        if level == 0:
            return 6
        return 0 if r.uniform() < 0.25 else int(r.integers(1, 7))
    return f


def build_cases():
    """The case list, in memory; Case.write(dir) puts a case's file on disk."""
    rng = np.random.default_rng(2024)
    cases = []

    # sizes at the 4-waves-per-block edges, on a complete 10-ary tree of depth 3 (the shape of ORBvoc.txt, smaller)
    voc = make_vocabulary_tree(10, 3, lambda l, o: 10, seed=11)
    cases.append(Case("sizes_k10_L3", voc, [(noisy_leaves(voc, rng, n), 2) for n in SIZES]))

    # depth 1: all words under the root; depth 10 with k = 2
    voc = make_vocabulary_tree(20, 1, lambda l, o: 20, seed=12)
    cases.append(Case("depth1_k20", voc, [(noisy_leaves(voc, rng, 257), l) for l in (0, 1, 2)]))
    voc = make_vocabulary_tree(2, 10, lambda l, o: 2, seed=13)
    cases.append(Case("depth10_k2", voc, [(noisy_leaves(voc, rng, 300), l) for l in (0, 4, 9, 10, 11)]))

    # levelsup 0, 1, L-1, L, L+1 on a complete tree
    voc = make_vocabulary_tree(5, 3, lambda l, o: 5, seed=14)
    cases.append(Case("levelsup_k5_L3", voc, [(noisy_leaves(voc, rng, 300), l) for l in (0, 1, 2, 3, 4)]))

    # unbalanced: leaves at depth 1..L, nodes with 1 child.  The reference leaves nid unset for a leaf above the nid level.
    for s, L in ((21, 4), (22, 3)):
        voc = make_vocabulary_tree(6, L, _unbalanced_children(s), seed=s)
        lv = sorted(set([0, 1, L - 1, L, L + 1]))
        cases.append(Case("unbalanced_s%d_L%d" % (s, L), voc, [(noisy_leaves(voc, rng, 400), l) for l in lv],
                          min_deep={0: 0.10, 1: 0.25}))

    # nodes with 130 (the root), 65, 64, 20, 2 and 1 children under a header k of 20: two and three trips of 64
    voc = make_vocabulary_tree(20, 3, _wide_children, seed=31)
    cases.append(Case("wide_65_130", voc, [(noisy_leaves(voc, rng, 1200), l) for l in (0, 1, 2)], min_late=0.30,
                      min_deep={0: 0.01, 1: 0.15}))

    # planted ties on the wide tree: the first child must win each one.  (parent, i, j, distance): children i and j tie.
    voc = make_vocabulary_tree(20, 3, _wide_children, seed=32)
    rc = [int(c) for c in children(voc, 0)]
    n130, n64, n20, n2, n65a, n130b, n65b, n65c = rc[0], rc[1], rc[2], rc[3], rc[5], rc[7], rc[12], rc[19]
    assert [len(children(voc, x)) for x in (n130, n64, n20, n2, n65a, n130b, n65b, n65c)] == [130, 64, 20, 2, 65, 130, 65, 65]
    plan = [(0, 21, 64, 3), (0, 30, 31, 2), (0, 22, 60, 4), (0, 63, 65, 2), (0, 100, 129, 3),    # the root: 130 children, these are leaves
            (n130, 0, 129, 4), (n130, 10, 100, 2), (n130, 70, 128, 3), (n130, 63, 64, 3), (n130, 126, 127, 1), (n130, 65, 66, 2),
            (n65a, 0, 64, 4), (n65b, 63, 64, 2), (n65c, 31, 64, 1),
            (n64, 0, 63, 3), (n64, 30, 31, 1), (n20, 0, 19, 4), (n20, 7, 8, 2), (n2, 0, 1, 4)]
    feats = [plant_tie(voc, parent, i, j, t, rng) for parent, i, j, t in plan]
    # two identical siblings, at distance 3 and at distance 0, in one trip and across two
    same = [(n130b, 5, 90, 3), (n130b, 20, 21, 0), (n130b, 64, 128, 0)]
    feats += [plant_tie(voc, parent, i, j, t, rng, identical=True) for parent, i, j, t in same]
    # distance 0 without a tie, and distance 256 to the same child: a feature equal to a root child, and its bit complement
    feats += [voc["desc"][rc[40]].copy(), ~voc["desc"][rc[40]]]
    n_tie = len(plan) + len(same)
    cases.append(Case("ties", voc, [(np.concatenate([np.array(feats, np.uint8), noisy_leaves(voc, rng, 64)]), l) for l in (0, 1, 2)],
                      min_ties=3 * n_tie, min_late=0.20, n_planted=n_tie))

    # distance 256 as the minimum: the root's two children are identical and the feature is their complement (a tie at 256,
    # and at 0 for the children's own descriptor); and a root with one child, whose complement has no other way to go
    voc = make_vocabulary_tree(2, 2, lambda l, o: 2, seed=33)
    voc["desc"][2] = voc["desc"][1]
    cases.append(Case("complement_identical_root", voc, [(np.concatenate([[~voc["desc"][1], voc["desc"][1]], noisy_leaves(voc, rng, 6)]), l)
                                                         for l in (0, 1)], min_ties=4, n_planted=2))
    voc = make_vocabulary_tree(2, 2, lambda l, o: 1 if l == 0 else 2, seed=34)
    cases.append(Case("complement_one_child_root", voc, [(np.concatenate([[~voc["desc"][1]], noisy_leaves(voc, rng, 7)]), 1)]))

    # stopped words: a fifth of them, and all of them (empty BowVector and FeatureVector, norm 0: no division)
    voc = make_vocabulary_tree(6, 2, lambda l, o: 6, seed=41, stop=0.2)
    cases.append(Case("stop_some", voc, [(noisy_leaves(voc, rng, 300), 1)]))
    for scoring in (0, 1, 5):
        voc = make_vocabulary_tree(6, 2, lambda l, o: 6, seed=42, stop=1.1, scoring=scoring)
        assert not voc["weight"].any()
        cases.append(Case("stop_all_s%d" % scoring, voc, [(noisy_leaves(voc, rng, 100), 1)]))

    # weighting x scoring: L1, L2 and DOT_PRODUCT (the one that does not normalise) with all four weightings, and one case
    # each of the other three scoring types, which normalise as L1.  300 features on 16 words: every word repeats.
    combos = [(w, s) for s in (0, 1, 5) for w in range(4)] + [(0, 2), (0, 3), (1, 4)]
    for w, s in combos:
        voc = make_vocabulary_tree(4, 2, lambda l, o: 4, seed=50, scoring=s, weighting=w, stop=0.1)
        cases.append(Case("weighting%d_scoring%d" % (w, s), voc, [(noisy_leaves(voc, rng, 300), 1), (noisy_leaves(voc, rng, 40), 1)]))

    # the file without its final newline: the product must read both spellings alike
    voc = make_vocabulary_tree(5, 2, lambda l, o: 5, seed=60)
    cases.append(Case("no_final_newline", voc, [(noisy_leaves(voc, rng, 100), 1)], trailing_newline=False))
    return cases


def score_pairs(results):
    """BowVector pairs for SCORE from a case's TRANSFORM results: each against the next, one against itself, two with no common
    word (the even and the odd entries of one vector), an empty one on either side and two empty ones."""
    bows = [r["bow"] for r in results]
    pairs = [(bows[i], bows[(i + 1) % len(bows)]) for i in range(len(bows))]
    b = max(bows, key=lambda x: len(x[0]))
    pairs.append((b, b))
    pairs.append(((b[0][0::2], b[1][0::2]), (b[0][1::2], b[1][1::2])))
    e = (np.zeros(0, np.int32), np.zeros(0, np.float64))
    pairs += [(b, e), (e, b), (e, e)]
    return pairs


def fv_per_feature(fv, n):
    """FeatureVector -> node id per feature (-1: not listed), after checking the map's order and each list's order."""
    node = np.full(n, -1, np.int64)
    ids = [nid for nid, _ in fv]
    assert ids == sorted(set(ids)), "FeatureVector node ids are not strictly ascending"
    for nid, idx in fv:
        assert len(idx) and (np.diff(idx) > 0).all(), "features of node %d are not in ascending order" % nid
        assert (node[idx] == -1).all()
        node[idx] = nid
    return node


def csr_to_fv(nids, off, idx):
    return [(int(nids[j]), np.asarray(idx[off[j]:off[j + 1]], np.int32)) for j in range(len(nids))]


# ---- comparisons shared by the CPU (oracle) and the GPU (product) pins

def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_run(tag, voc, feat, levelsup, got, ref):
    """got = ((word, node, weight), (ids, vals), (node_ids, off, idx)) of the code under test; ref = a TRANSFORM result.
    Word ids, weights and the BowVector are compared for every feature; node ids and FeatureVector membership where the
    reference defines them (leaf depth >= L - levelsup), and there the reference must have left its node id unset exactly
    where the walk says the leaf is too shallow."""
    (w, nd, wt), (ids, vals), (nids, off, idx) = got
    n = len(feat)
    assert len(w) == len(nd) == len(wt) == n == len(ref["word"]), tag
    assert np.array_equal(w, ref["word"].astype(np.int64)), "%s: word ids differ at %s" % (tag, np.nonzero(w != ref["word"])[0][:8])
    assert np.array_equal(u64(wt), u64(ref["weight"])), "%s: weights differ" % tag
    depth, _, _ = descend(voc, feat)
    deep = depth >= voc["L"] - levelsup
    assert np.array_equal(ref["node"] != NID_UNSET, deep), "%s: the reference sets nid on other features than the walk predicts" % tag
    assert np.array_equal(nd[deep], ref["node"][deep].astype(np.int64)), "%s: node ids differ at %s" % (
        tag, np.nonzero(deep)[0][nd[deep] != ref["node"][deep]][:8])
    assert not nd[~deep].any(), "%s: a leaf above the nid level must give node id 0 (include/orbv.h)" % tag
    assert np.array_equal(ids, ref["bow"][0]), "%s: BowVector word ids differ" % tag
    assert np.array_equal(u64(vals), u64(ref["bow"][1])), "%s: BowVector values differ: %s vs reference %s" % (tag, vals[:4], ref["bow"][1][:4])
    assert (np.diff(ids) > 0).all()
    got_node, ref_node = fv_per_feature(csr_to_fv(nids, off, idx), n), fv_per_feature(ref["fv"], n)
    assert np.array_equal(got_node >= 0, wt > 0) and np.array_equal(ref_node >= 0, wt > 0), "%s: FeatureVector lists other features than the unstopped ones" % tag
    assert np.array_equal(got_node[deep], ref_node[deep]), "%s: FeatureVector nodes differ" % tag
    if deep.all():
        assert [x for x, _ in csr_to_fv(nids, off, idx)] == [x for x, _ in ref["fv"]], tag
    return deep


def parse_vocabulary_text(path):
    """A third, plain reading of the text format (empty lines skipped, as include/orbv.h documents): vocabulary_arrays' dict."""
    from test_vocabulary import vocabulary_arrays
    with open(path) as f:
        lines = [l.split() for l in f.read().split("\n")]
    k, L, scoring, weighting = (int(x) for x in lines[0])
    rows = [l for l in lines[1:] if l]
    assert all(len(r) == 35 for r in rows)
    return vocabulary_arrays(k, L, scoring, weighting, [int(r[0]) for r in rows], [int(r[1]) > 0 for r in rows],
                             [[int(x) for x in r[2:34]] for r in rows], [float(r[34]) for r in rows])


def check_load(tag, voc, ref):
    """The node table a test built (or parsed) against LOAD."""
    for key in ("k", "L", "scoring", "weighting", "nnodes", "nwords"):
        assert voc[key] == ref[key], "%s: %s is %s, reference %s" % (tag, key, voc[key], ref[key])
    for key in ("parent", "leaf", "child_off", "child_ids", "desc"):
        assert np.array_equal(voc[key], ref[key]), "%s: %s differs" % (tag, key)
    lf = ref["leaf"]
    assert not lf[0] and np.array_equal(voc["word_of"][lf], ref["word_of"][lf]), "%s: word ids differ" % tag
    assert np.array_equal(u64(voc["weight"]), u64(ref["weight"])), "%s: weights differ" % tag


def pinned_cases(d, build=False):
    """(cases written under d, {name: (LOAD result, [TRANSFORM result per run])}) from one ref_dbow process; None when the
    binary is absent (and, with build, cannot be built)."""
    if (ensure() if build else (EXE if os.path.exists(EXE) and os.access(EXE, os.X_OK) else None)) is None:
        return None
    cases = [c.write(d) for c in build_cases()]
    it = iter(run([r for c in cases for r in c.requests()]))
    return cases, {c.name: (next(it), [next(it) for _ in c.runs]) for c in cases}


def golden_fixture():
    """tests/golden/dbow/k6_L3.*: (path of the text file, [(features, levelsup, TRANSFORM result)], LOAD result,
    [(run a, run b, score)]), as tests/golden/make_golden_dbow.py stored them."""
    g = os.path.join(ROOT, "tests", "golden", "dbow")
    z = np.load(os.path.join(g, "k6_L3.npz"))
    o, b, fo, fi = z["run_off"], z["bow_off"], z["fv_off"], z["fv_idx_off"]
    runs = []
    for r, levelsup in enumerate(z["levelsup"]):
        fv = [(int(z["fv_node"][j]), z["fv_idx"][fi[j]:fi[j + 1]]) for j in range(fo[r], fo[r + 1])]
        res = dict(word=z["word"][o[r]:o[r + 1]], weight=z["weight"][o[r]:o[r + 1]], node=z["node"][o[r]:o[r + 1]],
                   bow=(z["bow_ids"][b[r]:b[r + 1]], z["bow_vals"][b[r]:b[r + 1]]), fv=fv)
        runs.append((z["features"][o[r]:o[r + 1]], int(levelsup), res))
    load = {k[5:]: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("load_")}
    scores = [(int(a), int(c), s) for (a, c), s in zip(z["score_pairs"], z["scores"])]
    return os.path.join(g, "k6_L3.txt"), runs, load, scores
