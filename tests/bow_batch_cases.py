"""Inputs of the batched SearchByBoW tests (orbm_search_by_bow_batch / orbm_search_by_bow_kf_batch, include/orbm.h).  Seeded numpy,
no extractor and no vocabulary: descriptors are random bits, FeatureVectors are built by hand.

A case is one shared side and a list of candidates.  `variant` says which call it is for:
    "frame"   Relocalization: the candidates are key frames (the SERIAL side of the walk), the shared side is the frame (LANES)
    "kf"      ComputeSim3: the shared side is key frame 1 (SERIAL), the candidates are the key frames 2 (LANES)
A candidate's descriptors are copies of a random subset of the shared side's with 0 to 30 flipped bits, in the node of their
source, plus unrelated random ones.  Its angles are the source's plus one rotation per candidate plus a small jitter, with a few
outliers, so that the histogram cull has something to remove.

Planted on top, each in a node of its own:
    contest   two serial-side features (list order s1, s2), both within TH_LOW of one lane-side feature whose node-mates are far:
              s1 takes it (:209 makes s2 skip it), s2 gets nothing
    tie "dup"    two identical lane-side features: best == second best, the ratio test fails for every nnratio <= 1: no match;
                 with nnratio > 1 the first in the list is taken
    tie "equal"  two different lane-side features at the same distance: the same, the first in the list being the one `<` keeps
The oracle (tests/oracle_lib.py) is called once per candidate: oracle(case)."""
import numpy as np

import oracle_lib as O

TH_LOW = 50
FAR_NODE = 1 << 20          # node ids from here on exist in one side only


class Side:
    def __init__(self, kps, desc, fv, valid):
        self.kps, self.desc, self.fv, self.valid = kps, desc, fv, valid

    def __len__(self):
        return len(self.desc)

    @property
    def angle(self):
        return np.ascontiguousarray(self.kps["angle"])

    def tup(self):
        return (self.kps, self.desc, self.fv, self.valid)


class Builder:
    """Features are added as (node, descriptor, angle, valid) and get a handle; build() gives them shuffled indices, while the order
    inside a node's list stays the order of the add() calls."""

    def __init__(self, rng):
        self.rng, self.rows = rng, []

    def add(self, node, desc, angle, valid=1):
        self.rows.append((int(node), np.asarray(desc, np.uint8), float(angle), int(valid)))
        return len(self.rows) - 1

    def build(self, valid="mask"):
        n = len(self.rows)
        at = self.rng.permutation(n).astype(np.int32)          # handle -> feature index
        desc = np.zeros((n, 32), np.uint8)
        kps = np.zeros(n, O.KP_DTYPE)
        val = np.ones(n, np.uint8)
        lists = {}
        for h, (node, d, a, v) in enumerate(self.rows):
            desc[at[h]] = d
            kps["angle"][at[h]] = np.float32(a % 360.0) if np.float32(a % 360.0) < 360 else np.float32(0)
            kps["octave"][at[h]] = h % 8
            val[at[h]] = v
            lists.setdefault(node, []).append(at[h])
        nodes = sorted(lists)
        off = np.zeros(len(nodes) + 1, np.int32)
        off[1:] = np.cumsum([len(lists[k]) for k in nodes])
        idx = np.array([i for k in nodes for i in lists[k]], np.int32).reshape(-1)
        if valid == "zero":
            val[:] = 0
        elif valid == "ones":
            val[:] = 1
        side = Side(kps, desc, (np.array(nodes, np.int32), off, idx), None if valid == "none" else val)
        return side, at


def flip(rng, desc, k):
    d = np.unpackbits(np.asarray(desc, np.uint8))
    d[rng.choice(256, size=k, replace=False)] ^= 1
    return np.packbits(d)


def flip_bits(desc, bits):
    d = np.unpackbits(np.asarray(desc, np.uint8))
    d[list(bits)] ^= 1
    return np.packbits(d)


class Case:
    def __init__(self, name, variant, shared, cands, nnratio, check_ori, contests=(), ties=()):
        self.name, self.variant, self.shared, self.cands = name, variant, shared, cands
        self.nnratio, self.check_ori = nnratio, check_ori
        self.contests = list(contests)      # (candidate, s1, s2, lane feature): indices of the built sides
        self.ties = list(ties)              # (candidate, serial feature, first lane feature, second lane feature)

    def with_params(self, nnratio, check_ori):
        return Case(self.name, self.variant, self.shared, self.cands, nnratio, check_ori, self.contests, self.ties)

    def first(self, k):
        return Case(self.name, self.variant, self.shared, self.cands[:k], self.nnratio, self.check_ori,
                    [c for c in self.contests if c[0] < k], [t for t in self.ties if t[0] < k])


def oracle_one(case, cand):
    """(row of the table over the shared side's features, count) of one candidate, from the CPU oracle"""
    s = case.shared
    if case.variant == "frame":
        return O.search_by_bow(cand.desc, cand.angle, cand.fv, s.desc, s.angle, s.fv, case.nnratio, case.check_ori, valid_kf=cand.valid)
    return O.search_by_bow_kf(s.desc, s.angle, s.valid, s.fv, cand.desc, cand.angle, cand.valid, cand.fv, case.nnratio, case.check_ori)


def oracle(case):
    n = len(case.shared)
    table = np.full((len(case.cands), n), -1, np.int32)
    counts = np.zeros(len(case.cands), np.int32)
    for c, cand in enumerate(case.cands):
        if len(cand) == 0 and case.variant == "frame":          # nothing to visit: the reference's loop body never runs
            continue
        table[c], counts[c] = oracle_one(case, cand)
    return table, counts


def pairs_of(case, row):
    """the matches of one table row as a set of (serial-side feature, lane-side feature)"""
    hit = np.nonzero(row >= 0)[0]
    if case.variant == "frame":
        return {(int(row[i]), int(i)) for i in hit}
    return {(int(i), int(row[i])) for i in hit}


def node_sizes_many(rng, n):
    """about n / 3.4 nodes of 1 to 10 features"""
    w = 1.0 / np.arange(1, 11)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.choice(np.arange(1, 11), p=w / w.sum())), n - sum(sizes)))
    return sizes


def make_case(name, variant, seed, n_shared, sizes, cand_specs, nnratio=0.75, check_ori=True, contests=0, ties=False, dup_pairs=0):
    """sizes: the shared side's node sizes ("one" = a single node, "many" = about 100 small ones, or a list).
    cand_specs: per candidate a dict: n (features), copy (fraction that are copies, default 0.7), valid ("mask" | "none" | "zero" |
    "ones"), absent (True: every feature in a node the shared side does not have), nodes (only copy sources from these shared
    nodes), inside (True: the unrelated features go into the shared side's nodes too, so that with one shared node the candidate's
    list in that node has exactly n entries).
    contests: planted contests per candidate that has room for them; ties: plant both kinds of tie into candidate 0;
    dup_pairs: near-duplicate pairs inside the shared side (a contest for the kf variant, a failed ratio test for the frame one)."""
    rng = np.random.default_rng(seed)
    serial_shared = variant == "kf"
    if sizes == "one":
        sizes = [n_shared]
    elif sizes == "many":
        sizes = node_sizes_many(rng, n_shared)
    assert sum(sizes) == n_shared
    sb = Builder(rng)
    sh_node, sh_desc, sh_angle = [], [], []                     # by handle
    for k, sz in enumerate(sizes):
        for _ in range(sz):
            d, a = rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360)
            sh_node.append(3 + 7 * k); sh_desc.append(d); sh_angle.append(a)
            sb.add(3 + 7 * k, d, a, 1 if rng.random() > 0.08 else 0)
    next_node = [3 + 7 * len(sizes) + 100]

    def fresh_node():
        next_node[0] += 5
        return next_node[0]

    ncand = len(cand_specs)
    cbs = [Builder(rng) for _ in range(ncand)]
    rots = [rng.uniform(0, 360) for _ in range(ncand)]
    plan_contests, plan_ties = [], []                           # in handles; resolved after build()
    for c, spec in enumerate(cand_specs):
        n, frac = spec["n"], spec.get("copy", 0.7)
        ncopy = int(np.ceil(n * frac))
        pool = np.arange(n_shared) if "nodes" not in spec else np.array([h for h in range(n_shared) if sh_node[h] in spec["nodes"]])
        src = rng.choice(pool, size=min(ncopy, len(pool)), replace=False) if n else []
        rows = []
        for h in src:
            a = sh_angle[h] + rots[c] + rng.uniform(-3, 3) if rng.random() > 0.06 else rng.uniform(0, 360)
            rows.append((sh_node[h] if not spec.get("absent") else FAR_NODE + sh_node[h], flip(rng, sh_desc[h], int(rng.integers(0, 31))), a))
        while len(rows) < n:
            node = sh_node[int(rng.integers(0, n_shared))] if spec.get("inside") or rng.random() < 0.7 else FAR_NODE + int(rng.integers(0, 50))
            rows.append((FAR_NODE + node if spec.get("absent") else node, rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360)))
        for k in rng.permutation(len(rows)):
            node, d, a = rows[k]
            cbs[c].add(node, d, a, 1 if rng.random() > 0.08 else 0)
        if spec.get("absent") or spec.get("valid") == "zero" or n == 0:
            continue
        for _ in range(contests):                               # a node of its own: two serial features, one lane feature, two far lane mates
            node, base, a = fresh_node(), rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360)
            S, L = (sb, cbs[c]) if serial_shared else (cbs[c], sb)
            a_s, a_l = (a, a + rots[c]) if serial_shared else (a + rots[c], a)      # candidate angle = shared angle + rotation
            s1 = S.add(node, flip(rng, base, int(rng.integers(0, 12))), a_s)
            s2 = S.add(node, flip(rng, base, int(rng.integers(0, 12))), a_s)
            lane = L.add(node, base, a_l)
            for _ in range(2):
                L.add(node, rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360))
            plan_contests.append((c, s1, s2, lane))
        if ties and c == 0:
            for kind in ("dup", "equal"):
                node, base, a = fresh_node(), rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360)
                S, L = (sb, cbs[c]) if serial_shared else (cbs[c], sb)
                a_s, a_l = (a, a + rots[c]) if serial_shared else (a + rots[c], a)
                s = S.add(node, base, a_s)
                d1 = flip_bits(base, range(0, 9))
                d2 = d1 if kind == "dup" else flip_bits(base, range(9, 18))
                l1, l2 = L.add(node, d1, a_l), L.add(node, d2, a_l)
                L.add(node, rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360))
                plan_ties.append((c, s, l1, l2))
    for _ in range(dup_pairs):
        h = int(rng.integers(0, n_shared))
        sb.add(sh_node[h], flip(rng, sh_desc[h], 3), sh_angle[h])
    shared, s_at = sb.build("mask")
    cands, c_at = [], []
    for c, spec in enumerate(cand_specs):
        valid = spec.get("valid", "mask")
        if variant == "kf" and valid == "none":                 # the key-frame call needs a mask on both sides
            valid = "ones" if spec.get("inside") else "mask"
        side, at = cbs[c].build(valid)
        cands.append(side); c_at.append(at)
    # planted features are usable whatever the random masks say
    def usable(side, i):
        if side.valid is not None:
            side.valid[i] = 1
    cs, ts = [], []
    for c, s1, s2, lane in plan_contests:
        sa, la = (s_at, c_at[c]) if serial_shared else (c_at[c], s_at)
        for side, i in ((shared if serial_shared else cands[c], sa[s1]), (shared if serial_shared else cands[c], sa[s2]),
                        (cands[c] if serial_shared else shared, la[lane])):
            usable(side, i)
        cs.append((c, int(sa[s1]), int(sa[s2]), int(la[lane])))
    for c, s, l1, l2 in plan_ties:
        sa, la = (s_at, c_at[c]) if serial_shared else (c_at[c], s_at)
        usable(shared if serial_shared else cands[c], sa[s])
        for l in (l1, l2):
            usable(cands[c] if serial_shared else shared, la[l])
        ts.append((c, int(sa[s]), int(la[l1]), int(la[l2])))
    return Case(name, variant, shared, cands, nnratio, check_ori, cs, ts)


# ---- the suite -------------------------------------------------------------------------------------------------------------------
SERIAL_COUNTS = (300, 65, 64, 63, 1, 0)                         # the staging batch of 64 at, below and above its edge; several rounds


def specs_k(k, exact=False):
    """k candidates cycling through the staging-edge sizes, with an absent and an all-invalid one and a NULL mask among them when
    k >= 8.  exact: every feature of a candidate lies in the shared side's nodes and is usable, so that with ONE shared node the list
    a wave walks (serial side, frame variant) or holds on its lanes (key-frame variant) has exactly SERIAL_COUNTS entries"""
    out = []
    for c in range(k):
        s = {"n": SERIAL_COUNTS[c % len(SERIAL_COUNTS)]}
        if exact:
            s.update(inside=True, valid="ones")
        if c % 6 == 1:
            s["valid"] = "none"
        if c == 6:
            s.update(n=40, absent=True)
        if c == 7:
            s.update(n=50, valid="zero")
        out.append(s)
    return out


def list_in_node(side, node):
    """(entries, usable entries) of a side's list in one vocabulary node"""
    nodes, off, idx = side.fv
    k = np.nonzero(nodes == node)[0]
    if len(k) == 0:
        return 0, 0
    ids = idx[off[k[0]]:off[k[0] + 1]]
    return len(ids), int(len(ids) if side.valid is None else side.valid[ids].sum())


def shape_case(variant, sizes, k=17, seed=0):
    """the shapes test: shared side of 300 features in one node (the candidates' lists in it have exactly SERIAL_COUNTS entries, all
    usable) or in about 100, k candidates"""
    return make_case("%s-%s" % (variant, sizes), variant, 1000 + seed + (0 if variant == "frame" else 50) + (0 if sizes == "one" else 7),
                     300, sizes, specs_k(k, exact=sizes == "one"), contests=0)


def variants_case(variant):
    """candidates of different sizes, an empty one, one without a shared node, one whose `valid` is all zero, a NULL mask"""
    specs = [{"n": 220}, {"n": 0}, {"n": 90, "absent": True}, {"n": 130, "valid": "zero"}, {"n": 75, "valid": "none"}, {"n": 310}]
    return make_case("variants-" + variant, variant, 77 if variant == "frame" else 78, 260, "many", specs, contests=2, dup_pairs=4)


def contest_case(variant):
    """planted contests and ties; every candidate has enough copies for 20 matches"""
    specs = [{"n": 150}, {"n": 200, "valid": "none"}, {"n": 120}]
    return make_case("contest-" + variant, variant, 31 if variant == "frame" else 32, 240, "many", specs, contests=5, ties=True, dup_pairs=3)


def fallback_case(variant="frame"):
    """a node of 4200 lane-side features next to one of 50: candidate 0 lives in the small node only and stays in the launch,
    candidates 1 and 2 are in both and take the host selection"""
    if variant == "frame":
        small = 3 + 7
        return make_case("fallback-frame", "frame", 55, 4250, [4200, 50], [{"n": 30, "nodes": {small}, "copy": 1.0}, {"n": 60}, {"n": 45}])
    # key-frame variant: the lanes are the candidate's, so the large node is candidate 1's own
    return make_case("fallback-kf", "kf", 56, 80, "one", [{"n": 60}, {"n": 7000, "copy": 0.01}, {"n": 70}])


def suite():
    """name -> Case: what the CPU test checks the coverage of and the GPU test runs"""
    out = {}
    for variant in ("frame", "kf"):
        for case in (variants_case(variant), contest_case(variant)):
            out[case.name] = case
    return out
