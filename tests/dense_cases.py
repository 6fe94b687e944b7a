"""Planted cases and a plain numpy reference for the best / second-best Hamming matcher (dense, batched and CSR) and its
acceptance.  Pure numpy: neither the library nor the C oracle is imported here, so that tests/test_dense_cases_cpu.py can hold the
oracle and this restatement against each other on exactly the inputs the GPU tests use.

Every builder returns (q, t, facts) -- or a dict for the batched / CSR forms -- where `facts` holds what the planting promises
(best index, best and second-best distance per query).  check_facts() asserts them with ref_best2 before anything is compared with
a kernel: a case whose planting failed is an error, never a skip.  All seeds are fixed; the asserts guard them.

The rule (src/ORBmatcher.cc:214-223): strictly smaller wins, so the lowest list position wins a tie, a tie with the best becomes the
second best, and the second best may sit ahead of the best in the list.  A distance of 256 is never a best."""
import functools

import numpy as np

NONE_D = 256


# ---------------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(d):
    return np.unpackbits(np.ascontiguousarray(d, np.uint8).reshape(-1, 32), axis=1)


def _pack(bits):
    return np.packbits(np.asarray(bits, np.uint8).reshape(-1, 256), axis=1)


def hamming(q, t):
    """All nq x nt distances from the unpacked bits: |a ^ b| = |a| + |b| - 2 a.b (sums of at most 256 ones: exact in float32)."""
    qb, tb = _bits(q).astype(np.float32), _bits(t).astype(np.float32)
    return (qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2.0 * (qb @ tb.T)).astype(np.int32)


def _select(D):
    """(list position of the best or -1, best distance, second-best distance) per row of D: the sort of (distance, position)."""
    n, L = D.shape
    pos, bd, sd = np.full(n, -1, np.int32), np.full(n, NONE_D, np.int32), np.full(n, NONE_D, np.int32)
    if n == 0 or L == 0:
        return pos, bd, sd
    order = np.argsort(D, axis=1, kind="stable")[:, :2]          # stable: equal distances stay in list order
    rows = np.arange(n)
    bd = np.minimum(D[rows, order[:, 0]], NONE_D).astype(np.int32)
    pos = np.where(bd < NONE_D, order[:, 0], -1).astype(np.int32)
    if L > 1:
        sd = np.minimum(D[rows, order[:, 1]], NONE_D).astype(np.int32)
    return pos, bd, sd


def ref_best2(q, t, off=None, idx=None):
    """(best_idx, best_d, second_d), int32 per query; dense over all of t, or over the candidate lists idx[off[i]:off[i+1]]."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    if off is None:
        return _select(hamming(q, t))
    nq = len(q)
    bi, bd, sd = np.full(nq, -1, np.int32), np.full(nq, NONE_D, np.int32), np.full(nq, NONE_D, np.int32)
    for i in range(nq):
        lst = np.asarray(idx[off[i]:off[i + 1]], np.int64)
        p, d1, d2 = _select(hamming(q[i:i + 1], t[lst]))
        bd[i], sd[i] = d1[0], d2[0]
        bi[i] = lst[p[0]] if p[0] >= 0 else -1
    return bi, bd, sd


def ref_accept(bi, bd, sd, th, nnratio):
    """(match12, nmatches) of src/ORBmatcher.cc:228-232, the ratio test computed in float32 as the reference does."""
    bd, sd = np.asarray(bd, np.int32), np.asarray(sd, np.int32)
    ok = (bd <= th) & (bd.astype(np.float32) < np.float32(nnratio) * sd.astype(np.float32))
    m = np.where(ok, np.asarray(bi, np.int32), -1).astype(np.int32)
    return m, int(ok.sum())


def check_facts(q, t, facts, off=None, idx=None):
    """The planting holds (by ref_best2); returns the reference triple.  facts: any of bi / bd / sd (arrays or scalars), and
    `alone`: no third row lies at or below the second-best distance."""
    bi, bd, sd = ref_best2(q, t, off, idx)
    for name, got in (("bi", bi), ("bd", bd), ("sd", sd)):
        if name in facts:
            want = np.broadcast_to(np.asarray(facts[name], np.int32), got.shape)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "planting failed: %s of query %d is %d, planted %d" % (name, bad[0], got[bad[0]], want[bad[0]])
    if facts.get("alone"):
        n_within = (hamming(q, t) <= sd[:, None]).sum(1)
        assert (n_within == 2).all(), "planting failed: query %d has %d rows within its second-best distance" % (
            int(np.argmax(n_within != 2)), int(n_within[np.argmax(n_within != 2)]))
    return bi, bd, sd


# ---------------------------------------------------------------------------------------------------------------------------------
# marker construction: train row j = base ^ m_j with a random weight-32 marker m_j; a query aimed at rows p and p2 is base ^ x with
# a bits that only m_p has and b bits that only m_p2 has: its distances to the two rows are exactly 32 - a + b and 32 - b + a, every
# other row lies at 64 - 2 * overlap.
# ---------------------------------------------------------------------------------------------------------------------------------
def _marker_train(rng, nt):
    base = rng.integers(0, 2, 256, dtype=np.uint8)
    m = np.zeros((nt, 256), np.uint8)
    np.put_along_axis(m, np.argsort(rng.random((nt, 256)), axis=1)[:, :32], 1, axis=1)
    return base, m


def _aim(base, m, p, p2, a, b):
    only_p, only_p2 = np.flatnonzero((m[p] == 1) & (m[p2] == 0)), np.flatnonzero((m[p2] == 1) & (m[p] == 0))
    assert len(only_p) >= a and len(only_p2) >= b, "markers %d and %d overlap too much" % (p, p2)
    x = np.zeros(256, np.uint8)
    x[only_p[:a]] = 1
    x[only_p2[:b]] = 1
    return base ^ x


def planted(nt, ps, gap, a, b, seed):
    """Query k is aimed at train rows ps[k] and ps[k] + gap with (a, b) bits (scalars or one per query)."""
    rng = np.random.default_rng(seed)
    base, m = _marker_train(rng, nt)
    ps = np.asarray(ps, np.int64)
    a, b = np.broadcast_to(np.asarray(a), ps.shape), np.broadcast_to(np.asarray(b), ps.shape)
    q = _pack(np.stack([_aim(base, m, int(p), int(p) + gap, int(x), int(y)) for p, x, y in zip(ps, a, b)]))
    t = _pack(base[None, :] ^ m)
    d1, d2 = 32 - a + b, 32 - b + a                      # distance to row p, to row p + gap
    facts = {"bi": np.where(d1 <= d2, ps, ps + gap), "bd": np.minimum(d1, d2), "sd": np.maximum(d1, d2), "alone": True}
    return q, t, facts


TIE, UNEQUAL = (16, 16), (15, 17)       # a tie at 32 | best 30 at the HIGHER index, second best 34 at the lower one


def tie_sweep(gap, ab):
    """nt = 672: query i is aimed at rows i and i + gap, for every i: every adjacent-row boundary of whatever tile, stage, split
    or lane layout is hit (gap 1), or every row against the one a part (224) / more than a part (352) further on."""
    return planted(672, np.arange(672 - gap), gap, ab[0], ab[1], seed=6720 + gap)


def chunk_sweep(nt, gap, ab):
    """Pairs around the 4096-row index chunk boundaries."""
    assert (nt, gap) in ((4200, 1), (8300, 1), (8300, 4096))
    if nt == 4200:
        ps = np.arange(3990, 4199)
    elif gap == 1:
        ps = np.concatenate([np.arange(4090, 4100), np.arange(8186, 8196)])
    else:
        ps = np.concatenate([np.arange(0, 10), np.arange(4090, 4100), np.arange(4194, 4204)])
    return planted(nt, ps, gap, ab[0], ab[1], seed=nt + gap)


def identical_rows(nt, d):
    """All train rows are one descriptor; 33 queries at distance d from it: the first row is the best, the second ties with it."""
    rng = np.random.default_rng(1000 * d + nt)
    row = rng.integers(0, 2, 256, dtype=np.uint8)
    qb = np.tile(row, (33, 1))
    for i in range(33):
        qb[i, rng.permutation(256)[:d]] ^= 1
    return _pack(qb), np.tile(_pack(row), (nt, 1)), {"bi": 0, "bd": d, "sd": d}


LADDER = (0, 1, 2, 63, 64, 127, 128, 129, 254, 255, 256)
LADDER_QUERIES = (0, 1, 2, 128, 255, 256)


def _scan(D):
    """The reference's loop, literally (for the facts of the small planted tables)."""
    n, L = D.shape
    bi, bd, sd = np.full(n, -1, np.int32), np.full(n, NONE_D, np.int32), np.full(n, NONE_D, np.int32)
    for i in range(n):
        for j in range(L):
            d = D[i, j]
            if d < bd[i]:
                sd[i], bd[i], bi[i] = bd[i], d, j
            elif d < sd[i]:
                sd[i] = d
    return bi, bd, sd


def ladder(nt, ds, rows, seed):
    """Train row rows[k] is the query with exactly ds[k] bits flipped; every other row is its complement (distance 256).  The flipped
    bits are nested, and query c is itself the first query with c bits flipped, so its distance to a row of d flips is |c - d|: the
    first query sees the ladder as it stands, the others see its far end from nearby."""
    rng = np.random.default_rng(seed)
    q0, perm = rng.integers(0, 2, 256, dtype=np.uint8), rng.permutation(256)

    def flipped(d):
        x = q0.copy()
        x[perm[:d]] ^= 1
        return x
    dvec = np.full(nt, 256, np.int32)
    dvec[np.asarray(rows)] = np.asarray(ds)
    lut = np.stack([flipped(d) for d in range(257)])
    t = _pack(lut[dvec])
    q = _pack(lut[np.asarray(LADDER_QUERIES)])
    bi, bd, sd = _scan(np.abs(np.asarray(LADDER_QUERIES, np.int32)[:, None] - dvec[None, :]))
    return q, t, {"bi": bi, "bd": bd, "sd": sd}


SHAPE_NQ = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
SHAPE_NT = (0, 1, 2, 31, 32, 33, 95, 96, 97, 127, 128, 129)


def shape_case(nq, nt):
    """Random train rows; query i is the LAST train row with i % 5 bits flipped, so the winner sits at nt - 1."""
    rng = np.random.default_rng(1000 * nq + nt)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    if nt == 0:
        return rng.integers(0, 256, (nq, 32), dtype=np.uint8), t, {"bi": -1, "bd": 256, "sd": 256}
    qb = np.tile(_bits(t[nt - 1]), (nq, 1))
    for i in range(nq):
        qb[i, rng.permutation(256)[:i % 5]] ^= 1
    facts = {"bi": nt - 1, "bd": np.arange(nq) % 5}
    if nt == 1:
        facts["sd"] = 256
    return _pack(qb), t, facts


def shape_cases():
    """Every (nq, nt) of SHAPE_NQ x SHAPE_NT, large and small shapes in turn."""
    combos = sorted(((nq, nt) for nq in SHAPE_NQ for nt in SHAPE_NT), key=lambda s: (s[0] * s[1], s))
    order = []
    while combos:
        order.append(combos.pop())
        if combos:
            order.append(combos.pop(0))
    return order


# ---------------------------------------------------------------------------------------------------------------------------------
# acceptance: query i owns train rows 2i and 2i + 1, the query with bd_i and with sd_i bits flipped (in that order for even i, the
# second best first for odd i).  The queries are rows of the 256 x 256 Sylvester-Hadamard matrix (any two exactly 128 bits apart)
# under one random mask, so foreign rows stay far away.
# ---------------------------------------------------------------------------------------------------------------------------------
NNRATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)


def accept_pairs():
    pairs = set()
    for u, v in ((3, 5), (9, 10), (3, 4), (7, 10), (4, 5)):
        k = 1
        while k * u <= 50:
            for e in (-1, 0, 1):
                pairs.add((k * u + e, k * v))
            k += 1
    pairs.update([(50, 100), (51, 100)])
    return sorted(pairs)


@functools.lru_cache(maxsize=None)
def accept_case():
    rng = np.random.default_rng(2850)
    pairs = accept_pairs()
    nq = len(pairs)
    assert nq <= 255
    H = np.array([[bin(i & j).count("1") & 1 for j in range(256)] for i in range(1, nq + 1)], np.uint8)
    qb = H ^ rng.integers(0, 2, 256, dtype=np.uint8)[None, :]
    tb = np.repeat(qb, 2, axis=0)
    bi, bd, sd = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    for i, (d1, d2) in enumerate(pairs):
        perm = rng.permutation(256)
        first, second = (2 * i, 2 * i + 1) if i % 2 == 0 else (2 * i + 1, 2 * i)
        tb[first, perm[:d1]] ^= 1                      # disjoint bit sets for the two rows
        tb[second, perm[d1:d1 + d2]] ^= 1
        bd[i], sd[i] = min(d1, d2), max(d1, d2)
        bi[i] = first if d1 < d2 else min(first, second) if d1 == d2 else second
    return _pack(qb), _pack(tb), {"bi": bi, "bd": bd, "sd": sd, "alone": True}


# ---------------------------------------------------------------------------------------------------------------------------------
# batched (device-resident) form: [nb, cap, 32] arrays with per-pair counts.  What lies beyond the counts is NOT zero: the rows
# nts[b]..cap of t are copies of the pair's queries and the rows nqs[b]..cap of q copies of its train rows, so a row that slips past
# its mask is an exact match at once.
# ---------------------------------------------------------------------------------------------------------------------------------
def pad_batch(pairs, cap):
    nb = len(pairs)
    q, t = np.zeros((nb, cap, 32), np.uint8), np.zeros((nb, cap, 32), np.uint8)
    nqs, nts = np.array([len(p[0]) for p in pairs], np.int32), np.array([len(p[1]) for p in pairs], np.int32)
    for b, (ql, tl) in enumerate(pairs):
        nq, nt = len(ql), len(tl)
        assert nq <= cap and nt <= cap and nq + nt > 0
        q[b, :nq], t[b, :nt] = ql, tl
        src = tl if nt else ql
        q[b, nq:] = src[np.arange(cap - nq) % len(src)]
        src = ql if nq else tl
        t[b, nt:] = src[np.arange(cap - nt) % len(src)]
    return q, t, nqs, nts


def _batch(pairs_facts, cap):
    q, t, nqs, nts = pad_batch([(p[0], p[1]) for p in pairs_facts], cap)
    return {"q": q, "t": t, "nqs": nqs, "nts": nts, "cap": cap, "facts": [p[2] for p in pairs_facts]}


@functools.lru_cache(maxsize=None)
def batch_case(name):
    rng = np.random.default_rng(77)
    if name == "counts":         # cap = 672, six pairs: nt in {0, 1}, nq = 0, nq = cap, nt = cap
        k = np.arange(672)
        ab = np.where(k % 2 == 0, 16, 15), np.where(k % 2 == 0, 16, 17)
        p0 = planted(671, k % 670, 1, ab[0], ab[1], seed=1)
        p1 = (np.zeros((0, 32), np.uint8), rng.integers(0, 256, (672, 32), dtype=np.uint8), {})
        p2 = (rng.integers(0, 256, (100, 32), dtype=np.uint8), np.zeros((0, 32), np.uint8), {"bi": -1, "bd": 256, "sd": 256})
        row = rng.integers(0, 2, 256, dtype=np.uint8)
        qb = np.tile(row, (671, 1))
        for i in range(671):
            qb[i, :i % 40] ^= 1
        p3 = (_pack(qb), _pack(row), {"bi": 0, "bd": np.arange(671) % 40, "sd": 256})
        p4 = planted(672, np.arange(33) * 13, 224, 16, 16, seed=4)
        p5 = planted(225, [223], 1, 15, 17, seed=5)
        return _batch([p0, p1, p2, p3, p4, p5], 672)
    if name == "chunk":          # cap = 4200: many splits (the grid-wide pre-merge of the partials) and the 4096-row chunk boundary
        return _batch([chunk_sweep(4200, 1, TIE), planted(4199, np.arange(4000, 4198), 1, 15, 17, seed=10)], 4200)
    if name == "accept":         # the acceptance table as one pair
        q, t, facts = accept_case()
        return _batch([(q, t, facts)], len(t))
    raise KeyError(name)


def batch_reference(c):
    """(bi, bd, sd) as [nb, cap] arrays: ref_best2 on the live part of every pair (its facts asserted), -1 / 256 / 256 beyond the count."""
    nb, cap = len(c["nqs"]), c["cap"]
    bi, bd, sd = np.full((nb, cap), -1, np.int32), np.full((nb, cap), NONE_D, np.int32), np.full((nb, cap), NONE_D, np.int32)
    for b in range(nb):
        nq, nt = int(c["nqs"][b]), int(c["nts"][b])
        bi[b, :nq], bd[b, :nq], sd[b, :nq] = check_facts(c["q"][b, :nq], c["t"][b, :nt], c["facts"][b])
    return bi, bd, sd


# ---------------------------------------------------------------------------------------------------------------------------------
# CSR: one candidate list per query.  Train rows 2i and 2i + 1 are near query i (A, B), the rest of the pool is far from everything.
# ---------------------------------------------------------------------------------------------------------------------------------
CSR_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
CSR_KINDS = ("tie", "second_first", "best_first", "twice")


@functools.lru_cache(maxsize=None)
def csr_case():
    """Lists of every length in CSR_LENGTHS with A and B at positions (0,1), (0,64), (63,64), (1,65) and the last two (across lanes,
    across the iterations of one lane, both), as a tie, with the second best ahead of the best, the other way round, and with the
    same train index listed twice."""
    rng = np.random.default_rng(640)
    plan = []
    for L in CSR_LENGTHS:
        spots = sorted({s for s in ((0, 1), (0, 64), (63, 64), (1, 65), (L - 2, L - 1)) if 0 <= s[0] < s[1] < L})
        if not spots:
            plan.append((L, None, None))
        for s in spots:
            for kind in CSR_KINDS:
                plan.append((L, s, kind))
    nq, nfar = len(plan), 300
    qb = rng.integers(0, 2, (nq, 256), dtype=np.uint8)
    tb = np.concatenate([np.repeat(qb, 2, axis=0), rng.integers(0, 2, (nfar, 256), dtype=np.uint8)])
    off, idx = np.zeros(nq + 1, np.int32), []
    bi, bd, sd = np.full(nq, -1, np.int32), np.full(nq, NONE_D, np.int32), np.full(nq, NONE_D, np.int32)
    far = np.zeros(nq, bool)
    for i, (L, s, kind) in enumerate(plan):
        lst = (2 * nq + rng.integers(0, nfar, L)).astype(np.int32)
        if s is None:
            far[i] = True
        else:
            dA, dB = {"tie": (20, 20), "second_first": (25, 20), "best_first": (20, 25), "twice": (20, 20)}[kind]
            perm = rng.permutation(256)
            tb[2 * i, perm[:dA]] ^= 1
            tb[2 * i + 1, perm[100:100 + dB]] ^= 1
            lst[s[0]], lst[s[1]] = 2 * i, (2 * i if kind == "twice" else 2 * i + 1)
            bi[i], bd[i], sd[i] = (2 * i + 1 if kind == "second_first" else 2 * i), min(dA, dB), max(dA, dB)
        idx.append(lst)
        off[i + 1] = off[i] + L
    q, t, idx = _pack(qb), _pack(tb), np.concatenate(idx).astype(np.int32)
    r = ref_best2(q, t, off, idx)
    keep = ~far
    for name, want, got in (("bi", bi, r[0]), ("bd", bd, r[1]), ("sd", sd, r[2])):
        assert np.array_equal(want[keep], got[keep]), "planting failed: %s of the CSR lists" % name
    return {"q": q, "t": t, "off": off, "idx": idx, "plan": plan}


# ---------------------------------------------------------------------------------------------------------------------------------
# the dense host-API cases, by name, large and small shapes in turn
# ---------------------------------------------------------------------------------------------------------------------------------
_L11 = (0, 3, 4, 31, 32, 95, 96, 4094, 4095, 4096, 4199)
_DENSE = {
    "chunk8300_gap1_tie": lambda: chunk_sweep(8300, 1, TIE),
    "identical2_d0": lambda: identical_rows(2, 0),
    "chunk8300_gap4096_unequal": lambda: chunk_sweep(8300, 4096, UNEQUAL),
    "ladder_top3_up_nt97": lambda: ladder(97, (254, 255, 256), (31, 32, 96), 11),
    "chunk4200_tie": lambda: chunk_sweep(4200, 1, TIE),
    "identical33_d37": lambda: identical_rows(33, 37),
    "ladder_up": lambda: ladder(4200, LADDER, _L11, 12),
    "ladder_256_alone_nt1": lambda: ladder(1, (256,), (0,), 13),
    "sweep_gap1_tie": lambda: tie_sweep(1, TIE),
    "identical2_d37": lambda: identical_rows(2, 37),
    "chunk8300_gap4096_tie": lambda: chunk_sweep(8300, 4096, TIE),
    "ladder_top3_down_nt97": lambda: ladder(97, (256, 255, 254), (31, 32, 96), 14),
    "sweep_gap224_unequal": lambda: tie_sweep(224, UNEQUAL),
    "ladder_255_256_nt33": lambda: ladder(33, (255, 256), (0, 32), 15),
    "ladder_down": lambda: ladder(4200, LADDER[::-1], _L11, 16),
    "identical33_d0": lambda: identical_rows(33, 0),
    "sweep_gap352_tie": lambda: tie_sweep(352, TIE),
    "ladder_256_alone_nt33": lambda: ladder(33, (256,), (32,), 17),
    "chunk4200_unequal": lambda: chunk_sweep(4200, 1, UNEQUAL),
    "identical672_d37": lambda: identical_rows(672, 37),
    "ladder_top3_up_chunk": lambda: ladder(4200, (254, 255, 256), (4095, 4096, 4199), 18),
    "sweep_gap1_unequal": lambda: tie_sweep(1, UNEQUAL),
    "ladder_top3_down_chunk": lambda: ladder(4200, (256, 255, 254), (4095, 4096, 4199), 19),
    "identical672_d0": lambda: identical_rows(672, 0),
    "chunk8300_gap1_unequal": lambda: chunk_sweep(8300, 1, UNEQUAL),
    "sweep_gap224_tie": lambda: tie_sweep(224, TIE),
    "ladder_256_alone_nt4200": lambda: ladder(4200, (256,), (4096,), 20),
    "sweep_gap352_unequal": lambda: tie_sweep(352, UNEQUAL),
    "accept_table": accept_case,
}
DENSE_NAMES = tuple(_DENSE)


@functools.lru_cache(maxsize=None)
def dense_case(name):
    return _DENSE[name]()
