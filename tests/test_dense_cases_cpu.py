"""The planted matcher cases of dense_cases.py hold what they promise, and on exactly these inputs the C oracle and the independent
numpy restatement (ref_best2 / ref_accept) agree.  tests/test_dense_adversarial_gpu.py compares the kernels with the restatement."""
from fractions import Fraction

import numpy as np
import pytest

import dense_cases as DC
import oracle_lib as O


def _same(a, b, what):
    for name, x, y in zip(("bi", "bd", "sd"), a, b):
        assert np.array_equal(x, y), "%s: %s differs at %s" % (what, name, np.flatnonzero(np.asarray(x) != np.asarray(y))[:8])


@pytest.mark.parametrize("name", DC.DENSE_NAMES)
def test_dense_case_facts_and_oracle(name):
    q, t, facts = DC.dense_case(name)
    ref = DC.check_facts(q, t, facts)
    _same(ref, O.best2(q, t), name)


def test_shape_cases_facts_and_oracle():
    order = DC.shape_cases()
    assert len(order) == len(DC.SHAPE_NQ) * len(DC.SHAPE_NT) == len(set(order))
    for nq, nt in order:
        q, t, facts = DC.shape_case(nq, nt)
        assert q.shape == (nq, 32) and t.shape == (nt, 32)
        _same(DC.check_facts(q, t, facts), O.best2(q, t), "nq=%d nt=%d" % (nq, nt))


def test_far_end_of_the_distance_range_is_reached():
    """254, 255 and 256 occur as best and as second-best distances, and a lone 256 leaves no best."""
    seen = set()
    for name in DC.DENSE_NAMES:
        if name.startswith("ladder"):
            q, t, facts = DC.dense_case(name)
            bi, bd, sd = DC.check_facts(q, t, facts)
            seen.update(zip(bd.tolist(), sd.tolist()))
            assert ((bd == 256) == (bi == -1)).all()
    assert {(254, 255), (255, 256), (256, 256), (0, 1), (127, 128)} <= seen


def test_planted_ties_and_order():
    q, t, facts = DC.dense_case("sweep_gap1_tie")
    bi, bd, sd = DC.check_facts(q, t, facts)
    assert len(q) == 671 and np.array_equal(bi, np.arange(671)) and (bd == 32).all() and (sd == 32).all()
    q, t, facts = DC.dense_case("sweep_gap1_unequal")
    bi, bd, sd = DC.check_facts(q, t, facts)
    assert np.array_equal(bi, np.arange(671) + 1) and (bd == 30).all() and (sd == 34).all()     # second best at the LOWER index
    for nt, gap in ((672, 1), (4200, 1), (8300, 1)):
        q, t, _ = DC.planted(nt, [nt - 2], gap, 16, 16, seed=nt)
        third = np.sort(DC.hamming(q, t)[0])[2]
        assert third >= 36


@pytest.mark.parametrize("name", ["counts", "chunk", "accept"])
def test_batch_case_padding_and_oracle(name):
    c = DC.batch_case(name)
    bi, bd, sd = DC.batch_reference(c)
    for b in range(len(c["nqs"])):
        nq, nt = int(c["nqs"][b]), int(c["nts"][b])
        ql, tl = c["q"][b, :nq], c["t"][b, :nt]
        _same((bi[b, :nq], bd[b, :nq], sd[b, :nq]), O.best2(ql, tl), "%s pair %d" % (name, b))
        assert (bi[b, nq:] == -1).all() and (bd[b, nq:] == 256).all() and (sd[b, nq:] == 256).all()
        # beyond the counts: exact copies of the other side's live rows, never zeros
        if nq and nt < c["cap"]:
            assert (DC.hamming(ql[:c["cap"] - nt], c["t"][b, nt:]).diagonal() == 0).all()
        if nt and nq < c["cap"]:
            assert (DC.hamming(c["q"][b, nq:], tl[:c["cap"] - nq]).diagonal() == 0).all()
        for nnratio in DC.NNRATIOS:
            m, n = DC.ref_accept(bi[b, :nq], bd[b, :nq], sd[b, :nq], 50, nnratio)
            on, om = O.match_dense(ql, np.zeros(nq, np.float32), tl, np.zeros(nt, np.float32), 50, nnratio, False) \
                if nq else (0, np.zeros(0, np.int32))
            assert n == on and np.array_equal(m, om), (name, b, nnratio)
    if name == "counts":
        assert set(c["nts"].tolist()) >= {0, 1, c["cap"]} and set(c["nqs"].tolist()) >= {0, c["cap"]}


@pytest.mark.parametrize("nnratio", DC.NNRATIOS)
@pytest.mark.parametrize("th", [50, 45, 27])
def test_acceptance_boundaries_and_oracle(nnratio, th):
    q, t, facts = DC.accept_case()
    bi, bd, sd = DC.check_facts(q, t, facts)
    m, n = DC.ref_accept(bi, bd, sd, th, nnratio)
    zq, zt = np.zeros(len(q), np.float32), np.zeros(len(t), np.float32)
    on, om = O.match_dense(q, zq, t, zt, th, nnratio, False)
    assert n == on and np.array_equal(m, om)
    on, om = O.match_dense(q, zq, t, zt, th, nnratio, True)      # all angles equal: one histogram bin, nothing is culled
    assert n == on and np.array_equal(m, om)
    # bd == th is accepted wherever the ratio passes by a margin no rounding reaches (bd / sd < nnratio - 0.01, in integers) ...
    clear = (bd == th) & (100 * bd < (round(100 * nnratio) - 1) * sd)
    assert (m[clear] >= 0).all()
    assert clear.any() or th != 50       # 50/100 passes every ratio; at 45 and 27 a small ratio leaves only equalities (45/75, 27/45) or less
    assert (m[bd == th + 1] == -1).all() and (bd == th + 1).any()      # ... th + 1 never


def test_float32_ratio_test_differs_from_the_rational_where_expected():
    """The reference multiplies in float: (float)bd < nnratio * (float)sd.  Where that differs from the exact bd / sd < nnratio is
    part of what is pinned."""
    pairs = DC.accept_pairs()
    assert {(15, 25), (27, 45), (30, 50), (9, 10), (45, 50), (50, 100), (51, 100), (14, 25), (16, 25)} <= set(pairs)
    bd, sd = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    differs = {}
    for nnratio, frac in zip(DC.NNRATIOS, (Fraction(3, 5), Fraction(7, 10), Fraction(3, 4), Fraction(4, 5), Fraction(9, 10))):
        m, _ = DC.ref_accept(np.zeros(len(pairs), np.int32), bd, sd, 256, nnratio)
        exact = np.array([Fraction(int(a)) < frac * int(b) for a, b in pairs])
        differs[nnratio] = sorted(p for p, x, y in zip(pairs, m >= 0, exact) if x != y)
    assert differs[0.6] == [(15, 25), (27, 45), (30, 50)]        # accepted in float32, equal in the rationals
    assert differs[0.9] == []                                    # 9/10 ... 45/50: rejected either way
    m, _ = DC.ref_accept(np.zeros(5, np.int32), 9 * np.arange(1, 6), 10 * np.arange(1, 6), 256, 0.9)
    assert (m == -1).all()
    assert differs[0.75] == []                                   # 0.75 is exact in binary


def test_csr_case_lists_and_oracle():
    c = DC.csr_case()
    lens = np.diff(c["off"])
    assert set(lens.tolist()) == set(DC.CSR_LENGTHS)
    spots = {(L, s) for L, s, _ in c["plan"] if s}
    assert {(65, (0, 64)), (65, (63, 64)), (65, (0, 1)), (200, (1, 65)), (200, (198, 199)), (2, (0, 1)), (64, (62, 63))} <= spots
    assert {k for _, s, k in c["plan"] if s} == set(DC.CSR_KINDS)
    _same(DC.ref_best2(c["q"], c["t"], c["off"], c["idx"]), O.best2(c["q"], c["t"], c["off"], c["idx"]), "csr")
