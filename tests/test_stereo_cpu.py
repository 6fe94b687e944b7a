"""Frame::ComputeStereoMatches (src/Frame.cc:466-640) on the oracle (oro_stereo_matches), CPU only.  One hand-built case
per rule of the function (tests/stereo_cases.py), each checked against its own expectation and bit for bit against a
plain Python restatement; and an accuracy check on a rendered scene with a known sub-pixel disparity, which bit equality
between implementations cannot replace (a misreading shared by all of them would pass it)."""
import numpy as np
import pytest

import oracle_lib as O
import stereo_cases as S

CASES = S.hand_cases()
BY_NAME = {c.name: c for c in CASES}


oracle_run, python_run, assert_bits = S.oracle_run, S.python_run, S.assert_bits


def test_scale_tables_are_the_extractors():
    for sf, nl in [(1.2, 8), (2.0, 4), (1.5, 6)]:
        e = O.Extractor(500, sf, nl).e
        s, inv = S.scale_tables(sf, nl)
        assert_bits(s, np.array(list(e.scale)[:nl], np.float32), "scale")
        assert_bits(inv, np.array(list(e.inv_scale)[:nl], np.float32), "inv_scale")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_case(case):
    u, d = oracle_run(case)
    S.check_expectations(case, u, d)
    pu, pd = python_run(case)
    assert_bits(u, pu, "mvuRight")
    assert_bits(d, pd, "mvDepth")


def _trace(name, i=0):
    t = {}
    python_run(BY_NAME[name], t)
    return t[i]


def test_cases_reach_the_branches_they_name():
    """The constructed images produce the SAD landscapes the cases are named after (so each case tests its rule)."""
    assert len(set(_trace("sad_flat")["sads"])) == 1 and _trace("sad_flat")["bestinc"] == -5
    for t in (5, -5, 4, -4, 1):
        tr = _trace("sad_v_%+d" % t)
        assert tr["sads"] == [660 * abs(inc - t) for inc in range(-5, 6)], tr
    tr = _trace("sad_plateau_kink268")
    assert tr["sads"][8:] == [0, 0, 0] and min(tr["sads"][:8]) > 0 and tr["bestinc"] == 3
    tr = _trace("sad_plateau_kink265")
    assert tr["sads"][5:] == [0] * 6 and tr["bestinc"] == 0
    tr = _trace("sad_plateau_kink275")
    assert tr["bestinc"] == 5 and tr["sads"] == sorted(tr["sads"], reverse=True)
    for name in ("clamp_level0", "clamp_level1", "clamp_level2"):
        tr = _trace(name)
        assert tr["bestinc"] == 0 and tr["sads"][4] == tr["sads"][6] > 0, (name, tr)
    for name, k in [("hamming_tie_ab", 0), ("hamming_tie_ba", 0), ("hamming_better_later", 1), ("hamming_99_best_not_matched", 1)]:
        assert _trace(name)["bestIdxR"] == k, name
    assert _trace("hamming_99_best_not_matched")["bestDist"] == 99
    for name, sads in [("cull_odd", [3, 10, 10, 20, 21]), ("cull_even", [10, 10, 12, 21])]:
        t = {}
        python_run(BY_NAME[name], t)
        assert [min(t[i]["sads"]) for i in range(len(sads))] == sads
    for c in CASES:                             # the reference's domain: vDistIdx is never empty (:627)
        t = {}
        python_run(c, t)
        assert t["matched_before_cull"] >= 1, c.name
    # the odd case's threshold is exactly 21: 1.5f * 1.4f rounds to 2.0999999f and 2.0999999f * 10 ties to 21.0f
    assert np.float32(np.float32(np.float32(1.5) * np.float32(1.4)) * np.float32(10)) == np.float32(21.0)


def test_right_keypoint_order_decides_ties():
    """The tie rule is by index: permuting the right keypoints moves the result exactly as the restatement predicts."""
    c = BY_NAME["hamming_tie_ab"]
    perm = np.array([1, 0] + list(range(2, len(c.kr))))
    u0, _ = oracle_run(c)
    u1, d1 = oracle_run(c, kr=c.kr[perm], dr=c.dr[perm])
    ex = O.Extractor(500, c.sf, c.nl)
    pu, pd = S.stereo_reference(c.scale, c.inv_scale, c.kl, c.dl, c.kr[perm], c.dr[perm], ex.pyramid(c.left),
                                ex.pyramid(c.right), c.mb, c.mbf)
    assert_bits(u1, pu, "mvuRight")
    assert_bits(d1, pd, "mvDepth")
    assert abs(u0[0] - 240) <= 0.5 and abs(u1[0] - 275) <= 0.5


# ---------------------------------------------------------------------------------------------------------------------
# accuracy against a known disparity

@pytest.mark.parametrize("d,seed", S.ACC_CASES)
def test_accuracy_known_disparity_oracle(d, seed):
    ex, left, right, kl, dl, kr, dr = S.accuracy_scene(d, seed)
    mb, mbf = S.rig(500.0)
    u, depth = O.stereo_matches(ex, kl, dl, kr, dr, ex.pyramid(left), ex.pyramid(right), mb, mbf)
    S.check_accuracy(ex, kl, u, depth, d, mbf)
