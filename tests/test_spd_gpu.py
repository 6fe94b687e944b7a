"""orbm_spd_solve_f64 (include/orbm.h, csrc/orbm_spd.hip): the blocked Cholesky solve over many workgroups that
orbm_bundle_adjustment runs on its reduced system.  Sizes around the panel width NB = 48: 6 (one key frame), NB - 6, NB, NB + 6 and
3 NB + 6 (four panels, a ragged last one, off-diagonal tiles in the trailing update).  SCALE_SIZES reach what only a larger n runs:
k_spd_panel and k_spd_forward take 64 rows a workgroup, so n = NB + 64 and NB + 65 put exactly 64 and then 65 rows below the first
panel (one workgroup, two); k_spd_backward takes 256 entries a workgroup, so the last panel of n = 6 NB + 6 (j0 = 288) is the first
with a second workgroup and that of 11 NB + 6 (j0 = 528) has a third; 3066 is the essential graph's cap (the last panel 42 wide)
and 3072 ORBM_SPD_MAX_N (64 full panels, 2016 tiles in the first update).

The bar is Higham's normwise backward error bound for a Cholesky solve (Accuracy and Stability of Numerical Algorithms, theorem
10.4 with gamma_{3n+1}): |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf) <= (3 n + 1) 2^-53.  numpy's LAPACK solution of the same
system is held to the same cap first and printed beside the kernel's figure."""
import numpy as np
import pytest

import ba_cases as bc

pytestmark = pytest.mark.gpu

NB = bc.NB
SIZES = (6, NB - 6, NB, NB + 6, 3 * NB + 6)
SCALE_SIZES = (NB + 64, NB + 65, 6 * NB + 6, 11 * NB + 6, 3066, 3072)
MID = 11 * NB + 6                                                           # 534: three workgroups of k_spd_backward


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    yield h
    h.close()


def system(n, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    G = rng.normal(size=(n, n))
    return G @ G.T + n * np.eye(n), rng.normal(size=n)


def backward_error(A, x, b):
    return np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())


@pytest.mark.parametrize("n", SIZES + SCALE_SIZES)
def test_backward_error_within_highams_bound(m, n):
    A, b = system(n)
    cap = (3 * n + 1) * 2.0 ** -53
    ref = backward_error(A, np.linalg.solve(A, b), b)
    assert ref <= cap, "LAPACK itself misses the cap: %.3g > %.3g" % (ref, cap)
    x, ok = m.spd_solve(A, b)
    err = backward_error(A, x, b)
    print("n = %d: backward error %.3g, LAPACK %.3g, cap %.3g" % (n, err, ref, cap))
    assert ok and np.isfinite(x).all()
    assert err <= cap, "n = %d: backward error %.3g > %.3g (LAPACK: %.3g)" % (n, err, cap, ref)
    x2, ok2 = m.spd_solve(A, b)                                             # a second run gives the same bytes
    assert ok2 and x2.tobytes() == x.tobytes()


def exact_system(n):
    """(A, b, x0, L0) with A = L0 L0^T and b = A x0, in which every operation of a correct Cholesky solve is exact: L0's strictly
    lower entries are -1, 0 or 1 and its diagonal cycles through 1, 2, 4, 0.5, x0 holds integers in [-3, 3].  4 L0 is a matrix of
    integers of magnitude at most 16, so 16 A, 16 b and every partial sum that leads to them, in any order, are integers below
    n 256 (and 3 n^2 256 for b), far below 2^53: sums, products and fmas are exact.  The factorisation retraces L0: each entry of L
    is a partial sum of such products divided by a power of two, each pivot's root is of 1, 4, 16 or 0.25; the substitutions
    retrace L0^T x0 and x0.  So x must be x0 byte for byte, and only a dropped, repeated or misplaced term can prevent it."""
    rng = np.random.default_rng(7000 + n)
    L0 = np.tril(rng.integers(-1, 2, (n, n)).astype(np.float64), -1)
    L0[np.arange(n), np.arange(n)] = np.array([1.0, 2.0, 4.0, 0.5])[np.arange(n) % 4]
    x0 = rng.integers(-3, 4, n).astype(np.float64)
    A = L0 @ L0.T
    return A, A @ x0, x0, L0


@pytest.mark.parametrize("n", (NB + 65, 6 * NB + 6, MID, 3072))
def test_an_exactly_solvable_dense_system_gives_the_exact_bytes(m, n):
    """The construction is checked first: b recomputed in np.longdouble rounds to the same doubles, and so does A: all of it up to
    n = 534, and at 3072 the first and last rows, the rows either side of every eighth panel boundary and of the backward kernel's
    workgroup boundaries (np.longdouble has no BLAS: the whole product is 10^10 operations there), together with the bound
    exact_system() gives, which makes every double sum of these terms exact whatever its order."""
    A, b, x0, L0 = exact_system(n)
    Ll, xl = L0.astype(np.longdouble), x0.astype(np.longdouble)
    if n <= MID:
        rows = np.arange(n)
    else:
        rows = np.unique(np.concatenate([[0, 1, n - 2, n - 1], np.arange(8 * NB, n, 8 * NB) - 1, np.arange(8 * NB, n, 8 * NB),
                                         [255, 256, 511, 512]]))
    Al = Ll[rows] @ Ll.T
    assert np.array_equal(Al.astype(np.float64), A[rows]) and np.array_equal(Al, A[rows].astype(np.longdouble))
    bl = A.astype(np.longdouble) @ xl
    assert np.array_equal(bl.astype(np.float64), b) and np.array_equal(bl, b.astype(np.longdouble))
    assert np.array_equal(16 * A, np.rint(16 * A)) and n * 16.0 ** 2 < 2.0 ** 53 and np.array_equal(A, A.T)
    if n <= MID:
        assert np.array_equal(np.linalg.cholesky(A), L0)
    x, ok = m.spd_solve(A, b)
    wrong = np.flatnonzero(x != x0)
    assert ok and x.tobytes() == x0.tobytes(), "n = %d: %d entries differ, the first at %s" % (n, len(wrong), wrong[:8])


def only_the_lower_triangle_is_read(m, n):
    A, b = system(n)
    x, ok = m.spd_solve(A, b)
    x2, ok2 = m.spd_solve(np.tril(A) + np.triu(np.full_like(A, np.nan), 1), b)
    assert ok and ok2 and x.tobytes() == x2.tobytes()


def test_only_the_lower_triangle_is_read(m):
    only_the_lower_triangle_is_read(m, NB + 6)


def test_only_the_lower_triangle_is_read_over_three_backward_workgroups(m):
    only_the_lower_triangle_is_read(m, MID)


@pytest.mark.parametrize("n", (6, NB, 3 * NB + 6))
def test_identity_and_diagonal_are_exact(m, n):
    b = np.arange(1, n + 1, dtype=np.float64) * np.where(np.arange(n) % 2, -1.0, 1.0)
    x, ok = m.spd_solve(np.eye(n), b)
    assert ok and x.tobytes() == b.tobytes()
    # pivots whose square roots are exact and a right-hand side that divides exactly: every operation of the solve is exact
    d = np.array([1.0, 4.0, 9.0, 16.0, 0.25, 64.0])[np.arange(n) % 6]
    want = np.arange(1, n + 1, dtype=np.float64) - n // 2
    x, ok = m.spd_solve(np.diag(d), d * want)
    assert ok and x.tobytes() == want.tobytes()


def a_pivot_that_is_not_positive_is_reported_not_trapped(m, n, j):
    A, b = system(n)
    B = A.copy()
    B[j, j] = -1.0
    x, ok = m.spd_solve(B, b)                                               # returns ORBX_OK: spd_solve raises on any error code
    assert not ok and x.tobytes() == np.zeros(n).tobytes()
    B[j, j] = np.nan
    x, ok = m.spd_solve(B, b)
    assert not ok and x.tobytes() == np.zeros(n).tobytes()
    x, ok = m.spd_solve(A, b)                                               # the next solve on the handle is right
    assert ok and backward_error(A, x, b) <= (3 * n + 1) * 2.0 ** -53


@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_a_pivot_that_is_not_positive_is_reported_not_trapped(m, where):
    n = 3 * NB + 6
    a_pivot_that_is_not_positive_is_reported_not_trapped(m, n, {"first": 5, "middle": NB + NB // 2, "last": n - 1}[where])


@pytest.mark.parametrize("j", (5, 300, MID - 1))
def test_a_pivot_that_is_not_positive_over_three_backward_workgroups(m, j):
    """n = 534.  Column 300 lies in the panel at j0 = 288 > 256: that panel's k_spd_backward and the last one's run two and three
    workgroups, and every one of them takes the `failed` return"""
    a_pivot_that_is_not_positive_is_reported_not_trapped(m, MID, j)


def test_the_result_does_not_depend_on_the_handles_history(m, orbx):
    A, b = system(NB + 6, seed=1)
    first = m.spd_solve(A, b)[0]
    m.spd_solve(*system(3 * NB + 6, seed=2))
    m.spd_solve(*system(6, seed=3))
    assert m.spd_solve(A, b)[0].tobytes() == first.tobytes()
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        assert h.spd_solve(A, b)[0].tobytes() == first.tobytes()
        # the workspace grows under the live handle: 75 MB at ORBM_SPD_MAX_N between two runs of the small system
        big = system(orbx.ORBM_SPD_MAX_N, seed=4)
        xb, ok = h.spd_solve(*big)
        assert ok and backward_error(big[0], xb, big[1]) <= (3 * orbx.ORBM_SPD_MAX_N + 1) * 2.0 ** -53
        assert h.spd_solve(A, b)[0].tobytes() == first.tobytes()
    finally:
        h.close()
