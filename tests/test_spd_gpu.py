"""orbm_spd_solve_f64 (include/orbm.h, csrc/orbm_spd.hip): the blocked Cholesky solve over many workgroups that
orbm_bundle_adjustment runs on its reduced system.  Sizes around the panel width NB = 48: 6 (one key frame), NB - 6, NB, NB + 6 and
3 NB + 6 (four panels, a ragged last one, off-diagonal tiles in the trailing update).

The bar is Higham's normwise backward error bound for a Cholesky solve (Accuracy and Stability of Numerical Algorithms, theorem
10.4 with gamma_{3n+1}): |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf) <= (3 n + 1) 2^-53.  numpy's LAPACK solution of the same
system is held to the same cap first and printed beside the kernel's figure."""
import numpy as np
import pytest

import ba_cases as bc

pytestmark = pytest.mark.gpu

NB = bc.NB
SIZES = (6, NB - 6, NB, NB + 6, 3 * NB + 6)


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


@pytest.mark.parametrize("n", SIZES)
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


def test_only_the_lower_triangle_is_read(m):
    A, b = system(NB + 6)
    x, ok = m.spd_solve(A, b)
    x2, ok2 = m.spd_solve(np.tril(A) + np.triu(np.full_like(A, np.nan), 1), b)
    assert ok and ok2 and x.tobytes() == x2.tobytes()


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


@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_a_pivot_that_is_not_positive_is_reported_not_trapped(m, where):
    n = 3 * NB + 6
    A, b = system(n)
    j = {"first": 5, "middle": NB + NB // 2, "last": n - 1}[where]
    B = A.copy()
    B[j, j] = -1.0
    x, ok = m.spd_solve(B, b)                                               # returns ORBX_OK: spd_solve raises on any error code
    assert not ok and x.tobytes() == np.zeros(n).tobytes()
    B[j, j] = np.nan
    x, ok = m.spd_solve(B, b)
    assert not ok and x.tobytes() == np.zeros(n).tobytes()
    x, ok = m.spd_solve(A, b)                                               # the next solve on the handle is right
    assert ok and backward_error(A, x, b) <= (3 * n + 1) * 2.0 ** -53


def test_the_result_does_not_depend_on_the_handles_history(m, orbx):
    A, b = system(NB + 6, seed=1)
    first = m.spd_solve(A, b)[0]
    m.spd_solve(*system(3 * NB + 6, seed=2))
    m.spd_solve(*system(6, seed=3))
    assert m.spd_solve(A, b)[0].tobytes() == first.tobytes()
    h = orbx.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        assert h.spd_solve(A, b)[0].tobytes() == first.tobytes()
    finally:
        h.close()
