"""`stop` of Optimizer::LocalBundleAdjustment at every place where it is read (include/orbp.h): at entry (src/Optimizer.cc:655-657),
at the top of every iteration (g2o sparse_optimizer.cpp:376), in the trial loop's condition after a rejected trial
(optimization_algorithm_levenberg.cpp:149), and after the first optimize (:662: the second round is skipped, the final pass and the
write-back still run).  Both paths read the flag through one function, and the hook orbp_lba_set_stop_probe (csrc/orbp_internal.h)
calls back just before every read; the callback here counts the reads and sets the caller's flag before read number n, so every
case is deterministic.  The same sweep runs on the host path here and, marked gpu, on the GPU call against the host's answers.

What a stop between the rounds must leave is known independently: the flagging pass :672-702 and the final pass :715-743 apply one
test to the same stored errors and estimates, so the erase flags are the oracle's level-1 flags, and poses and points are the
oracle's after optimize(5).  The bar for those values is 4 x the spread of the oracle's two summation orders at that state, the
rule of tests/tools/measure_lba_spread.py, measured here because the tolerance file holds the spread of final results only."""
import ctypes as C

import numpy as np
import pytest

import lba_cases as lc
import lba_oracle as lo

CASE = "k2_p65_mixed"
PROBE = C.CFUNCTYPE(None, C.c_void_p)


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    orbx.lib()
    return orbx


def stopped_at(built, call, n, case=CASE):
    """call(problem, stop) with the flag set just before read number n of `stop` (n = 0: never) -> (result, number of reads)"""
    flag = np.zeros(1, np.uint8)
    reads = [0]

    def probe(_):
        reads[0] += 1
        if reads[0] == n:
            flag[0] = 1

    cb = PROBE(probe)
    built.lib().orbp_lba_set_stop_probe(C.cast(cb, C.c_void_p), None)
    try:
        res = call(lc.case(case), flag)
    finally:
        built.lib().orbp_lba_set_stop_probe(None, None)
    return res, reads[0]


_SWEEP = {}


def sweep_of(built, call, case):
    """the call stopped before each of its reads: {n: result}, n = 0 (never) .. number of reads + 1, and "reads": their number"""
    full, n_reads = stopped_at(built, call, 0, case)
    sweep = {0: full, "reads": n_reads}
    for n in range(1, n_reads + 2):
        sweep[n] = stopped_at(built, call, n, case)[0]
    return sweep


def host_sweep(built, case=CASE):
    if case not in _SWEEP:
        _SWEEP[case] = sweep_of(built, built.LocalBundleAdjustment, case)
    return _SWEEP[case]


def first_round(order):
    g = lo.Graph(lc.case(CASE), order)
    g.optimize(0, 5, {"iterations": [0, 0], "trials": [0, 0], "lambda": 0.0, "chi2": 0.0})
    return g


def check_sweep(sweep, n_reads, what):
    """what every stop position must give, from the reads' order alone"""
    full = sweep[0]
    it, tr = full[4]["iterations"], full[4]["trials"]
    # an accepted trial is not followed by a read; a rejected one (below 10 trials) is: one read a trial that is not its
    # iteration's last, and the entry, the tops of all iterations and the read between the rounds
    assert it == (5, 10) and n_reads == 2 + sum(it) + (sum(tr) - sum(it)), (what, full[4], n_reads)
    assert sweep[1][0] == 1, what                                           # ORBP_LBA_STOPPED at entry
    between = None
    for n in range(2, n_reads + 2):
        code, Tcw, xw, erase, st = sweep[n]
        assert code == 0 and np.isfinite(Tcw).all() and np.isfinite(xw).all() and (Tcw[:, 3, 3] == 1).all(), (what, n)   # written
        for r in (0, 1):
            assert st["iterations"][r] <= it[r] and st["trials"][r] <= tr[r], (what, n, st)
        if st["second_round"] == 0:
            assert st["iterations"][1] == 0 and st["trials"][1] == 0 and st["n_level1"] == 0, (what, n, st)
            if st["iterations"][0] == it[0] and st["trials"][0] == tr[0]:
                between = n if between is None else between
        else:
            assert st["iterations"][0] == it[0] and st["trials"][0] == tr[0] and st["n_level1"] == full[4]["n_level1"], (what, n, st)
        if n > 2:                                                           # a later stop never does less
            prev = sweep[n - 1][4]
            assert (prev["second_round"], prev["iterations"], prev["trials"]) <= (st["second_round"], st["iterations"], st["trials"]), (what, n)
    # stopped before the first iteration: nothing moved (a pose goes through the quaternion and back)
    assert sweep[2][4]["iterations"] == (0, 0) and np.array_equal(sweep[2][2], lc.case(CASE)["xw"]), what
    assert np.abs(sweep[2][1] - lc.case(CASE)["Tcw"][:len(sweep[2][1])]).max() <= 2.0 ** -22, what
    # every top of an iteration is a stop position of its own: the iteration counts 0 .. 4 and 0 .. 9 all occur
    seen = {(sweep[n][4]["second_round"], sweep[n][4]["iterations"]) for n in range(2, n_reads + 1)}
    assert {(0, (k, 0)) for k in range(5)} <= seen and {(1, (5, k)) for k in range(10)} <= seen, (what, sorted(seen))
    # a flag set after the last read changes nothing
    last = sweep[n_reads + 1]
    assert last[4] == full[4] and last[1].tobytes() == full[1].tobytes() and last[2].tobytes() == full[2].tobytes(), what
    assert np.array_equal(last[3], full[3]), what
    assert between is not None, what
    return between


def check_between_the_rounds(res, what):
    """stop set after the first optimize (:662-666): the final pass and the write-back ran on the first round's state"""
    code, Tcw, xw, erase, st = res
    f = lc.oracle(CASE)[0]
    gf, gr = first_round("forward"), first_round("reverse")
    K = len(Tcw)
    assert code == 0 and st["second_round"] == 0 and st["iterations"] == (5, 0) and st["n_level1"] == 0, (what, st)
    assert np.array_equal(erase, f["level1"]), what                          # one test on the same errors and estimates
    spread = (np.abs(np.asarray(gf.R)[:K] - np.asarray(gr.R)[:K]).max(), np.abs(np.asarray(gf.t)[:K] - np.asarray(gr.t)[:K]).max(),
              np.abs(gf.X - gr.X).max())
    got = (np.abs(Tcw[:, :3, :3] - np.asarray(gf.R)[:K]).max(), np.abs(Tcw[:, :3, 3] - np.asarray(gf.t)[:K]).max(), np.abs(xw - gf.X).max())
    size = (1.0, np.abs(np.asarray(gf.t)[:K]).max(), np.abs(gf.X).max())
    for name, d, s, m in zip(lc.KEYS, got, spread, size):
        allowed = 4 * s + 0.5 * lc.FLOAT_ULP * m
        print("%s: |d %s| = %.3g (4 x spread %.3g + float rounding %.3g)" % (what, name, d, 4 * s, allowed - 4 * s))
        assert d <= allowed, (what, name, d, allowed)
    moved = np.abs(xw - lc.case(CASE)["xw"]).max()
    assert moved > 1e-3, what                                               # and not the input's


def test_the_host_path_reads_stop_where_g2o_does(built):
    sweep = host_sweep(built)
    between = check_sweep(sweep, sweep["reads"], "host")
    assert between == 2 + 5 + (sweep[0][4]["trials"][0] - 5)
    check_between_the_rounds(sweep[between], "host")


def check_rejected_trials(sweep, what):
    """the trial loop's condition (optimization_algorithm_levenberg.cpp:149), on the case whose first round rejects trials: a flag
    set before the read that follows a rejected trial ends the iteration there, counted, with the estimates popped back to those
    at the iteration's top; the next top then ends the round"""
    full = sweep[0][4]
    rejected = sum(full["trials"]) - sum(full["iterations"])
    assert rejected > 0 and full["iterations"][1] == 0 and sweep["reads"] == 2 + full["iterations"][0] + rejected, (what, full)
    hits = 0
    for n in range(3, sweep["reads"]):
        st, nxt = sweep[n][4], sweep[n + 1][4]
        if not (st["iterations"][0] == nxt["iterations"][0] and st["trials"][0] < nxt["trials"][0]):
            continue                        # a top, or the read between the rounds
        hits += 1
        top = max(k for k in range(2, n) if sweep[k][4]["iterations"][0] == st["iterations"][0] - 1)
        assert st["second_round"] == 0 and st["trials"][0] > sweep[top][4]["trials"][0], (what, n)
        assert sweep[n][1].tobytes() == sweep[top][1].tobytes() and sweep[n][2].tobytes() == sweep[top][2].tobytes(), (what, n, top)
    assert hits == rejected, (what, hits, rejected)


def test_a_rejected_trial_is_followed_by_a_read(built):
    check_rejected_trials(host_sweep(built, "no_free"), "host")


@pytest.mark.gpu
def test_the_gpu_call_reads_stop_where_the_host_does(built):
    m = built.ORBmatcher(0.8, True, max_queries=64, max_train=64, max_pairs=256)
    try:
        sweep = sweep_of(built, m.local_bundle_adjustment, CASE)
        rejecting = sweep_of(built, m.local_bundle_adjustment, "no_free")
    finally:
        m.close()
    between = check_sweep(sweep, sweep["reads"], "gpu")
    check_between_the_rounds(sweep[between], "gpu")
    check_rejected_trials(rejecting, "gpu")
    for case, got in ((CASE, sweep), ("no_free", rejecting)):               # the host's decisions at every stop position
        host = host_sweep(built, case)
        assert got["reads"] == host["reads"], case
        for n in range(1, got["reads"] + 2):
            assert got[n][0] == host[n][0], (case, n)
            assert all(got[n][4][k] == host[n][4][k] for k in ("iterations", "trials", "n_level1", "second_round")), (case, n)
