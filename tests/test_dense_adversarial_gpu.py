"""The dense / batched / CSR best-and-second-best kernels and the acceptance on the planted cases of dense_cases.py: ties across
every adjacent-row boundary, across a train part and the 4096-row index chunk, the far end of the distance range, counts that are
no multiple of anything, rows beyond the counts that are exact copies of live rows, and the acceptance on its boundaries.  Integer
work throughout: the bar is equality with the numpy restatement (which tests/test_dense_cases_cpu.py holds against the C oracle on
the same inputs).

The kernel switches are read once per process or handle, so the whole file runs again in fresh child processes with
ORBM_MFMA_SPLITS, ORBM_MFMA_SP and ORBM_DENSE=popcount set (the tests at the end)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as DC

pytestmark = pytest.mark.gpu

CHILD_MARK = "ORBM_DENSE_CASES_CHILD"
_abnormal = []      # why nothing more is started on the GPU: the first error of the runtime in process, or the first child that ended
                    # by signal or timeout


def _gpu_step(fn):
    """An in-process test that ends in anything but a failed comparison (an error from the HIP runtime, say) bars the child runs."""
    @functools.wraps(fn)
    def run(*a, **kw):
        try:
            return fn(*a, **kw)
        except AssertionError:
            raise
        except Exception as e:
            _abnormal.append("%s ended in process with %s: %s" % (fn.__name__, type(e).__name__, str(e)[:200]))
            raise
    return run


@pytest.fixture(scope="module")
def matcher(orbx):
    """ONE handle for every case of this file, in file order: large and small shapes in turn, so that partials or results left by
    a wider earlier launch would show."""
    m = _gpu_step(orbx.ORBmatcher)(0.9, False)
    yield m
    m.close()


def _assert_same(got, ref, what):
    for name, x, y in zip(("best_idx", "best_d", "second_d"), got, ref):
        if not np.array_equal(x, y):
            bad = np.argwhere(np.asarray(x) != np.asarray(y))
            k = tuple(int(v) for v in bad[0])
            pytest.fail("%s: %s differs at %d places, first at %s: kernel %d, reference %d (best_idx / best_d / second_d there: "
                        "kernel %s, reference %s)" % (what, name, len(bad), k, x[k], y[k], [int(a[k]) for a in got], [int(a[k]) for a in ref]))


# ---- host API, dense ----
@pytest.mark.parametrize("name", DC.DENSE_NAMES)
@_gpu_step
def test_dense_planted(matcher, name):
    q, t, facts = DC.dense_case(name)
    ref = DC.check_facts(q, t, facts)
    _assert_same(matcher.best2(q, t), ref, name)


@_gpu_step
def test_dense_shapes(matcher):
    """nq around the query-block and workgroup sizes x nt around the tile and stage sizes (0 included), the winner in the last row."""
    for nq, nt in DC.shape_cases():
        q, t, facts = DC.shape_case(nq, nt)
        ref = DC.check_facts(q, t, facts)
        _assert_same(matcher.best2(q, t), ref, "nq=%d nt=%d" % (nq, nt))


# ---- host API, candidate lists ----
@_gpu_step
def test_csr_planted(matcher):
    c = DC.csr_case()
    ref = DC.ref_best2(c["q"], c["t"], c["off"], c["idx"])
    got = matcher.best2(c["q"], c["t"], c["off"], c["idx"])
    bad = np.flatnonzero((got[0] != ref[0]) | (got[1] != ref[1]) | (got[2] != ref[2]))
    if bad.size:
        i = int(bad[0])
        pytest.fail("list %d (length, positions, kind) = %s: kernel %s, reference %s" % (i, c["plan"][i], [int(a[i]) for a in got], [int(a[i]) for a in ref]))
    _assert_same(got, ref, "csr")


# ---- device-resident batches ----
_dev = {}


def _device_batch(name):
    import torch
    if name not in _dev:
        c = DC.batch_case(name)
        nb, cap = len(c["nqs"]), c["cap"]
        _dev[name] = dict(c=c, ref=DC.batch_reference(c), nb=nb, cap=cap,
                          q=torch.from_numpy(c["q"]).cuda(), t=torch.from_numpy(c["t"]).cuda(),
                          nq=torch.from_numpy(c["nqs"]).cuda(), nt=torch.from_numpy(c["nts"]).cuda(),
                          kp=torch.zeros((nb, cap, 7), dtype=torch.float32).cuda())       # every angle equal
    return _dev[name]


@pytest.mark.parametrize("name", ["chunk", "counts", "accept"])
@_gpu_step
def test_best2_batch_device(matcher, name):
    import torch
    d = _device_batch(name)
    out = [torch.full((d["nb"], d["cap"]), -7, dtype=torch.int32).cuda() for _ in range(3)]
    matcher.best2_batch_device(d["q"].data_ptr(), d["nq"].data_ptr(), d["t"].data_ptr(), d["nt"].data_ptr(), d["cap"], d["nb"],
                               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    torch.cuda.synchronize()
    _assert_same([o.cpu().numpy() for o in out], d["ref"], name)       # beyond the counts: -1 / 256 / 256


def _match_runs(name):
    if name == "accept":
        return [(th, r, ori) for r in DC.NNRATIOS for th in (50, 45, 27) for ori in (False, True)]
    return [(50, 0.9, False), (50, 0.9, True), (50, 0.6, False)]


@pytest.mark.parametrize("name", ["chunk", "counts", "accept"])
@_gpu_step
def test_match_batch_device(matcher, name):
    """Acceptance (bd == th against th + 1, the float32 ratio test at its equalities) on the merged partials; with the rotation
    check off, and on with every angle equal (one histogram bin: nothing may be culled)."""
    import torch
    d = _device_batch(name)
    bi, bd, sd = d["ref"]
    nb, cap = d["nb"], d["cap"]
    try:
        for th, nnratio, ori in _match_runs(name):
            want_m, want_n = np.full((nb, cap), -1, np.int32), np.zeros(nb, np.int32)
            for b in range(nb):
                nq = int(d["c"]["nqs"][b])
                want_m[b, :nq], want_n[b] = DC.ref_accept(bi[b, :nq], bd[b, :nq], sd[b, :nq], th, nnratio)
            m12 = torch.full((nb, cap), -7, dtype=torch.int32).cuda()
            nm = torch.full((nb,), -7, dtype=torch.int32).cuda()
            matcher.mfNNratio, matcher.mbCheckOrientation = nnratio, ori
            matcher.match_batch_device(d["q"].data_ptr(), d["kp"].data_ptr(), d["nq"].data_ptr(), d["t"].data_ptr(), d["kp"].data_ptr(),
                                       d["nt"].data_ptr(), cap, nb, m12.data_ptr(), nm.data_ptr(), th=th)
            torch.cuda.synchronize()
            got_m, got_n = m12.cpu().numpy(), nm.cpu().numpy()
            what = "%s th=%d nnratio=%s checkOri=%s" % (name, th, nnratio, ori)
            if not np.array_equal(got_m, want_m):
                k = tuple(int(v) for v in np.argwhere(got_m != want_m)[0])
                pytest.fail("%s: match12%s is %d, reference %d (bd %d, sd %d)" % (what, k, got_m[k], want_m[k], bd[k], sd[k]))
            assert np.array_equal(got_n, want_n), "%s: nmatches %s, reference %s" % (what, got_n, want_n)
    finally:
        matcher.mfNNratio, matcher.mbCheckOrientation = 0.9, False


@_gpu_step
def test_dense_after_batches(matcher):
    """The host path once more after the batched launches have left their wider partials in the handle."""
    for name in ("sweep_gap1_tie", "chunk8300_gap1_unequal", "identical2_d0"):
        q, t, facts = DC.dense_case(name)
        _assert_same(matcher.best2(q, t), DC.check_facts(q, t, facts), name)


# ---- the same file under the kernel switches, each in a fresh process ----
VARIANTS = [
    # (the in-loop chunk fold of k_best2_mfma already runs in process: at the default split counts row 4096 lies inside part 18 of 43
    # at nt = 8300 and inside part 21 of 22 of the cap = 4200 batch)
    {"ORBM_MFMA_SPLITS": "1"},                          # one workgroup walks all 8300 train rows: two chunk folds in one tile loop
    {"ORBM_MFMA_SPLITS": "2"},
    {"ORBM_MFMA_SP": "1"},                              # k_best2_mfma_sp
    {"ORBM_MFMA_SP": "1", "ORBM_MFMA_SPLITS": "1"},
    {"ORBM_DENSE": "popcount"},                         # k_best2_dense
]


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: "-".join("%s=%s" % kv for kv in sorted(e.items())))
def test_variant_in_fresh_process(env):
    if os.environ.get(CHILD_MARK):
        pytest.fail("a variant run must not start variant runs")
    if _abnormal:
        pytest.fail("not started: %s" % _abnormal[0])
    here = os.path.abspath(__file__)
    child_env = dict(os.environ, **env)
    child_env[CHILD_MARK] = "1"
    cmd = [sys.executable, "-m", "pytest", here, "-q", "-m", "gpu", "-k", "not variant", "-p", "no:cacheprovider"]
    try:
        p = subprocess.run(cmd, env=child_env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                           cwd=os.path.dirname(os.path.dirname(here)))
    except subprocess.TimeoutExpired as e:
        _abnormal.append("the run with %s did not end within 600 s" % env)
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        pytest.fail("%s\n%s" % (_abnormal[0], out[-2000:]))
    if p.returncode < 0 or p.returncode >= 128:         # ended by a signal (directly, or as a shell would report it)
        _abnormal.append("the run with %s ended abnormally (exit status %d)" % (env, p.returncode))
        pytest.fail("%s\n%s" % (_abnormal[0], p.stdout[-2000:]))
    assert p.returncode == 0, p.stdout[-4000:]
    assert " passed" in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
