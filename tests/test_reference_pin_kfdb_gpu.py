"""GPU parity against the reference's own src/KeyFrameDatabase.cc: the library (include/orbk.h: the scoring kernel of
csrc/orbk.hip and the host's reconstruction of the reference's loops from one record per key frame) and the C++ adapter
(my-slam_amd/host/KeyFrameDatabase.cc) == oracle/_ref/ref_kfdb, the reference's file compiled unmodified, with no step
through the restatement.  orbk_query_begin's list is compared with the reference's lScoreAndMatch (ids and float bits),
orbk_query_end's candidates with the reference's.  The handle's per-key-frame state has no getter: it is checked by
continuing the sequence (repeated query ids, neighbours that read stale scores, erase / clear / re-add in the cases).
ref_kfdb is a CPU program that build() leaves under oracle/_ref/; apart from it these tests read nothing of the reference,
and the last one (recorded outputs under tests/golden/kfdb/) does not need it either.

Each kernel-edge test first asserts, from the case's inputs alone, the condition that makes it meaningful."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import ref_kfdb as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pinned():
    out = R.pinned_cases()
    if out is None:
        pytest.skip("oracle/_ref/ref_kfdb was not built (build() compiles it where the reference tree is present)")
    return out


def check_queries(name, ref, got):
    rq = R.queries(ref)
    assert len(got) == len(rq), name
    for i, (a, b) in enumerate(zip(rq, got)):
        assert [k for k, _ in b[2]] == [k for k, _ in a[2]], "%s: orbk_query_begin ids of query %d" % (name, i)
        assert b[2] == a[2], "%s: orbk_query_begin score bits of query %d" % (name, i)
        assert b[1] == a[1], "%s: orbk_query_end candidates of query %d" % (name, i)
    return len(rq)


def run_case(orbx, c, ref, **kw):
    return check_queries(c.name, ref[c.name], R.run_library(orbx, c.ops, **c.handle, **kw))


def edge(pinned, name):
    _, ec, ref = pinned
    return next(c for c in ec if c.name == name), ref


def test_control_flow_equals_reference(orbx, pinned):
    """Query ids 0 / repeated / shared with the database, connected key frames, the 0.8f truncation, minScore at and one ulp
    above a score, neighbour lists around the ten the reference takes, stale scores of erased key frames, the strict
    0.75f retention, ties, zero scores, empty inputs, clear and refill, encounter order through erase, re-add and arena
    compaction, and three seeded sequences (one on a handle of 4 slots and 16 entries)."""
    cc, _, ref = pinned
    nq = sum(run_case(orbx, c, ref) for c in cc)
    assert nq == sum(c.nqueries for c in cc) and nq > 500
    comp = next(c for c in cc if c.name == "compaction_order")
    assert comp.facts["compactions"] == [0, 1, 2, 3] and comp.handle == dict(max_keyframes=4, max_entries=16)


def test_detect_calls_equal_reference(orbx, pinned):
    """DetectRelocalizationCandidates / DetectLoopCandidates of the Python binding against the reference's candidates."""
    cc, _, ref = pinned
    for c in cc:
        got = R.run_library(orbx, c.ops, detect=True, **c.handle)
        assert [g[1] for g in got] == [q[1] for q in R.queries(ref[c.name])], c.name


def test_chunk_edges_equal_reference(orbx, pinned):
    """BowVectors of 0, 1, 63, 64, 65, 128 and 129 entries with the shared words at lane 0 and lane 63 only, in the first
    chunk only, in the second chunk only (the first ballot is 0), in the last entry only, and in every other entry of three
    chunks (the lane-ordered sum)."""
    c, ref = edge(pinned, "chunks")
    f = c.facts
    assert [n for n, _ in f["second_chunk"]] == [65, 128, 129] and all(64 <= p < 128 for _, ps in f["second_chunk"] for p in ps)
    assert all(ps == [0, 63] for _, ps in f["lane0_lane63"]) and [n for n, _ in f["lane0_lane63"]] == [64, 65, 128, 129]
    assert all(ps == [n - 1] for n, ps in f["last_entry"]) and [n for n, _ in f["last_entry"]] == [1, 63, 64, 65, 128, 129]
    assert all(n == 129 and len(ps) == 65 for n, ps in f["dense"]) and len(f["dense"]) == 3
    assert run_case(orbx, c, ref) == 10


def test_prefilter_edges_equal_reference(orbx, pinned):
    """Key-frame words equal to the query's smallest and largest word and one outside each."""
    c, ref = edge(pinned, "prefilter")
    assert run_case(orbx, c, ref) == 4


def test_long_queries_equal_reference(orbx, pinned):
    """Queries of 1, 8192 (the longest staged in LDS) and 8193 words (searched in global memory)."""
    c, ref = edge(pinned, "long_queries")
    lens = c.facts["query_lengths"]
    assert lens == [1, R.LDS_QUERY, R.LDS_QUERY + 1] and lens[2] > R.LDS_QUERY and c.ops[0][1] >= R.LDS_QUERY + 1
    assert run_case(orbx, c, ref) == 6


@pytest.fixture(scope="module")
def slots_run(orbx, pinned):
    """The 16389-key-frame database is built once: the case's script through the library, with the live count the handle
    reports at every query."""
    c, ref = edge(pinned, "slots")
    live = []
    got = R.run_library(orbx, c.ops, on_query=lambda i, db: live.append(len(db)), **c.handle)
    return c, ref, got, live


def test_slot_stride_equals_reference(slots_run):
    """8191, 8192, 8193 and 16389 slots with dead ones among them: the waves of the launch take a second and a third trip."""
    c, ref, got, live = slots_run
    slots = c.facts["slots"]
    assert slots == [n for n in R.SLOT_COUNTS for _ in (0, 1)]           # from the script: one slot per add, no compaction
    assert slots[2] == R.WAVES and slots[4] > R.WAVES and slots[6] > 2 * R.WAVES
    assert live == c.facts["live"] and all(l < s for l, s in zip(live, slots))      # dead slots at every query
    assert check_queries(c.name, ref[c.name], got) == 8
    assert max(k for k, _ in got[-1][2]) > 2 * R.WAVES                    # the list reaches the third trip's key frames


def test_second_record_download_equals_reference(orbx, pinned):
    """A query with 7 records, then one with 330 (more than come back with the counter), then the first again."""
    c, ref = edge(pinned, "second_download")
    na, nb, nc = c.facts["records"]
    assert na < 10 and nb > 300 and nc == na and nb > max(R.REC_GUESS, na + na // 4)     # numpy counts, from the inputs
    assert run_case(orbx, c, ref) == 6


@pytest.fixture(scope="module")
def adapter(orbx, tmp_path_factory):
    """tests/cxx/kfdb_callsites.cc over host/KeyFrameDatabase.h, built as test_cxx_adapter_equals_the_restatement does,
    against the library build() left (a missing library is an error, not a reason to compile it here)."""
    orbx.lib()
    exe = str(tmp_path_factory.mktemp("kfdb_adapter") / "kfdb_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "kfdb_shims"),
           "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + inc + [os.path.join(ROOT, "tests", "cxx", "kfdb_callsites.cc"),
                                                              os.path.join(ROOT, "my-slam_amd", "host", "KeyFrameDatabase.cc"), "-o", exe,
                                                              "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    return exe


def check_adapter(exe, cases, ref):
    """Every case's script (without its dumps) through the adapter, a few processes at a time: its candidate lines are
    the reference's."""
    def run(c):
        return subprocess.run([exe], input=R.text(c.ops, dumps=False), capture_output=True, text=True, timeout=R.TIMEOUT)
    with ThreadPoolExecutor(4) as pool:
        results = list(pool.map(run, cases))
    n = 0
    for c, r in zip(cases, results):
        assert r.returncode == 0, (c.name, r.stderr)
        got = [[int(x) for x in l.split()] for l in r.stdout.split("\n")[:-1]]
        assert got == [q[1] for q in R.queries(ref[c.name])], c.name
        n += len(got)
    return n


def test_cxx_adapter_equals_reference_on_control_flow(adapter, pinned):
    """The adapter cuts the neighbour lists of 11 and 13 to ten itself, and keeps the query state in the handle."""
    cc, _, ref = pinned
    assert check_adapter(adapter, cc, ref) > 500


def test_cxx_adapter_equals_reference_on_kernel_edges(adapter, pinned):
    _, ec, ref = pinned
    assert check_adapter(adapter, ec, ref) == sum(c.nqueries for c in ec)


def test_golden_scripts_equal_their_recorded_reference_output(orbx):
    """tests/golden/kfdb/: a control-flow script and a kernel-edge script with ref_kfdb's recorded output."""
    n = 0
    for name in ("control", "edges"):
        ops = R.parse(open(os.path.join(R.GOLDEN, name + ".script")).read())
        ref = R.parse_output(open(os.path.join(R.GOLDEN, name + ".out")).read())
        n += check_queries(name, ref, R.run_library(orbx, ops))
    assert n == 61
