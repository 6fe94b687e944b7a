"""Client of oracle/_ref/ref_kfdb (the reference's own src/KeyFrameDatabase.cc, compiled unmodified behind the stand-in
KeyFrame / Frame of oracle/ref/kfdb_standin.h; script and output formats in oracle/ref/ref_kfdb.cc), the runners that feed
the same script to the restatement (tests/kfdb_oracle.py) and to the library (include/orbk.h), and the case list of
tests/test_reference_pin_kfdb_cpu.py and _gpu.py.

A case is a script in the language of tests/cxx/kfdb_callsites.cc plus "dump", so one text feeds the reference, the
restatement, the C ABI and the C++ adapter.  Every planted case proves what it planted from its inputs (numpy
intersections, exact dyadic arithmetic, slot_trace() over the script) when it is built, or from the reference's output in
its `proof` callable; never from the code under test.

Rules every script keeps, because the reference is undefined or differs from the library there (include/orbk.h): no word
id >= the vocabulary size, no add of a key frame that is already in the database, and a key frame's BowVector changes only
while it is outside the database (the reference's erase walks the current mBowVec)."""
import os
import subprocess

import numpy as np

import kfdb_oracle as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(REF_OUT, "ref_kfdb")
EXE_UBSAN = os.path.join(REF_OUT, "ref_kfdb_ubsan")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kfdb")
TIMEOUT = 120          # seconds; no run of a reference program goes without one
F32 = np.float32
NEIGHBOURS = 10        # GetBestCovisibilityKeyFrames(10), src/KeyFrameDatabase.cc:151 and :265

LDS_QUERY = 8192       # K_LDS_QUERY of orbk.hip: longer queries search global memory
WAVES = 8192           # 4 * K_MAX_BLOCKS of orbk.hip: with more slots than this a wave takes a second trip
REC_GUESS = 256        # run_score copies back max(rec_hint, 256) records with the counter


def ensure(allow_build=True):
    """Path to ref_kfdb, building it when it is missing and the reference exists; None when neither exists."""
    if os.path.exists(EXE) and os.path.exists(EXE_UBSAN):
        return EXE
    if not allow_build:
        return None
    import ref_pin
    if os.path.exists(os.path.join(ref_pin.reference_dir(), "src", "KeyFrameDatabase.cc")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref"), "kfdb"])
        return EXE
    return None


# ---- scripts

def bow(b):
    """A BowVector from a {word: value} dict or an (ids, values) pair: ascending int32 ids, float64 values."""
    if isinstance(b, dict):
        ks = sorted(b)
        return np.array(ks, np.int32), np.array([b[k] for k in ks], np.float64)
    return np.asarray(b[0], np.int32), np.asarray(b[1], np.float64)


def _fmt_bow(b):
    ids, vals = b
    return "%d%s" % (len(ids), "".join(" %d %.17g" % (w, v) for w, v in zip(ids.tolist(), vals.tolist())))


class Script:
    """Builds the op list.  With auto_dump a dump follows every command after the definitions."""

    def __init__(self, nwords, auto_dump=True):
        self.ops = [("words", nwords)]
        self.auto_dump = auto_dump

    def _d(self):
        if self.auto_dump:
            self.ops.append(("dump",))

    def kf(self, kid, b):
        self.ops.append(("kf", kid, bow(b)))

    def covis(self, kid, ids):
        self.ops.append(("covis", kid, [int(x) for x in ids]))

    def conn(self, kid, ids):
        self.ops.append(("conn", kid, [int(x) for x in ids]))

    def add(self, *kids):
        for k in kids:
            self.ops.append(("add", k)); self._d()

    def erase(self, *kids):
        for k in kids:
            self.ops.append(("erase", k)); self._d()

    def clear(self):
        self.ops.append(("clear",)); self._d()

    def reloc(self, qid, b):
        self.ops.append(("reloc", qid, bow(b))); self._d()

    def loop(self, kid, min_score=0.0):
        self.ops.append(("loop", kid, F32(min_score))); self._d()

    def dump(self):
        self.ops.append(("dump",))


def text(ops, dumps=True):
    """The script text; without dumps it is what tests/cxx/kfdb_callsites.cc reads."""
    out = []
    for op in ops:
        c = op[0]
        if c == "words":
            out.append("words %d" % op[1])
        elif c == "kf" or c == "reloc":
            out.append("%s %d %s" % (c, op[1], _fmt_bow(op[2])))
        elif c == "covis" or c == "conn":
            out.append("%s %d %d%s" % (c, op[1], len(op[2]), "".join(" %d" % x for x in op[2])))
        elif c == "add" or c == "erase":
            out.append("%s %d" % (c, op[1]))
        elif c == "loop":
            out.append("loop %d %.9g" % (op[1], op[2]))
        elif c == "clear":
            out.append("clear")
        elif c == "dump":
            if dumps:
                out.append("dump")
        else:
            raise ValueError(c)
    return "\n".join(out) + "\n"


def parse(script):
    """The op list of a script text (the inverse of text())."""
    ops = []
    for line in script.split("\n"):
        t = line.split()
        if not t:
            continue
        c = t[0]
        if c == "words":
            ops.append((c, int(t[1])))
        elif c == "kf" or c == "reloc":
            n = int(t[2])
            assert len(t) == 3 + 2 * n
            ops.append((c, int(t[1]), (np.array(t[3::2], np.int64).astype(np.int32), np.array([float(x) for x in t[4::2]], np.float64))))
        elif c == "covis" or c == "conn":
            assert len(t) == 3 + int(t[2])
            ops.append((c, int(t[1]), [int(x) for x in t[3:]]))
        elif c == "add" or c == "erase":
            ops.append((c, int(t[1])))
        elif c == "loop":
            ops.append((c, int(t[1]), F32(t[2])))
        elif c == "clear" or c == "dump":
            ops.append((c,))
        else:
            raise ValueError(line[:40])
    return ops


# ---- events: what a run of a script produces
# ("q", candidates, [(id, score bits)], min_common or None)   per reloc / loop
# ("d", {id: (mnLoopQuery, mnLoopWords, mLoopScore bits, mnRelocQuery, mnRelocWords, mRelocScore bits)})   per dump

def parse_output(out):
    ev, dump, lines = [], None, out.split("\n")
    assert lines[-1] == "", "the output does not end with a newline"
    i = 0
    while i < len(lines) - 1:
        t = lines[i].split()
        if t[0] == "C":
            l = lines[i + 1].split()
            assert l[0] == "L"
            ev.append(("q", [int(x) for x in t[1:]], [(int(a), int(b, 16)) for a, b in (x.split(":") for x in l[1:])], None))
            i += 2
            continue
        if t[0] == "D":
            dump = {} if dump is None else dump
            dump[int(t[1])] = (int(t[2]), int(t[3]), int(t[4], 16), int(t[5]), int(t[6]), int(t[7], 16))
        elif t[0] == "E":
            ev.append(("d", dump or {}))
            dump = None
        else:
            raise ValueError(lines[i][:40])
        i += 1
    assert dump is None
    return ev


def run_ref_text(script, exe=None):
    """One process of ref_kfdb (or exe) on a script text; returns its standard output.  A non-zero exit raises
    CalledProcessError (status 2: the driver refused the script; the UBSan build exits at the first undefined operation)."""
    exe = exe or EXE
    p = subprocess.run([exe], input=script, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    if p.returncode != 0:
        raise subprocess.CalledProcessError(p.returncode, [exe], p.stdout, p.stderr)
    return p.stdout


def run_ref(ops, exe=None):
    return parse_output(run_ref_text(text(ops), exe))


def queries(ev):
    return [e for e in ev if e[0] == "q"]


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


class World:
    """What a script has defined so far: BowVectors, covisibility orders and connected sets, by key-frame id."""

    def __init__(self):
        self.bows, self.cov, self.con, self.known = {}, {}, {}, set()

    def define(self, op):
        c = op[0]
        if c == "kf":
            self.bows[op[1]] = op[2]
            self.known.add(op[1])
        elif c == "covis":
            self.cov[op[1]] = op[2]
            self.known.update([op[1]] + op[2])
        elif c == "conn":
            self.con[op[1]] = op[2]
            self.known.update([op[1]] + op[2])
        elif c in ("add", "erase", "loop"):
            self.known.add(op[1])
        else:
            return False
        return c in ("kf", "covis", "conn")

    def bow_of(self, kid):
        return self.bows.get(kid, (np.zeros(0, np.int32), np.zeros(0, np.float64)))

    def covis10(self, ids):
        return {int(k): self.cov.get(int(k), [])[:NEIGHBOURS] for k in ids}


def run_oracle(ops):
    """The script through tests/kfdb_oracle.py; the events carry minCommonWords."""
    w, db, ev = World(), None, []
    for op in ops:
        c = op[0]
        if c == "words":
            db = K.KeyFrameDatabase(op[1])
        elif w.define(op):
            pass
        elif c == "add":
            db.add(op[1], w.bow_of(op[1]))
        elif c == "erase":
            db.erase(op[1])
        elif c == "clear":
            db.clear()
        elif c == "reloc" or c == "loop":
            loop = c == "loop"
            q = w.bow_of(op[1]) if loop else op[2]
            con = w.con.get(op[1], []) if loop else []
            ms = float(op[2]) if loop else 0.0
            scored, mc = db.query_begin(loop, op[1], q, con, ms)
            cand = db.query_end(loop, op[1], scored, mc, w.covis10([k for _, k in scored]), ms)
            ev.append(("q", cand, [(k, _bits(s)) for s, k in scored], mc))
        elif c == "dump":
            fresh = K.KF(0)
            st = {}
            for kid in sorted(w.known):
                k = db.kfs.get(kid, fresh)
                st[kid] = (k.mnLoopQuery, k.mnLoopWords, _bits(k.mLoopScore), k.mnRelocQuery, k.mnRelocWords, _bits(k.mRelocScore))
            assert set(db.kfs) <= w.known
            ev.append(("d", st))
    return ev


def run_library(orbx, ops, max_keyframes=1024, max_entries=1 << 20, on_query=None, detect=False):
    """The script through the C ABI: orbk_query_begin's list and orbk_query_end's candidates per query, or with detect the
    candidates of the binding's DetectRelocalizationCandidates / DetectLoopCandidates.  Dumps are skipped: the handle's
    per-key-frame state is visible only through the queries that follow."""
    w, ev, db = World(), [], None
    for op in ops:
        c = op[0]
        if c == "words":
            db = orbx.KeyFrameDatabase(op[1], max_keyframes=max_keyframes, max_entries=max_entries)
        elif w.define(op) or c == "dump":
            pass
        elif c == "add":
            db.add(op[1], w.bow_of(op[1]))
        elif c == "erase":
            db.erase(op[1])
        elif c == "clear":
            db.clear()
        elif c == "reloc" or c == "loop":
            loop = c == "loop"
            kind = orbx.ORBK_LOOP if loop else orbx.ORBK_RELOC
            q = w.bow_of(op[1]) if loop else op[2]
            if detect:
                cov = {k: v[:NEIGHBOURS] for k, v in w.cov.items()}
                ev.append(("q", db.DetectLoopCandidates(op[1], q, w.con.get(op[1], []), float(op[2]), cov) if loop else
                           db.DetectRelocalizationCandidates(op[1], q, cov), None, None))
                continue
            ids, si = db.query_begin(kind, op[1], q, w.con.get(op[1], []) if loop else [], float(op[2]) if loop else 0.0)
            cand = db.query_end(kind, ids, w.covis10(ids))
            ev.append(("q", cand, list(zip([int(x) for x in ids], si.view(np.uint32).tolist())), None))
            if on_query:
                on_query(len(ev) - 1, db)
    return ev


def slot_trace(ops, max_keyframes=1024, max_entries=1 << 20):
    """Per query: (slots in the handle's table, live key frames, compactions so far) when it runs, from the script and the
    growth rule of orbk_create / orbk_make_room alone: a slot per add, erased slots stay until an add finds the table or the
    arena full, then the dead ones go and the capacities become max(old, 2 * (live + the new one))."""
    w = World()
    cap_s, cap_e = max(max_keyframes, 4), max(max_entries, 256)
    slots, tail, ncompact, out, live = [], 0, 0, [], {}       # slots: [id, len, live]
    for op in ops:
        c = op[0]
        if w.define(op):
            continue
        if c == "add":
            n = len(w.bow_of(op[1])[0])
            assert op[1] not in live, "add of a key frame that is in the database"
            if not (len(slots) < cap_s and tail + n <= cap_e):
                slots = [s for s in slots if s[2]]
                live_e = sum(s[1] for s in slots)
                cap_e, cap_s = max(cap_e, 2 * (live_e + n)), max(cap_s, 2 * (len(slots) + 1))
                tail = live_e
                ncompact += 1
            slots.append([op[1], n, True])
            live[op[1]] = slots[-1]
            tail += n
        elif c == "erase":
            if op[1] in live:
                live.pop(op[1])[2] = False
        elif c == "clear":
            slots, tail, live = [], 0, {}
        elif c == "reloc" or c == "loop":
            out.append((len(slots), len(live), ncompact))
    return out


def shared(q, b):
    """Positions in the key frame's vector b and in the query q of their common words (numpy, from the inputs)."""
    _, iq, ib = np.intersect1d(bow(q)[0], bow(b)[0], assume_unique=True, return_indices=True)
    return np.sort(ib), np.sort(iq)


def l1_values(rng, n):
    """Non-dyadic positive values, L1-normalised as the vocabulary produces them: summation order matters."""
    v = rng.random(n) + 1e-3
    return v / v.sum()


class Case:
    def __init__(self, name, script, handle=None, proof=None, facts=None):
        self.name, self.ops = name, script.ops if isinstance(script, Script) else script
        self.handle = handle or {}
        self.proof = proof          # proof(reference events): asserts what the case planted, from the reference's output
        self.facts = facts or {}    # what was proved from the inputs when the case was built
        ids = [i for op in self.ops if op[0] in ("kf", "reloc") for i in op[2][0].tolist()]
        assert not ids or (0 <= min(ids) and max(ids) < self.ops[0][1]), "word id beyond the vocabulary"
        slot_trace(self.ops, **self.handle)        # asserts no double add

    @property
    def text(self):
        return text(self.ops)

    @property
    def nqueries(self):
        return sum(op[0] in ("reloc", "loop") for op in self.ops)


# ---- control flow: small databases, dyadic values where a threshold is planted

def _ids(q):
    return [k for k, _ in q[2]]


def case_query_ids():
    s = Script(64)
    s.kf(1, {1: 0.5}); s.kf(2, {2: 0.5}); s.kf(3, {1: 0.25, 2: 0.25}); s.kf(9, {1: 0.5, 2: 0.5}); s.kf(0, {1: 0.5})
    s.add(1, 2, 3)
    s.reloc(0, {1: 0.5, 2: 0.5})        # 0: query id 0 on fresh key frames: mnRelocQuery == 0 already, nothing pushed
    s.loop(0)                           # 1: the same for mnLoopQuery
    s.loop(9)                           # 2: pushes 1, 2, 3
    s.loop(9)                           # 3: the same loop query again: nothing pushed, counts accumulate
    s.reloc(4, {1: 0.5, 2: 0.5})        # 4
    s.reloc(4, {2: 0.25, 5: 0.5})       # 5: a second relocalisation with the same frame id
    s.loop(3)                           # 6: the query key frame is in the database: it scores against itself
    s.reloc(0, {1: 0.5})                # 7: id 0 once the key frames carry another id: pushed

    def proof(ev):
        q = queries(ev)
        assert q[0][1:3] == ([], []) and q[1][1:3] == ([], [])
        d = [e[1] for e in ev if e[0] == "d"]
        assert d[3][3][4] == 2 and d[3][3][3] == 0          # after query 0: key frame 3 counted 2 words under id 0
        assert _ids(q[2]) == [3] and q[3][1:3] == ([], [])  # 3 shares two words, 1 and 2 one: int(2 * 0.8f) = 1
        assert q[5][2] == [] and 3 in _ids(q[6]) and _ids(q[7]) == [1, 3]
    return Case("query_ids", s, proof=proof)


def case_connected():
    s = Script(64)
    s.kf(1, {w: 0.125 for w in (1, 2, 3, 4)}); s.kf(2, {1: 0.25, 2: 0.25}); s.kf(3, {3: 0.5})
    for k in (10, 12):
        s.kf(k, {w: 0.25 for w in (1, 2, 3, 4)})
    s.conn(10, [1]); s.covis(2, [1, 3]); s.covis(3, [1])
    s.add(1, 2, 3)
    s.loop(10)          # 0: 1 is connected and shares four words: never pushed, its count reads 1 afterwards
    s.conn(10, [])
    s.loop(10)          # 1: same id, 1 no longer connected: pushed now with 4; 2 and 3 accumulate, unpushed
    s.loop(12)          # 2: not connected in A ...
    s.conn(12, [1, 2])
    s.loop(12)          # 3: ... connected in B of the same id: mnLoopQuery == 12 already, the set is never looked at

    def proof(ev):
        q = queries(ev)
        d = [e[1] for e in ev if e[0] == "d"]
        assert d[3][1][:2] == (0, 1) and 1 not in _ids(q[0]) and 1 not in q[0][1]     # dump 3 follows query 0
        assert _ids(q[1]) == [1] and d[4][2][:2] == (10, 4) and d[4][1][:2] == (10, 4)
        assert _ids(q[2]) == [1] and q[3][2] == [] and d[6][1][:2] == (12, 8)
    return Case("connected", s, proof=proof)


def case_min_common_words():
    s = Script(64)
    q = {w: 0.0625 for w in range(10)}
    kid, expect = 1, []
    for qid, M in enumerate((1, 4, 5, 6, 10), start=1):
        mc = int(F32(M) * F32(0.8))
        assert mc == {1: 0, 4: 3, 5: 4, 6: 4, 10: 8}[M]
        s.clear()
        group = []
        for nshare in (M, mc + 1, mc):
            if nshare == 0:
                continue              # a key frame sharing no word is never met
            b = {w: 0.0625 for w in range(nshare)}
            b[20 + kid] = 0.25        # and one word the query lacks
            assert len(shared(q, b)[0]) == nshare
            s.kf(kid, b); s.add(kid)
            group.append((kid, nshare))
            kid += 1
        s.kf(100 + qid, q)
        s.reloc(qid, q); s.loop(100 + qid)
        expect.append([k for k, n in group if n > mc])       # the key frame at exactly minCommonWords is left out

    def proof(ev):
        qs = queries(ev)
        for i, ids in enumerate(expect):
            assert _ids(qs[2 * i]) == ids and _ids(qs[2 * i + 1]) == ids, (i, qs[2 * i])
    return Case("min_common_words", s, proof=proof)


def case_min_score():
    s = Script(64)
    s.kf(1, {1: 0.5}); s.kf(2, {2: 0.25}); s.kf(3, {3: 0.5})
    for k in (20, 21):
        s.kf(k, {1: 0.5, 2: 0.5, 3: 0.5})
    s.add(1, 2, 3)
    above = np.nextafter(F32(0.25), F32(1))
    assert above > F32(0.25) and F32("%.9g" % above) == above
    s.loop(20, 0.25)        # equal to 2's score: kept
    s.loop(21, above)       # one float ulp above it: dropped, yet mLoopScore is written

    def proof(ev):
        q = queries(ev)
        d = [e[1] for e in ev if e[0] == "d"]
        assert q[0][2] == [(1, _bits(0.5)), (2, _bits(0.25)), (3, _bits(0.5))]
        assert _ids(q[1]) == [1, 3] and d[-1][2][:3] == (21, 1, _bits(0.25))
    return Case("min_score", s, proof=proof)


def case_neighbours():
    """Neighbour lists of 0, 9, 10, 11 and 13 entries (the reference takes ten), duplicates, the key frame itself, an
    erased key frame with a stale score of the same query id, and a key frame never added.  Key frame i scores s_i
    against a query whose every value is 1 (the term of a common word is -2 * min)."""
    s = Script(64)
    score = {i: 0.03125 for i in range(1, 15)}
    score[14] = 0.5
    score[15] = 0.25
    for i, v in score.items():
        s.kf(i, {i: v})
    cov = {1: [], 2: list(range(3, 12)), 3: list(range(4, 14)), 4: list(range(5, 14)) + [1, 14],
           5: list(range(6, 14)) + [1, 2, 3, 4, 14], 6: [14, 1], 7: [7, 7, 8, 8], 8: [99], 9: [15]}
    assert [len(cov[k]) for k in (1, 2, 3, 4, 5)] == [0, 9, 10, 11, 13]
    assert cov[4].index(14) == 10 and cov[5].index(14) == 12           # cut off by GetBestCovisibilityKeyFrames(10)
    for k, v in cov.items():
        s.covis(k, v)
    main = {i: 1.0 for i in range(1, 15)}
    s.add(*range(1, 16))
    s.reloc(7, {15: 1.0})           # 15 gets mnRelocQuery 7 and mRelocScore 0.25 ...
    s.erase(15)                     # ... and leaves
    s.reloc(7, main)                # 9's neighbour 15 still counts
    s.add(15)
    s.kf(30, {15: 1.0})
    s.loop(30)
    s.erase(15)
    s.kf(30, main)                  # 30 is outside the database
    s.loop(30)

    def proof(ev):
        q = queries(ev)
        for big in (q[1], q[3]):
            assert _ids(big) == list(range(1, 15)) and 15 not in _ids(big)
            # 6 names 14 (0.5) within its first ten: acc 0.5625, best 14; 14 itself: 0.5.  9 + stale 15: 0.28125.
            # 4 and 5 would reach 0.5 + 9 * 0.03125 with 14; without it they stay below 0.75 * 0.5625
            assert big[1] == [14]
        assert q[0][2] == [(15, _bits(0.25))] and q[2][2] == [(15, _bits(0.25))]
    return Case("neighbours", s, proof=proof)


def case_stale_neighbour_wins():
    """The stale score of an erased key frame is the best of its group: the candidate is a key frame outside the database."""
    s = Script(64)
    s.kf(1, {1: 0.125}); s.kf(15, {15: 0.75}); s.covis(1, [15])
    s.add(1, 15)
    s.reloc(7, {15: 1.0}); s.erase(15); s.reloc(7, {1: 1.0})
    s.add(15); s.kf(30, {15: 1.0}); s.loop(30); s.erase(15); s.kf(30, {1: 1.0}); s.loop(30)

    def proof(ev):
        q = queries(ev)
        assert q[1][1:3] == ([15], [(1, _bits(0.125))]) and q[3][1:3] == ([15], [(1, _bits(0.125))])
    return Case("stale_neighbour_wins", s, proof=proof)


def case_retention():
    s = Script(64)
    sc = {1: 0.5, 2: 0.25, 3: 0.375, 4: 0.5, 11: 0.25, 12: 0.5, 13: 0.5, 21: 0.25, 22: 0.5, 23: 0.5}
    for i, v in sc.items():
        s.kf(i, {i: v})
    s.covis(1, [4]); s.covis(2, [4]); s.covis(3, [1])
    # accumulated: 1 -> 1.0 (best 1: 0.5 is not > 0.5), 2 -> 0.75 (best 4), 3 -> 0.875 (best 1), 4 -> 0.5
    acc = {1: sc[1] + sc[4], 2: sc[2] + sc[4], 3: sc[3] + sc[1], 4: sc[4]}
    assert acc[2] == 0.75 * max(acc.values()) and acc[3] > 0.75 * max(acc.values())    # exact: dyadic
    s.covis(11, [13, 12]); s.covis(21, [22, 23])
    s.add(1, 2, 3, 4)
    s.reloc(1, {i: 1.0 for i in (1, 2, 3, 4)})          # [1]: 2 is exactly at 0.75 * best (strict: dropped), 3 names 1 again
    s.kf(40, {i: 1.0 for i in (1, 2, 3, 4)}); s.loop(40)
    s.clear(); s.add(11, 12, 13)
    s.reloc(2, {i: 1.0 for i in (11, 12, 13)})          # 12 and 13 tie at 0.5; 11's list names 13 first
    s.clear(); s.add(21, 22, 23)
    s.reloc(3, {i: 1.0 for i in (21, 22, 23)})          # the other order
    s.kf(41, {i: 1.0 for i in (21, 22, 23)}); s.loop(41, 0.5)

    def proof(ev):
        q = queries(ev)
        assert q[0][1] == [1] and q[1][1] == [1] and _ids(q[0]) == [1, 2, 3, 4]
        assert q[2][2][1][1] == q[2][2][2][1] and q[2][1] == [13] and q[3][1] == [22]
        assert _ids(q[4]) == [22, 23] and q[4][1] == [22, 23]     # 21 is below minScore 0.5; nothing exceeds it: 0.5 > 0.375
    return Case("retention", s, proof=proof)


def case_float_steps():
    """accScore += and 0.75f * bestAccScore are float operations (src/KeyFrameDatabase.cc:161, :176, :276, :290).  Two
    plants where doing either in double keeps a key frame that the reference drops.  Key frame i scores its own value
    against a query value of 2 (the term of a common word is -2 * min), all values are exact in float."""
    s = Script(64)
    e = 2.0 ** -25
    # A = 0.75 with two neighbours of 2^-25: each float add is half an ulp of 0.75 and rounds back (to even); B = 1.0
    f_acc = F32(F32(F32(0.75) + F32(e)) + F32(e))
    assert f_acc == F32(0.75) and 0.75 + e + e > 0.75 and not f_acc > F32(0.75) * F32(1.0)
    for k, v in ((1, 0.75), (2, 1.0), (3, e), (4, e)):
        s.kf(k, {k: v})
    s.covis(1, [3, 4])
    s.add(1, 2, 3, 4)
    q = {k: 2.0 for k in (1, 2, 3, 4)}
    s.reloc(1, q); s.kf(50, q); s.loop(50)
    # best = 1 + 2^-23: 0.75f * best needs 1.5 ulps of 0.75 and rounds up to 0.75 + 2^-23; a key frame at exactly that
    # value is not above it, though it is above the double product
    u = 2.0 ** -23
    assert F32(0.75) * F32(1.0 + u) == F32(0.75 + u) and 0.75 + u > 0.75 * (1.0 + u)
    s.clear()
    s.kf(11, {11: 0.75 + u}); s.kf(12, {12: 1.0 + u})
    s.add(11, 12)
    q = {11: 2.0, 12: 2.0}
    s.reloc(2, q); s.kf(51, q); s.loop(51)

    def proof(ev):
        qs = queries(ev)
        assert qs[0][2][:2] == [(1, _bits(0.75)), (2, _bits(1.0))] and qs[0][1] == [2] and qs[1][1] == [2]
        assert qs[2][2] == [(11, _bits(0.75 + u)), (12, _bits(1.0 + u))] and qs[2][1] == [12] and qs[3][1] == [12]
    return Case("float_steps", s, proof=proof)


def case_zero_and_empty():
    s = Script(64)
    s.kf(1, {1: 0.0, 2: 0.5}); s.kf(2, {3: 0.5}); s.kf(50, {1: 0.5, 4: 0.5}); s.kf(51, {}); s.kf(3, {})
    s.reloc(1, {1: 0.5}); s.loop(50)                    # an empty database
    s.add(1, 2, 3)
    s.reloc(2, {1: 0.5, 4: 0.5})                        # the only common word has value 0 in the key frame: si is 0
    s.loop(50)
    s.reloc(3, {}); s.loop(51)                          # empty queries
    s.reloc(4, {2: 0.5, 3: 0.5})
    s.clear()
    s.reloc(5, {2: 0.5, 3: 0.5})                        # emptied by clear
    s.add(2)
    s.reloc(4, {3: 0.5})                                # refilled: 2 keeps mnRelocQuery == 4, nothing pushed
    s.reloc(6, {3: 0.5})

    def proof(ev):
        q = queries(ev)
        assert [x[1:3] for x in q[:2]] == [([], []), ([], [])]
        for z in (q[2], q[3]):
            assert _ids(z) == [1] and z[2][0][1] & 0x7FFFFFFF == 0 and z[1] == []
        assert [x[1:3] for x in q[4:6]] == [([], []), ([], [])]
        assert q[6][1] == [1, 2] and q[7][1:3] == ([], []) and q[8][1:3] == ([], []) and q[9][1] == [2]
    return Case("zero_and_empty", s, proof=proof)


def case_encounter_order():
    s = Script(64)
    s.kf(1, {3: 0.5, 9: 0.25}); s.kf(2, {3: 0.25, 7: 0.5})
    s.kf(60, {3: 0.5})
    s.add(1, 2); s.reloc(1, {3: 0.5}); s.loop(60)
    s.clear(); s.add(2, 1); s.reloc(2, {3: 0.5})
    s.erase(2); s.add(2); s.reloc(3, {3: 0.5})
    s.erase(1); s.erase(2); s.add(2); s.add(1); s.reloc(4, {2: 0.5, 3: 0.5})

    def proof(ev):
        assert [_ids(q) for q in queries(ev)] == [[1, 2], [1, 2], [2, 1], [1, 2], [2, 1]]
    return Case("encounter_order", s, proof=proof)


def case_compaction_order():
    """A tiny handle (4 slots): the fifth add finds the table full, the erased slots go and the live ones move; the add
    order must survive it."""
    handle = dict(max_keyframes=4, max_entries=16)
    s = Script(64)
    for k in range(1, 12):
        s.kf(k, {3: 0.5 / k, 10 + k: 0.25})
    s.add(1, 2, 3, 4); s.erase(1); s.erase(3)
    s.reloc(1, {3: 0.5})
    s.add(3)                            # the table is full: compaction
    s.add(1)
    s.reloc(2, {3: 0.5})
    s.add(5, 6); s.erase(2); s.erase(5); s.add(7)
    s.reloc(3, {3: 0.5})
    s.add(2, 8, 5, 9, 10); s.erase(4); s.erase(9); s.add(11)
    s.reloc(4, {3: 0.5})
    tr = slot_trace(s.ops, **handle)
    assert [t[2] for t in tr] == [0, 1, 2, 3], tr        # a compaction between every two queries, from the script

    def proof(ev):
        assert [_ids(q) for q in queries(ev)] == [[2, 4], [2, 4, 3, 1], [4, 3, 1, 6, 7], [3, 1, 6, 7, 2, 8, 5, 10, 11]]
    return Case("compaction_order", s, handle=handle, proof=proof, facts=dict(compactions=[t[2] for t in tr]))


VALS = (0.125, 0.25, 0.5, 1.0)


def _small_bow(rng, nw):
    n = int(rng.integers(0, 9))
    ids = np.sort(rng.choice(nw, n, replace=False)).astype(np.int32)
    return ids, np.array([VALS[i] for i in rng.integers(0, 4, n)], np.float64)


def case_random(seed, nops=300, dyadic=True, handle=None, nkf=35, dump_every=1):
    """A seeded sequence in the style of run_sequence (tests/test_kfdb_gpu.py), a dump after every dump_every operations.
    With dyadic values ties and thresholds are frequent; without, the values are L1-normalised and summation order matters."""
    rng = np.random.default_rng(seed)
    nw = 40
    s = Script(nw, auto_dump=dump_every == 1)

    def rb():
        b = _small_bow(rng, nw)
        return b if dyadic or not len(b[0]) else (b[0], l1_values(rng, len(b[0])))
    present = set()
    for k in range(1, nkf + 1):
        s.kf(k, rb())
        s.covis(k, rng.integers(1, nkf + 2, int(rng.integers(0, 14))))
        s.conn(k, rng.choice(np.arange(1, nkf + 1), int(rng.integers(0, 5)), replace=False))
    for i in range(nops):
        if dump_every > 1 and i and i % dump_every == 0:
            s.dump()
        op = rng.random()
        if op < 0.3:
            k = int(rng.integers(1, nkf - 4))
            if k not in present:
                s.add(k); present.add(k)
        elif op < 0.45:
            k = int(rng.integers(1, nkf + 1))
            s.erase(k); present.discard(k)
        elif op < 0.47:
            s.clear(); present = set()
        elif op < 0.75:
            s.reloc(int(rng.integers(0, 7)), rb())
        else:
            s.loop(int(rng.integers(1, nkf + 1)), F32(rng.choice([0.0, 0.125, 0.25, 0.5])) if dyadic else F32(rng.choice([0.0, 0.05, 0.2])))
    if dump_every > 1:
        s.dump()
    return Case("random_%d" % seed, s, handle=handle)


def control_cases():
    return [case_query_ids(), case_connected(), case_min_common_words(), case_min_score(),
            case_neighbours(), case_stale_neighbour_wins(), case_retention(), case_float_steps(), case_zero_and_empty(), case_encounter_order(),
            case_compaction_order(), case_random(11), case_random(12, dyadic=False),
            case_random(13, handle=dict(max_keyframes=4, max_entries=16))]


# ---- kernel edges: each the smallest shape at which k_kfdb_score can still go wrong

CHUNK_LENGTHS = (0, 1, 63, 64, 65, 128, 129)


def _planted_kf(rng, n, planted):
    """n ascending words: entry j is 4j + 1 (odd: in no query), or 4j where planted (the queries hold only even words)."""
    ids = np.array([4 * j if j in planted else 4 * j + 1 for j in range(n)], np.int32)
    return ids, l1_values(rng, n)


def case_chunks(lengths=CHUNK_LENGTHS, only=None):
    """Key frames of 0, 1, 63, 64, 65, 128 and 129 words whose shared words sit in planted 64-entry chunks and lanes.
    Within a group every key frame shares the same number of words, so all are scored and appear in lScoreAndMatch.
    lengths / only cut the case down to some lengths and groups (the stored fixture)."""
    rng = np.random.default_rng(21)
    s = Script(1024, auto_dump=False)
    groups = {
        "lane0_lane63": lambda n: {0, 63} if n >= 64 else None,
        "first_chunk": lambda n: {min(n, 64) // 2} if n >= 1 else None,
        "second_chunk": lambda n: {64 + (min(n, 128) - 64) // 2} if n >= 65 else None,
        "last_entry": lambda n: {n - 1} if n >= 1 else None,
        "dense": lambda n: set(range(0, n, 2)) if n == 129 else None,
    }
    kid, qid, facts, expect = 1, 1, {}, []
    for gname, plant in groups.items():
        if only and gname not in only:
            continue
        s.clear()
        members, words = [], set()
        for n in tuple(lengths) + ((129, 129) if gname == "dense" else ()):
            p = plant(n)
            b = _planted_kf(rng, n, p or set())
            s.kf(kid, b); s.add(kid)
            if p:
                members.append((kid, b, p))
                words |= {4 * j for j in p}
            kid += 1
        filler = {4 * j + 2 for j in range(0, 140, 3)}          # in no key frame: query positions differ from entries
        qw = np.array(sorted(words | filler), np.int32)
        q = (qw, l1_values(rng, len(qw)))
        for k, b, p in members:
            pos, _ = shared(q, b)
            assert set(pos.tolist()) == p                        # numpy: exactly the planted entries are shared
            if gname == "second_chunk":
                assert all(64 <= x < 128 for x in pos)           # the first chunk's ballot is 0
            if gname == "last_entry":
                assert pos.tolist() == [len(b[0]) - 1]
            if gname == "lane0_lane63":
                assert pos.tolist() == [0, 63]
        assert len({len(p) for _, _, p in members}) == 1         # equal counts: int(c * 0.8f) < c, all are scored
        facts[gname] = [(len(b[0]), sorted(p)) for _, b, p in members]
        s.reloc(qid, q)
        s.kf(900 + qid, q); s.loop(900 + qid)
        expect.append(sorted(k for k, _, _ in members))
        qid += 1
    s.dump()
    if lengths == CHUNK_LENGTHS and not only:
        assert [n for n, _ in facts["second_chunk"]] == [65, 128, 129] and [n for n, _ in facts["last_entry"]] == [1, 63, 64, 65, 128, 129]

    def proof(ev):
        qs = queries(ev)
        for i, ids in enumerate(expect):
            assert ids and sorted(_ids(qs[2 * i])) == ids and sorted(_ids(qs[2 * i + 1])) == ids
    return Case("chunks", s, proof=proof, facts=facts)


def case_prefilter():
    """Key-frame words equal to the query's smallest and largest word and just outside both (the qmin / qmax test)."""
    rng = np.random.default_rng(22)
    s = Script(512, auto_dump=False)
    q = (np.array([100, 200, 300], np.int32), l1_values(rng, 3))
    kfs = {1: [100], 2: [300], 3: [99], 4: [301], 5: [99, 100], 6: [300, 301], 7: [99, 301], 8: [0, 99, 200, 301, 511], 9: [0, 511]}
    for k, w in kfs.items():
        s.kf(k, (np.array(w, np.int32), l1_values(rng, len(w)))); s.add(k)
    expect = [k for k, w in kfs.items() if len(shared(q, (w, np.ones(len(w))))[0])]
    assert expect == [1, 2, 5, 6, 8] and all(len(shared(q, (w, np.ones(len(w))))[0]) <= 1 for w in kfs.values())
    s.reloc(1, q); s.kf(90, q); s.loop(90)
    s.reloc(2, (q[0][:1], np.array([1.0]))); s.reloc(3, (q[0][2:], np.array([1.0])))    # qmin == qmax
    s.dump()

    def proof(ev):
        qs = queries(ev)
        assert sorted(_ids(qs[0])) == expect and sorted(_ids(qs[1])) == expect
        assert sorted(_ids(qs[2])) == [1, 5] and sorted(_ids(qs[3])) == [2, 6]
    return Case("prefilter", s, proof=proof)


def case_long_queries():
    """Queries of 1, 8192 and 8193 words (LDS and global-memory search) on 16384 words.  Every key frame shares 30 words
    with the 8192-word query and 30 or 31 with the 8193-word one, so all are scored."""
    rng = np.random.default_rng(23)
    nw = 16384
    s = Script(nw, auto_dump=False)
    perm = rng.permutation(nw)
    q8192 = np.sort(perm[:LDS_QUERY]).astype(np.int32)
    x, outside = int(perm[LDS_QUERY]), perm[LDS_QUERY + 1:]
    q8193 = np.sort(np.append(q8192, x)).astype(np.int32)
    w0 = int(q8192[0])
    nkf = 36
    for k in range(1, nkf + 1):
        words = set(rng.choice(q8192[1:], 30 - (k % 3 == 0), replace=False).tolist()) | set(rng.choice(outside, 10, replace=False).tolist())
        if k % 3 == 0:
            words.add(w0)
        if k % 2 == 0:
            words.add(x)
        ids = np.array(sorted(words), np.int32)
        b = (ids, l1_values(rng, len(ids)))
        assert len(shared((q8192, None), b)[0]) == 30 and len(shared((q8193, None), b)[0]) == 30 + (k % 2 == 0)
        s.kf(k, b); s.add(k)
    lens = []
    for qid, qw in enumerate(([w0], q8192, q8193), start=1):
        q = (np.asarray(qw, np.int32), l1_values(rng, len(qw)))
        lens.append(len(q[0]))
        s.reloc(qid, q); s.kf(900 + qid, q); s.loop(900 + qid)
    assert lens == [1, LDS_QUERY, LDS_QUERY + 1] and nw >= LDS_QUERY + 1
    s.dump()

    def proof(ev):
        qs = queries(ev)
        assert sorted(_ids(qs[0])) == list(range(3, nkf + 1, 3))
        for z in qs[2:]:
            assert sorted(_ids(z)) == list(range(1, nkf + 1))
    return Case("long_queries", s, proof=proof, facts=dict(query_lengths=lens))


SLOT_COUNTS = (8191, 8192, 8193, 16389)


def case_slots():
    """8191, 8192, 8193 and 16389 slots in the handle's table when the query runs, dead slots among the live ones.  Key
    frames have two or three words, at most one of them a query word, so every key frame that shares a word is scored
    (counts are all 1) and the reference's list names the key frames of the second and third trip of the wave stride."""
    rng = np.random.default_rng(24)
    nw = 4096
    handle = dict(max_keyframes=20000, max_entries=1 << 17)      # no compaction: the table only grows
    s = Script(nw, auto_dump=False)
    perm = rng.permutation(nw)
    qwords, other = np.sort(perm[:64]), perm[64:]
    added, erased, qid, last = 0, [], 1, {}
    for target in SLOT_COUNTS:
        while added < target:
            added += 1
            tail = added > target - 6                            # the last slots before each query share a word
            share = tail or rng.random() < 0.5
            words = set(rng.choice(other, int(rng.integers(2, 4)) - share, replace=False).tolist())
            if share:
                words.add(int(rng.choice(qwords)))
            ids = np.array(sorted(words), np.int32)
            assert 2 <= len(ids) <= 3 and len(np.intersect1d(ids, qwords)) <= 1
            s.kf(added, (ids, l1_values(rng, len(ids)))); s.add(added)
            if added % 97 == 0:                                  # a dead slot left behind, never one of the tail
                k = int(rng.integers(1, added - 8))
                if k not in erased:
                    s.erase(k); erased.append(k)
        q = (qwords.astype(np.int32), l1_values(rng, 64))
        s.reloc(qid, q); s.kf(100000 + qid, q); s.loop(100000 + qid)
        last[target] = ([k for k in range(target - 4, target + 1)], list(erased))
        qid += 1
    s.dump()
    tr = slot_trace(s.ops, **handle)
    assert [t[0] for t in tr] == [n for n in SLOT_COUNTS for _ in (0, 1)] and all(t[2] == 0 for t in tr)
    assert all(t[1] < t[0] for t in tr) and tr[-1][0] > 2 * WAVES and tr[2][0] == WAVES and tr[4][0] == WAVES + 1

    def proof(ev):
        qs = queries(ev)
        for i, target in enumerate(SLOT_COUNTS):
            for z in (qs[2 * i], qs[2 * i + 1]):
                got = set(_ids(z))
                assert set(last[target][0]) <= got and not (set(last[target][1]) & got)
                assert target < WAVES + 1 or max(got) > WAVES         # the list names slots of the second trip
    return Case("slots", s, handle=handle, proof=proof, facts=dict(slots=[t[0] for t in tr], live=[t[1] for t in tr]))


def case_second_download():
    """A query matching fewer than 10 key frames, then one matching more than 300 (more records than the first copy
    brings back), then the small one again."""
    rng = np.random.default_rng(25)
    s = Script(2048, auto_dump=False)
    A, B = 7, 1500
    bows = {}
    for k in range(1, 401):
        words = set(rng.choice(np.arange(100, 1400), 3, replace=False).tolist())
        if k % 60 == 1:
            words.add(A)
        if k > 70:
            words.add(B)
        ids = np.array(sorted(words), np.int32)
        bows[k] = (ids, l1_values(rng, len(ids)))
        s.kf(k, bows[k]); s.add(k)
    qa, qb = ({A: 1.0}, {B: 1.0})
    na = sum(len(shared(qa, b)[0]) > 0 for b in bows.values())
    nb = sum(len(shared(qb, b)[0]) > 0 for b in bows.values())
    nab = sum(len(shared(qa, b)[0]) > 0 and len(shared(qb, b)[0]) > 0 for b in bows.values())
    hint_after_a = na + na // 4
    assert na < 10 and nb > 300 and nb > max(hint_after_a, REC_GUESS)       # the second copy is needed
    s.reloc(1, qa); s.reloc(2, qb); s.reloc(3, qa)
    s.kf(901, qa); s.kf(902, qb)
    s.loop(901); s.loop(902); s.loop(901)
    s.dump()

    def proof(ev):
        qs = queries(ev)
        # the last: loop 902 retagged the key frames that hold B, so only those holding A and B are pushed again
        assert [len(z[2]) for z in qs] == [na, nb, na, na, nb, nab]
    return Case("second_download", s, proof=proof, facts=dict(records=[na, nb, na]))


def edge_cases():
    return [case_chunks(), case_prefilter(), case_long_queries(), case_slots(), case_second_download()]


# ---- the hand-worked expectations of tests/test_kfdb_cpu.py as scripts: (name, script, expected per query)
# expected per query: (candidates or None, lScoreAndMatch as [(score, id)] or None)

def hand_worked():
    out = []

    def start(kfs, nwords=100):
        s = Script(nwords, auto_dump=False)
        for kid, d in kfs:
            s.kf(kid, d); s.add(kid)
        return s
    q35 = {3: 0.5, 5: 0.5}
    s = start([(1, {5: 0.5}), (2, {3: 0.5}), (3, {3: 0.5, 5: 0.25})]); s.reloc(10, q35)
    out.append(("encounter_order_a", s, [(None, [(0.75, 3)])]))
    s = start([(1, {5: 0.5}), (2, {3: 0.5}), (3, {3: 0.25})]); s.reloc(10, q35)
    out.append(("encounter_order_b", s, [(None, [(0.5, 2), (0.25, 3), (0.5, 1)])]))
    s = start([(1, {5: 0.5}), (2, {3: 0.5}), (3, {3: 0.25})]); s.erase(2); s.add(2); s.reloc(10, q35); s.erase(77); s.reloc(11, q35)
    out.append(("erase_then_add", s, [(None, [(0.25, 3), (0.5, 2), (0.5, 1)])] * 2))
    q10 = {w: 0.0625 for w in range(10)}
    r = lambda n: {w: 0.0625 for w in range(n)}
    s = start([(1, r(6)), (2, r(5)), (3, r(4))]); s.reloc(1, q10)
    out.append(("min_common_6", s, [(None, [(0.375, 1), (0.3125, 2)])]))
    s = start([(1, r(5)), (2, r(4))]); s.reloc(1, q10)
    out.append(("min_common_5", s, [(None, [(0.3125, 1)])]))
    s = start([(1, {1: 0.5}), (2, {2: 0.25}), (3, {3: 0.5})]); s.kf(50, {1: 0.5, 2: 0.5, 3: 0.5}); s.loop(50, 0.5)
    out.append(("min_score_inclusive", s, [(None, [(0.5, 1), (0.5, 3)])]))
    s = start([(1, {1: 0.25}), (2, {2: 0.5}), (3, {3: 0.5})])
    s.covis(1, [3, 2]); s.covis(2, [3]); s.covis(3, [2]); s.reloc(9, {1: 0.5, 2: 0.5, 3: 0.5})
    out.append(("best_tie_and_duplicates", s, [([3, 2], [(0.25, 1), (0.5, 2), (0.5, 3)])]))
    s = start([(1, {2: 0.25, 3: 0.25}), (2, {1: 0.75}), (4, {4: 0.125, 5: 0.125})])
    s.reloc(10, {1: 0.75, 2: 0.25}); s.covis(1, [2]); s.reloc(11, {w: 0.5 for w in (1, 2, 3, 4, 5)})
    out.append(("stale_reloc_score", s, [([2], None), ([2], [(0.5, 1), (0.25, 4)])]))
    q12 = {1: 0.5, 2: 0.5}
    s = start([(1, {1: 0.5}), (2, {2: 0.5})]); s.reloc(0, q12); s.reloc(5, q12); s.reloc(0, q12)
    out.append(("query_id_zero", s, [([], []), ([1, 2], None), (None, [(0.5, 1), (0.5, 2)])]))
    s = start([(1, {1: 0.5})]); s.kf(0, {1: 0.5}); s.loop(0)
    out.append(("query_id_zero_loop", s, [([], [])]))
    s = start([(1, {1: 1.0}), (2, {2: 0.25, 3: 0.25})]); s.kf(7, {1: 1.0}); s.loop(7)
    s.kf(7, {1: 0.5, 2: 0.5, 3: 0.5}); s.covis(2, [1]); s.loop(7)
    out.append(("repeated_loop_id", s, [([1], None), ([1], [(0.5, 2)])]))
    s = start([(1, {1: 0.5})]); s.reloc(3, {1: 0.5}); s.reloc(3, {1: 0.5})
    out.append(("repeated_reloc_id", s, [([1], None), ([], None)]))
    s = start([(1, {1: 0.5, 2: 0.5, 3: 0.5}), (2, {1: 0.25, 2: 0.25})])
    s.kf(20, {1: 0.5, 2: 0.5, 3: 0.5}); s.conn(20, [1]); s.covis(2, [1]); s.loop(20)
    out.append(("connected_excluded", s, [([2], [(0.5, 2)])]))
    s = start([(1, {1: 0.5}), (2, {2: 0.5})]); s.reloc(4, q12); s.clear(); s.add(2); s.reloc(4, {2: 0.5}); s.reloc(6, {2: 0.5})
    out.append(("state_outlives_clear", s, [([1, 2], None), ([], None), ([2], None)]))
    s = start([(1, {}), (2, {1: 0.5})]); s.reloc(1, {}); s.reloc(2, {9: 0.5}); s.kf(3, {}); s.loop(3); s.reloc(4, {1: 0.5})
    out.append(("empty_bow_vectors", s, [([], None), ([], None), ([], None), ([2], None)]))
    for _, s, _ in out:
        s.dump()
    return out


# ---- comparison helpers shared by the two test files

def min_common_bounds(before, after, q, loop, qid):
    """What the reference's dumps around a query say about its minCommonWords: key frames pushed by it (their query id
    became qid) that are in lScoreAndMatch had more words, pushed ones outside it at most that many.  Only for queries
    whose list holds every scored key frame (relocalisation, or a loop query with minScore <= 0 and no negative score).
    Returns (lo, hi): lo <= minCommonWords < hi."""
    iq, iw = (0, 1) if loop else (3, 4)
    pushed = [k for k in after if after[k][iq] == qid and before.get(k, (0,) * 6)[iq] != qid]
    inl = set(_ids(q))
    lo = max([after[k][iw] for k in pushed if k not in inl], default=0)
    hi = min([after[k][iw] for k in pushed if k in inl], default=1 << 30)
    return lo, hi


def pinned_cases(build=False):
    """(control cases, edge cases, {name: reference events}), every proof checked; None where ref_kfdb is not built (and,
    with build, cannot be built).  Without build nothing of the reference tree is read."""
    if not ensure(allow_build=build):
        return None
    cc, ec = control_cases(), edge_cases()
    ref = {}
    for c in cc + ec:
        ref[c.name] = run_ref(c.ops)
        if c.proof:
            c.proof(ref[c.name])
    return cc, ec, ref
