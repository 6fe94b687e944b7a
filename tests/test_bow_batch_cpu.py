"""No-GPU checks of the four SearchByBoW entry points (include/orbm.h): the batch and the one-candidate calls' argument checks and
host answers through ctypes with a NULL handle, and what the case module (tests/bow_batch_cases.py) plants, on the oracle's output
alone."""
import ctypes as C

import numpy as np
import pytest

import bow_batch_cases as B


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


@pytest.fixture(scope="module")
def suite():
    """name -> (case, oracle table, oracle counts), computed once"""
    return {name: (case,) + B.oracle(case) for name, case in B.suite().items()}


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def small(variant, seed=3):
    return B.make_case("small", variant, seed, 40, [10, 10, 10, 10], [{"n": 25}, {"n": 12, "valid": "mask"}, {"n": 18}])


class Call:
    """one call of either entry point on copies of a case's arrays, outputs pre-filled with 77"""

    def __init__(self, orbx, variant, case=None):
        self.orbx, self.variant = orbx, variant
        case = case or small(variant)
        copy = lambda s: [s.kps.copy(), s.desc.copy(), [a.copy() for a in s.fv], None if s.valid is None else s.valid.copy()]
        self.shared = copy(case.shared)
        self.cands = [copy(c) for c in case.cands]
        self.nkf = len(self.cands)
        self.table = np.full((self.nkf, len(case.shared)), 77, np.int32)
        self.counts = np.full(self.nkf, 77, np.int32)
        self.null, self.null_args = set(), set()

    def run(self, handle=None, nnratio=0.75, check_ori=1):
        L = self.orbx.lib()
        sh, keep1 = self.orbx.bow_sides([tuple(self.shared)])
        cs, keep2 = self.orbx.bow_sides([tuple(c) for c in self.cands])
        for who, field in self.null:                      # a NULL buffer where the count says there is one
            setattr(sh[0] if who < 0 else cs[who], field, None)
        for who, field, value in getattr(self, "counts_override", []):
            setattr(sh[0] if who < 0 else cs[who], field, value)
        shp, csp = C.cast(sh, C.c_void_p), C.cast(cs, C.c_void_p)
        table = None if "table" in self.null_args else p(self.table)
        counts = None if "counts" in self.null_args else p(self.counts)
        if "shared" in self.null_args:
            shp = None
        if "cands" in self.null_args:
            csp = None
        if self.variant == "frame":
            return L.orbm_search_by_bow_batch(handle, csp, self.nkf, shp, C.c_float(nnratio), check_ori, table, counts)
        return L.orbm_search_by_bow_kf_batch(handle, shp, csp, self.nkf, C.c_float(nnratio), check_ori, table, counts)

    def untouched(self):
        return (self.table == 77).all() and (self.counts == 77).all()


class SingleCall(Call):
    """orbm_search_by_bow / orbm_search_by_bow_kf on the shared side and candidate `c` of a case: the same arrays, mutations and 77
    fill as Call, with who = 0 for the one candidate"""

    def __init__(self, orbx, variant, case=None, c=0):
        super().__init__(orbx, variant, case)
        self.cands, self.nkf = [self.cands[c]], 1
        self.table = np.full(len(self.shared[1]), 77, np.int32)
        self.counts = np.full(1, 77, np.int32)

    def side(self, who, with_valid):
        kps, desc, fv, valid = self.shared if who < 0 else self.cands[who]
        a = dict(desc=p(desc), kps=p(kps), n=len(desc), valid=p(valid), fv_node=p(fv[0]), fv_off=p(fv[1]), fv_idx=p(fv[2]), fv_n=len(fv[0]))
        a.update({field: None for w, field in self.null if w == who})
        a.update({field: value for w, field, value in getattr(self, "counts_override", []) if w == who})
        return [a["desc"], a["kps"], a["n"]] + ([a["valid"]] if with_valid else []) + [a["fv_node"], a["fv_off"], a["fv_idx"], a["fv_n"]]

    def run(self, handle=None, nnratio=0.75, check_ori=1):
        L = self.orbx.lib()
        out = [C.c_float(nnratio), check_ori, None if "table" in self.null_args else p(self.table),
               None if "counts" in self.null_args else p(self.counts)]
        if self.variant == "frame":
            return L.orbm_search_by_bow(handle, *(self.side(0, True) + self.side(-1, False) + out))
        return L.orbm_search_by_bow_kf(handle, *(self.side(-1, True) + self.side(0, True) + out))


def test_the_symbols_and_their_wrappers_exist(built):
    """Fails on a library built without my-slam_amd/csrc/orbm_bow.hip."""
    L = C.CDLL(built.LIB_PATH)
    assert hasattr(L, "orbm_search_by_bow_batch") and hasattr(L, "orbm_search_by_bow_kf_batch")
    assert hasattr(built.ORBmatcher, "SearchByBoWBatch") and hasattr(built.ORBmatcher, "SearchByBoWKFBatch")
    assert C.sizeof(built.BowSide) == 64


def side_mutations(variant, who):
    """(mutation of a Call, text of the refusal) for every malformed side; who = -1: the shared side, else that candidate"""
    FV = 2
    side = lambda c: c.shared if who < 0 else c.cands[who]
    yield lambda c: side(c)[FV][1].__setitem__(0, 1), b"fv_off[0] must be 0"
    yield lambda c: side(c)[FV][1].__setitem__(2, int(side(c)[FV][1][1]) - 1), b"fv_off not monotone"
    yield lambda c: side(c)[FV][0].__setitem__(1, int(side(c)[FV][0][0])), b"node ids not ascending"
    yield lambda c: side(c)[FV][0].__setitem__(2, int(side(c)[FV][0][1]) - 1), b"node ids not ascending"
    yield lambda c: side(c)[FV][2].__setitem__(3, len(side(c)[1])), b"feature index"
    yield lambda c: side(c)[FV][2].__setitem__(len(side(c)[FV][2]) - 1, -1), b"feature index -1"
    for field in ("desc", "kps", "fv_node", "fv_off", "fv_idx") + (("valid",) if variant == "kf" else ()):
        yield lambda c, field=field: c.null.add((who, field)), b"NULL buffer"
    yield lambda c: setattr(c, "counts_override", [(who, "n", -1)]), b"negative count"
    yield lambda c: setattr(c, "counts_override", [(who, "fv_n", -3)]), b"negative count"


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_argument_checks_come_before_any_device_work(built, variant):
    """With a NULL handle every bad argument gets ORBX_E_INVALID and a text, and no output is written."""
    L = built.lib()

    def bad(mutate, text):
        c = Call(built, variant)
        mutate(c)
        assert c.run() == built.ORBX_E_INVALID and text in L.orbm_last_error(), L.orbm_last_error()
        assert c.untouched()

    for who in (-1, 0, 2):                                # the shared side, the first and the last candidate
        for mutate, text in side_mutations(variant, who):
            bad(mutate, text)
    for out in ("table", "counts", "shared", "cands"):
        bad(lambda c: c.null_args.add(out), b"NULL buffer")
    bad(lambda c: setattr(c, "nkf", -1), b"nkf=-1")


@pytest.mark.parametrize("cand", [0, 1])
@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_the_one_candidate_calls_check_as_the_batch_calls_do(built, variant, cand):
    """orbm_search_by_bow / orbm_search_by_bow_kf on one candidate of the same case, NULL handle: the same refusals with the same
    texts before anything is written."""
    L = built.lib()
    seen = 0
    for who in (-1, 0):
        for mutate, text in side_mutations(variant, who):
            c = SingleCall(built, variant, c=cand)
            mutate(c)
            assert c.run() == built.ORBX_E_INVALID and text in L.orbm_last_error(), (who, text, L.orbm_last_error())
            assert c.untouched(), (who, text)
            seen += 1
    assert seen == 2 * (14 if variant == "kf" else 13)
    for out in ("table", "counts"):
        c = SingleCall(built, variant, c=cand)
        c.null_args.add(out)
        assert c.run() == built.ORBX_E_INVALID and b"NULL buffer" in L.orbm_last_error()
        assert c.untouched()


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_a_one_candidate_call_without_a_shared_node_is_answered_on_the_host(built, variant):
    """ORBX_OK, a table of -1 and a count of 0 without a handle: an empty side (n == 0 or no node, either side), a candidate in
    nodes the shared side does not have, a candidate without a usable feature."""
    case = B.make_case("absent", variant, 5, 40, [10, 10, 10, 10], [{"n": 25, "absent": True}, {"n": 0}, {"n": 18, "valid": "zero"}])
    calls = [SingleCall(built, variant, case, c=k) for k in range(3)]
    for who in (-1, 0):
        for field in ("n", "fv_n"):
            c = SingleCall(built, variant)
            c.counts_override = [(who, field, 0)]
            if (who, field) == (-1, "n"):
                c.table = np.full(0, 77, np.int32)
            calls.append(c)
    for c in calls:
        assert c.run() == built.ORBX_OK, built.lib().orbm_last_error()
        assert (c.table == -1).all() and (c.counts == 0).all()


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_a_one_candidate_call_fails_loudly_without_a_handle(built, variant):
    """device work without a handle: the batch calls' status, and the outputs as they were"""
    import torch
    L = built.lib()
    c = SingleCall(built, variant)
    if torch.cuda.is_available():
        assert c.run() == built.ORBX_E_INVALID and b"NULL handle" in L.orbm_last_error()
    else:
        assert c.run() == built.ORBX_E_HIP and b"no CPU path" in L.orbm_last_error()
    assert c.untouched()


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_an_empty_batch_touches_nothing(built, variant):
    c = Call(built, variant)
    c.nkf = 0
    assert c.run() == built.ORBX_OK and c.untouched()
    L = built.lib()
    assert L.orbm_search_by_bow_batch(None, None, 0, None, C.c_float(0.7), 1, None, None) == built.ORBX_OK
    assert L.orbm_search_by_bow_kf_batch(None, None, None, 0, C.c_float(0.7), 1, None, None) == built.ORBX_OK


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_a_batch_without_a_shared_node_is_answered_on_the_host(built, variant):
    """No handle is needed: every candidate lives in nodes the shared side does not have, is empty, or has no usable feature."""
    case = B.make_case("absent", variant, 5, 40, [10, 10, 10, 10], [{"n": 25, "absent": True}, {"n": 0}, {"n": 18, "valid": "zero"}])
    c = Call(built, variant, case)
    assert c.run() == built.ORBX_OK
    assert (c.table == -1).all() and (c.counts == 0).all()
    # a candidate with n == 0 whose node lists are not empty is not refused for them: it has 0 matches, as in the one-candidate call
    c = Call(built, variant, case)
    c.counts_override = [(0, "n", 0)]
    assert c.run() == built.ORBX_OK, built.lib().orbm_last_error()
    assert (c.table == -1).all() and (c.counts == 0).all()
    # an empty shared side: n == 0, or no node
    for field in ("n", "fv_n"):
        c = Call(built, variant)
        c.counts_override = [(-1, field, 0)]
        if field == "n":                                  # its node lists are not looked at, as in the one-candidate calls
            c.table = np.full((c.nkf, 0), 77, np.int32)
        assert c.run() == built.ORBX_OK, built.lib().orbm_last_error()
        assert (c.table == -1).all() and (c.counts == 0).all()


@pytest.mark.parametrize("variant", ["frame", "kf"])
def test_the_entry_point_fails_loudly_without_a_handle(built, variant):
    """as orbm_create_new_map_points: ORBX_E_HIP where there is no device, ORBX_E_INVALID where there is one; no half answer"""
    import torch
    L = built.lib()
    c = Call(built, variant)
    if torch.cuda.is_available():
        assert c.run() == built.ORBX_E_INVALID and b"NULL handle" in L.orbm_last_error()
    else:
        assert c.run() == built.ORBX_E_HIP and b"no CPU path" in L.orbm_last_error()
    assert c.untouched()


# ---- the suite covers what it is about: on the oracle's output alone

def test_every_case_has_a_candidate_with_twenty_matches(suite):
    for name, (case, table, counts) in suite.items():
        assert counts.max() >= 20, name
        assert ((table >= 0).sum(axis=1) == counts).all(), name


def test_the_planted_contests_are_won_by_the_first_in_list_order(suite):
    planted = 0
    for name, (case, table, counts) in suite.items():
        for c, s1, s2, lane in case.contests:
            pairs = B.pairs_of(case, table[c])
            assert (s1, lane) in pairs, (name, c, s1, lane)
            assert sum(1 for _, l in pairs if l == lane) == 1 and not any(s == s2 for s, _ in pairs), (name, c, s2)
            planted += 1
    assert planted >= 20


def test_the_rotation_cull_removes_something(suite):
    removed = 0
    for name, (case, table, counts) in suite.items():
        _, unculled = B.oracle(case.with_params(case.nnratio, False))
        assert (unculled >= counts).all()
        removed += int((unculled - counts).sum() > 0)
    assert removed >= 1


def test_every_planted_tie_resolves_as_stated(suite):
    seen = 0
    for name, (case, _, _) in suite.items():
        if not case.ties:
            continue
        strict, _ = B.oracle(case.with_params(0.9, True))          # best == second best: the ratio test fails
        loose, _ = B.oracle(case.with_params(1.5, True))           # nnratio > 1: the first in the list is the best
        for c, s, l1, l2 in case.ties:
            assert not any(a == s or b in (l1, l2) for a, b in B.pairs_of(case, strict[c])), (name, "strict")
            got = B.pairs_of(case, loose[c])
            assert (s, l1) in got and not any(b == l2 for _, b in got), (name, "loose")
            seen += 1
    assert seen >= 4                                               # both kinds, both variants
