"""The wave reduction of k_search_area (best / second-best over 64 lanes and several rounds of 64 items) on planted ties.

One grid of 130 keypoints in one cell column, all inside one window: the wave walks them in rounds of 64 + 64 + 2, and the
position p of a candidate sits in lane p % 64 of round p // 64.  Eight queries, each with a few near descriptors planted at chosen
positions of the candidate order (the rest of the train set is far from every query):
  a   best tied between positions 3 and 40: two lanes of round 0                            -> the first, second == best
  b   best tied between positions 10 and 74: one lane, rounds 0 and 1                      -> the first, second == best
  c   best at position 70 (lane 6, round 1), the same distance again at 129 (lane 1, round 2): the second is the best of a lane
      that lost, and equals the best's distance plus 0
  d   exactly one candidate (the only keypoint of octave 5, level window [5, 5])             -> second == 256
  e   exactly one candidate (octave 6), which the mask F removes                             -> -1 / 256 / 256 under F
  f   best tied between positions 1, 20 and 50; F removes positions 0..3, so the positions shift and the winner is the first
      candidate that is left
  g   best at 90, second at 5: the second is the best of a lane that lost, found in an earlier round
  h   second at 30, best at 94: the same lane, the second first
Skip masks: none, F = positions 0..3 and e's only candidate, and everything (every query -1 / 256 / 256).
The expected values come from the oracle's windowed search; the CPU test checks that the oracle gives the planted answers.
(The CSR twin of these shapes, k_best2_csr, is covered by tests/dense_cases.py csr_case: kinds tie / second_first / best_first at
spots (0, 1), (0, 64), (63, 64), (1, 65) of lists of 65 to 200 candidates, and lists of 0, 1 and 2 candidates.)"""
import functools

import numpy as np
import pytest

import oracle_lib as O

BOUNDS = (0.0, 640.0, 0.0, 480.0)
N = 130
WINDOW = (103.0, 113.0, 30.0)
# query -> [(position, distance)], level window
PLAN = {"a": ([(3, 20), (40, 20)], -1), "b": ([(10, 20), (74, 20)], -1), "c": ([(70, 20), (129, 20)], -1), "d": ([(100, 30)], 5),
        "e": ([(110, 30)], 6), "f": ([(1, 20), (20, 20), (50, 20)], -1), "g": ([(90, 20), (5, 25)], -1), "h": ([(30, 25), (94, 20)], -1)}
NAMES = tuple(PLAN)
FAR = 80                                        # every distance that is not planted is above this


def _pack(bits):
    return np.packbits(bits, axis=1, bitorder="little")


@functools.lru_cache(maxsize=None)
def fixture():
    rng = np.random.default_rng(130)
    k = np.zeros(N, O.KP_DTYPE)
    k["x"] = 103.0
    k["y"] = (126.0 - 0.2 * np.arange(N)).astype(np.float32)     # cell rows 13 .. 10: the candidate order is not the index order
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    grid = O.FrameGrid(k, *BOUNDS)
    order = grid.features_in_area(*WINDOW)                      # order[p] = keypoint at position p
    assert sorted(order.tolist()) == list(range(N)) and not np.array_equal(order, np.arange(N))
    k["octave"][order[100]] = 5
    k["octave"][order[110]] = 6
    grid = O.FrameGrid(k, *BOUNDS)
    assert np.array_equal(grid.features_in_area(*WINDOW), order)
    qb = rng.integers(0, 2, (len(NAMES), 256), dtype=np.uint8)
    tb = rng.integers(0, 2, (N, 256), dtype=np.uint8)
    for qi, name in enumerate(NAMES):
        for p, d in PLAN[name][0]:
            tb[order[p]] = qb[qi]
            tb[order[p], rng.permutation(256)[:d]] ^= 1
    lv = np.array([PLAN[n][1] for n in NAMES], np.int32)
    nq = len(NAMES)
    masks = {"none": None, "F": np.zeros(N, np.uint8), "all": np.ones(N, np.uint8)}
    masks["F"][order[[0, 1, 2, 3, 110]]] = 1
    fx = dict(kps=k, grid=grid, order=order, q=_pack(qb), t=_pack(tb), x=np.full(nq, WINDOW[0], np.float32),
              y=np.full(nq, WINDOW[1], np.float32), r=np.full(nq, WINDOW[2], np.float32), mn=lv, mx=lv.copy(), masks=masks)
    fx["want"] = {name: grid.search_area_best2(fx["q"], fx["x"], fx["y"], fx["r"], lv, lv, fx["t"], sk) for name, sk in masks.items()}
    return fx


def test_oracle_gives_the_planted_answers():
    fx = fixture()
    o = fx["order"]
    row = lambda mask, name: tuple(int(a[NAMES.index(name)]) for a in fx["want"][mask])
    assert row("none", "a") == (o[3], 20, 20)
    assert row("none", "b") == (o[10], 20, 20)
    assert row("none", "c") == (o[70], 20, 20)
    assert row("none", "d") == (o[100], 30, 256)
    assert row("none", "e") == (o[110], 30, 256)
    assert row("none", "f") == (o[1], 20, 20)
    assert row("none", "g") == (o[90], 20, 25)
    assert row("none", "h") == (o[94], 20, 25)
    # F: positions 0 .. 3 are gone, every later candidate moves up by four
    bi, bd, sd = row("F", "a")
    assert (bi, bd) == (o[40], 20) and FAR < sd < 256
    assert row("F", "b") == (o[10], 20, 20)
    assert row("F", "e") == (-1, 256, 256)
    assert row("F", "f") == (o[20], 20, 20)
    for name in NAMES:
        assert row("all", name) == (-1, 256, 256)
    # nothing but the planted rows is near a query
    D = np.unpackbits(fx["q"][:, None, :] ^ fx["t"][None, :, :], axis=2).sum(2)
    for qi, name in enumerate(NAMES):
        planted = [o[p] for p, _ in PLAN[name][0]]
        assert np.delete(D[qi], planted).min() > FAR


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ["none", "F", "all"])
def test_search_area_planted_ties(orbx, mask):
    import torch
    fx = fixture()
    m = orbx.ORBmatcher(0.9, True, max_queries=64, max_train=256, max_pairs=4096)
    m.grid_build(fx["kps"], *BOUNDS)
    sk = fx["masks"][mask]
    want = fx["want"][mask]
    got = m.search_area_best2(fx["q"], fx["x"], fx["y"], fx["r"], fx["mn"], fx["mx"], fx["t"], sk)
    for g, w, what in zip(got, want, ("best_idx", "best_d", "second_d")):
        assert np.array_equal(g, w), (what, mask, dict(zip(NAMES, zip(g.tolist(), w.tolist()))))
    # the device-pointer form on resident arrays
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, dx, dy, dr, dmn, dmx, dt = [dev(fx[n]) for n in ("q", "x", "y", "r", "mn", "mx", "t")]
    dsk = dev(sk) if sk is not None else None
    out = torch.full((3, len(NAMES)), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    orbx._mchk(m.L.orbm_search_area_best2_device(m.h, dq.data_ptr(), dx.data_ptr(), dy.data_ptr(), dr.data_ptr(), dmn.data_ptr(),
                                                 dmx.data_ptr(), len(NAMES), dt.data_ptr(), dsk.data_ptr() if dsk is not None else None,
                                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st.cuda_stream))
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    for g, w, what in zip(res, want, ("best_idx", "best_d", "second_d")):
        assert np.array_equal(g, w), ("device form", what, mask, dict(zip(NAMES, zip(g.tolist(), w.tolist()))))
    m.close()
