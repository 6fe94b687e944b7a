"""tests/device_geometry_cases.py without a GPU: the oracle's output meets the vacuity conditions the GPU tests rest on, the case
builders put pixels and poison where they say, the covering set covers, and the emulated tail guard of the 4x4 resize kernels
shows which layouts its old form got wrong."""
import numpy as np
import pytest

import device_geometry_cases as G
import oracle_lib as O

ALL = list(G.SHAPES.values())
BASE = 0x7F0000000000       # a tensor base as the allocator hands them out: a multiple of 256 and more


def cell_origin_last(n):
    """first keypoint coordinate that only the last cell column (row) of a level of n pixels can produce (ORBextractor.cc:776-800)"""
    lo, hi = 16 - 3, n - 16 + 3
    cells = (hi - lo) // 30
    size = -(-(hi - lo) // cells)
    return lo + 3 + (cells - 1) * size


@pytest.mark.parametrize("shape", ALL + [G.TALL], ids=lambda s: s.name)
def test_vacuity_conditions_hold_on_the_oracle(shape):
    ex = O.Extractor(G.NFEATURES, shape.scale, shape.nlevels)
    W, H = shape.W, shape.H
    for img, (k, d, npl, lv) in zip(G.frames(shape), G.oracle(shape.name)):
        assert len(npl) == shape.nlevels and min(npl) > 0, npl
        assert len(k) == sum(npl) and d.shape == (len(k), 32)
        k0 = k[k["octave"] == 0]
        x, y = k0["x"], k0["y"]
        assert (x >= cell_origin_last(W)).any() and (y >= cell_origin_last(H)).any()
        assert (x + 27 >= W).any(), "no keypoint whose patch load would leave the row: k_describe's byte path is not reached"
        assert ((x >= 21) & (y >= 21) & (x + 27 < W) & (y + 21 < H)).any()
        assert np.array_equal(lv[0], img)
        flipped, zeroed = img.copy(), img.copy()
        flipped[-1, -1] ^= 0xFF
        zeroed[-1, -1] = 0
        assert ex.pyramid(flipped)[1][-1, -1] != lv[1][-1, -1], "level 1's last pixel does not see level 0's"
        assert ex.pyramid(zeroed)[1][-1, -1] != lv[1][-1, -1], "a dropped last pixel would go unnoticed"


@pytest.mark.parametrize("shape", ALL, ids=lambda s: s.name)
def test_builders_place_pixels_and_poison(shape):
    imgs = G.frames(shape)
    for lay in G.layouts(shape):
        assert lay.rs >= shape.W and lay.fs >= (shape.H - 1) * lay.rs + shape.W, lay      # frames do not overlap
        mask = G.pixel_mask(lay, shape)
        assert mask.sum() == lay.B * shape.W * shape.H
        assert not mask[:lay.pre].any() and mask[lay.pre] and mask[len(mask) - 1 - lay.tail] and not mask[len(mask) - lay.tail:].any()
        for poison in G.POISONS:
            buf = G.build(lay, shape, imgs, poison)
            assert len(buf) == G.numel(lay, shape)
            v = G.view(buf, lay, shape)
            for f in range(lay.B):
                assert np.array_equal(v[f], imgs[f % 3])
            assert (buf[~mask] == poison).all()
        if lay.tail == 0:                                   # the last frame ends on the tensor's last byte
            assert G.frame_bases(0, lay)[-1] + (shape.H - 1) * lay.rs + shape.W == G.numel(lay, shape)


@pytest.mark.parametrize("shape", ALL, ids=lambda s: s.name)
def test_the_set_covers(shape):
    """every line of the list, per shape: base residues, row strides, frame-base residues, a region, both parities of the end, the
    batch sizes, and both sides of l0_aligned"""
    W, H = shape.W, shape.H
    L = G.layouts(shape)
    names = [l.name for l in L]
    assert len(set(names)) == len(names) and set(G.SWITCHED) <= set(names)
    assert {l.name for l in L if l.B == 17} == {n for n in names if n.endswith("B17")} | set(G.B17_NAMES)
    for n in G.SWITCHED:                                    # the switch tests want unaligned layouts that are never cut
        l = next(l for l in L if l.name == n)
        assert l.B < 16 and not G.l0_aligned(BASE + l.pre, l)
    # sub-batches: 17 frames in 2, 3 and 4 pieces; with 3 the pieces start at frames 0, 5 and 11, so an odd frame stride puts their
    # level-0 bases at different residues mod 4 (2 and 4 pieces start at multiples of 4 frames: same residue, other addresses)
    assert [G.sub_batches(17, n) for n in G.NSUBS] == [[(0, 8), (8, 9)], [(0, 5), (5, 6), (11, 6)], [(0, 4), (4, 4), (8, 4), (12, 5)]]
    assert G.sub_batches(3, 4) == [(0, 3)]
    res3 = [{(BASE + l.pre + f0 * l.fs) & 3 for f0, _ in G.sub_batches(17, 3)} for l in L if l.B == 17]
    assert any(len(r) == 3 for r in res3) and any(r == {0} for r in res3), res3
    aligned_strides = [l for l in L if l.rs % 4 == 0 and l.fs % 4 == 0]
    assert {(BASE + l.pre) & 3 for l in aligned_strides} == {0, 1, 2, 3}
    assert {W, W + 1, W + 2, W + 3} <= {l.rs for l in L}
    assert any(l.rs % 64 == 4 and l.rs > W + 3 for l in L)
    fs_extra = {l.fs - l.rs * H for l in L}
    assert {0, 1, 13} <= fs_extra and any(e >= 256 for e in fs_extra)
    later = {b & 3 for l in L if (BASE + l.pre) % 4 == 0 and l.rs % 4 == 0 for b in G.frame_bases(BASE, l)[1:]}
    assert later == {0, 1, 2, 3}
    assert any(l.rs >= 2 * W and l.pre > l.rs and (l.pre % l.rs) % 2 == 1 for l in L), "no region of a larger image"
    ends = {(G.frame_bases(BASE, l)[-1] + (H - 1) * l.rs + W) & 3 for l in L if l.tail == 0}
    assert ends == {0, 1, 2, 3}
    assert {l.B for l in L} == set(G.BATCHES)
    for B in G.BATCHES:                                     # each batch size on both sides of the kernels' alignment test
        assert {G.l0_aligned(BASE + l.pre, l) for l in L if l.B == B} == {True, False}, B
    if W % 4 == 0:
        assert any(G.l0_aligned(BASE + l.pre, l) and l.rs == W and l.fs == W * H for l in L)   # the one geometry the suite had before


@pytest.mark.parametrize("shape", [s for s in ALL if s.scale < 2.0], ids=lambda s: s.name)
def test_old_guard_and_old_offset_fail_where_the_new_ones_hold(shape):
    """Why the GPU test bites, on numbers alone.  (1) The old 32-bit `off - shift` wraps for every frame whose base is not a multiple of
    4.  (2) The old tail guard `offa + 8 <= endoff` drops a dword that holds the last pixels of the last row for some layouts of the
    set; the new one `offa + 4 < endoff` keeps every needed dword for all of them; where base, strides and width are all multiples of
    4 (the only geometry the suite had) the two agree."""
    dropped = []
    for lay in G.layouts(shape):
        bases = G.frame_bases(BASE, lay)
        S = bases[-1]
        assert G.guard_keeps(S, lay, shape, new=True), lay
        if not G.guard_keeps(S, lay, shape, new=False):
            dropped.append(lay.name)
        if G.l0_aligned(BASE + lay.pre, lay):               # (a width that is no multiple of 4 ends the buffer off a dword all the same)
            assert not any(G.first_dword_offset_wraps(b) for b in bases)
            assert G.guard_keeps(S, lay, shape, new=False) or shape.W % 4
        else:
            assert any(G.first_dword_offset_wraps(b) for b in bases) or lay.rs % 4, lay
    assert dropped, "no layout of the set reaches a straddling last dword"
    print(shape.name, "old guard drops a needed dword in:", dropped)


def test_far_places_lie_inside_the_allocation():
    for p0 in (0x7F0000000000, 0x7F00FFFFFFFF, 0x7F0080000200, 0x7EFF00000001):
        M = G.far_places(p0)
        assert M % (1 << 32) == 0 and p0 <= M < p0 + (1 << 32)
        for lo in (0x80000001, 0xFFFFFFFF - 100):
            a = M + lo
            assert a & 0xFFFFFFFF == lo and p0 <= a and a + (64 << 20) <= p0 + G.FAR_BYTES
        assert (1 << 23) - 1 < (1 << 23) and 239 * ((1 << 23) - 1) + 320 < (1 << 31)       # accepted: an odd pitch below 8 MiB
        assert 511 * (1 << 22) < (1 << 31) == 512 * (1 << 22)                             # accepted / rejected frame size
