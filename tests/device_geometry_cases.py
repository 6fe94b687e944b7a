"""The caller geometries of orbx_extract_batch_device that tests/test_device_geometry_gpu.py runs and
tests/test_device_geometry_cpu.py proves (no GPU here).

A geometry changes WHERE the pixels of a call lie in the caller's tensor, never what they are: a Layout is four byte counts
(pre, row_stride, frame_stride, tail) and a batch size.  The tensor holds `pre` bytes before frame 0, B frames `frame_stride`
apart with rows `row_stride` apart, and `tail` bytes behind the last pixel of the last frame; every byte that is not a pixel
holds a poison pattern.  So the oracle runs once per distinct frame (oracle(shape), cached, nobody may change it) and every
layout of a shape is checked against the same values.

Vacuity conditions, proved in the CPU test on the oracle's output alone (SEEDS were chosen so that they hold):
  * every pyramid level of every frame has keypoints;
  * a level-0 keypoint lies in the last cell column and one in the last cell row (the right-edge tile load of k_fast_cells);
  * a level-0 keypoint lies within 21 + 6 px of the right border (`fast` false in k_describe) and one at least that far from
    every border (`fast` true);
  * level 1's bottom-right pixel depends on level 0's last pixel (flipping it changes the oracle's level 1), and setting
    that pixel to zero changes it too -- a tail guard that drops the last dword of the buffer is then visible in level 1
    whatever the poison.

guard_keeps() emulates the tail guard of the 4x4 resize kernels on a layout's numbers, in its old and its new form; the
CPU test shows with it which layouts the old form gets wrong (the argument that the GPU test bites; nothing is reverted on
the GPU to watch it fail)."""
import collections
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NFEATURES = 500
POISONS = (0x00, 0xFF)
BATCHES = (1, 3, 17)

Shape = collections.namedtuple("Shape", "name W H scale nlevels seeds")
# 320 x 240 and 321 x 243 at 1.2 (RESIZE_FAST6: k_resize_linear_4x4s), 1.5 (k_resize_linear_4x4) and 2.0 (k_resize_area2) read level 0.
# k_resize_area2 runs only for an exact halving (even width and height: the planner follows cv::resize, which reroutes INTER_LINEAR
# to INTER_AREA only then).  At 2.0 the third level of these textures has no corner left, so that shape has two levels (every
# level must have keypoints).
SHAPES = collections.OrderedDict((s.name, s) for s in (
    Shape("320x240", 320, 240, 1.2, 8, (1, 2, 3)),
    Shape("321x243", 321, 243, 1.2, 8, (1, 2, 3)),
    Shape("321x243@1.5", 321, 243, 1.5, 4, (1, 2, 3)),
    Shape("320x240@2.0", 320, 240, 2.0, 2, (1, 2, 3)),
))
# part B: one frame whose height puts H * 2^22 just below 2^31 (511 * 2^22 = 2^31 - 2^22); the 320 x 240 frames serve everything else
TALL = Shape("320x511", 320, 511, 1.2, 8, (3,))

Layout = collections.namedtuple("Layout", "name pre rs fs tail B")


def frames(shape):
    import conftest  # noqa: F401  (makes my_slam_amd importable)
    import my_slam_amd.synth as synth
    return [synth.texture(s, shape.W, shape.H) for s in shape.seeds]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """[(keypoints, descriptors, per-level counts, pyramid levels)] for the distinct frames of a shape, from oracle_lib alone"""
    import oracle_lib as O
    shape = SHAPES.get(name, TALL)
    ex = O.Extractor(NFEATURES, shape.scale, shape.nlevels)
    out = []
    for img in frames(shape):
        k, d, npl, lv = ex.extract(img, want_levels=True)
        for a in (k, d) + tuple(lv):
            a.setflags(write=False)
        out.append((k, d, tuple(npl), tuple(lv)))
    return tuple(out)


def up(x, a):
    return (x + a - 1) // a * a


def layouts(shape):
    """The covering set for one shape: every line of the list at least once, the batch sizes dealt round-robin so that each of 1, 3
    and 17 meets aligned and unaligned layouts.  17 cycles the three frames; it is cut into sub-batches only on a handle whose
    ORBX_OPT_SUBBATCHES was raised (NSUBS below), which the GPU test does for every 17-frame layout."""
    W, H = shape.W, shape.H
    W4 = up(W, 4)
    L = []

    def add(name, pre, rs, fs, tail, B):
        L.append(Layout(name, pre, rs, fs, tail, B))

    # base offset 0..3 into the tensor, aligned strides, the last frame ends on the tensor's last byte (all four residues of the end)
    for pre, B in ((0, 3), (1, 1), (2, 17), (3, 3)):
        add("base+%d" % pre, pre, W4, W4 * H, 0, B)
    # row strides W .. W+3 and a padded one that is 4 mod 64; frames packed
    for pad, B in ((0, 17), (1, 3), (2, 1), (3, 3)):
        add("rs=W+%d" % pad, 0, W + pad, (W + pad) * H, 0, B)
    rsp = up(W, 64) + 64 + 4
    add("rs=64k+4", 0, rsp, rsp * H, 64, 3)
    # frame strides: frame 0 aligned, the later frames at every residue mod 4
    for extra, B in ((1, 3), (3, 3), (13, 17), (1, 17)):
        add("fs=rs*H+%d/B%d" % (extra, B), 0, W4, W4 * H + extra, 0, B)
    add("fs=padded", 0, W4, up(W4 * H, 256) + 256, 128, 3)
    # a region of a larger device image: odd x0, frames below each other with a gap of rows
    pitch = 2 * W4 + 36
    add("region", 5 * pitch + 37, pitch, (H + 3) * pitch, pitch * 2 + 11, 3)
    add("region/odd-pitch", 2 * (pitch + 1) + 3, pitch + 1, (H + 1) * (pitch + 1), 0, 1)
    # wholly aligned (what the suite had before), at the batch sizes the lines above leave without one
    add("aligned/B1", 0, W4, W4 * H, 0, 1)
    add("aligned/B17", 0, W4, up(W4 * H, 256), 32, 17)
    # everything odd at once, one frame and many
    add("odd/B1", 3, W + 3, (W + 3) * H + 1, 0, 1)
    add("odd/B17", 1, W + 1, (W + 1) * H + 2, 0, 17)
    return L


# The handle's switches.  As created a handle runs every call as ONE sub-batch with the resize chain on the call's stream ahead of
# FAST; ORBX_OPT_SUBBATCHES cuts calls of 16 frames and more, ORBX_OPT_OVERLAP_PYRAMID moves the chain of an uncut call to a side
# stream, set_profiling(2) drops events between the stages.  The GPU tests run all of them on caller memory:
NSUBS = (2, 3, 4)               # 17 frames: sub-batches start at frames (0, 8), (0, 5, 11), (0, 4, 8, 12)
B17_NAMES = ("base+2", "rs=W+0")                # the 17-frame layouts whose names do not say so
SWITCHED = ("fs=rs*H+3/B3", "odd/B1")           # unaligned layouts of fewer than 16 frames, for the overlap and profiling switches


def sub_batches(B, nsub):
    """[(first frame, frames)] as make_sub_batches (csrc/orbx_capi.hip) cuts a call: one piece below 16 frames"""
    if B < 16:
        nsub = 1
    return [(B * i // nsub, B * (i + 1) // nsub - B * i // nsub) for i in range(nsub)]


def numel(lay, shape):
    return lay.pre + (lay.B - 1) * lay.fs + (shape.H - 1) * lay.rs + shape.W + lay.tail


def frame_index(lay, f, nframes=3):
    return f % nframes


def pixel_mask(lay, shape):
    m = np.zeros(numel(lay, shape), bool)
    v = np.lib.stride_tricks.as_strided(m[lay.pre:], (lay.B, shape.H, shape.W), (lay.fs, lay.rs, 1), writeable=True)
    v[...] = True
    return m


def view(buf, lay, shape):
    """the (B, H, W) frames of a tensor laid out by `lay` (a strided view of buf)"""
    return np.lib.stride_tricks.as_strided(buf[lay.pre:], (lay.B, shape.H, shape.W), (lay.fs, lay.rs, 1), writeable=False)


def build(lay, shape, imgs, poison):
    """the caller's tensor as a host array: poison everywhere, then frame f % len(imgs) at pre + f * fs"""
    buf = np.full(numel(lay, shape), poison, np.uint8)
    v = np.lib.stride_tricks.as_strided(buf[lay.pre:], (lay.B, shape.H, shape.W), (lay.fs, lay.rs, 1), writeable=True)
    for f in range(lay.B):
        v[f] = imgs[frame_index(lay, f, len(imgs))]
    return buf


def l0_aligned(base, lay):
    """the kernels' own test (orbx_fast.hip, orbx_describe.hip): one shift for the whole level, or one per row"""
    return ((base | lay.rs | lay.fs) & 3) == 0


def frame_bases(base, lay):
    return [base + lay.pre + f * lay.fs for f in range(lay.B)]


# ---- the 4x4 resize kernels' reads of the last rows of the last frame, emulated on the numbers of a layout ----
def last_block_column(shape):
    """xofs of the first column of the last 4-column block of level 1's rows (cv::resize: floor((dx + 0.5) * W0 / W1 - 0.5))"""
    dw = oracle(shape.name)[0][3][1].shape[1]
    x4 = (dw - 1) // 4 * 4
    return max(int(math.floor((x4 + 0.5) * (shape.W / dw) - 0.5)), 0)


def guard_keeps(S, lay, shape, new):
    """For the last block of the last row of the frame at address S (the last frame of the call): does the guard keep every
    dword that holds a needed pixel?  S + off is the first needed byte, S + endoff the byte behind the frame's last pixel (src_end: the
    library computes it from the geometry, it knows nothing of a tail); the kernel reads three aligned dwords from (S + off) & ~3.
    old: dword k is read if it lies wholly before the end; new: if its first byte does."""
    off = (shape.H - 1) * lay.rs + last_block_column(shape)
    endoff = (shape.H - 1) * lay.rs + shape.W
    a = (S + off) & ~3                                       # absolute address of dword 0
    end = S + endoff
    last_needed = S + (shape.H - 1) * lay.rs + shape.W - 1
    for k in (1, 2):
        needed = a + 4 * k <= last_needed
        kept = (a + 4 * k < end) if new else (a + 4 * k + 4 <= end)
        if needed and not kept:
            return False
    return True


def first_dword_offset_wraps(S):
    """The old address arithmetic: offa = off - ((S + off) & 3) in uint32 for off == 0 (first block of row 0: xofs[0] == yofs[0] == 0)
    is 2^32 - (S & 3) for an unaligned frame base, i.e. a read near S + 4 GiB."""
    return ((0 - (S & 3)) & 0xFFFFFFFF) >= (1 << 31)


# ---- part B: places inside one allocation of FAR_BYTES ----
FAR_BYTES = (8 << 30) + (64 << 20)


def far_places(p0):
    """addresses inside [p0, p0 + FAR_BYTES): M = the first multiple of 2^32 at or above p0; M .. M + 2^32 lies inside whatever p0 is"""
    M = up(p0, 1 << 32)
    assert p0 <= M and M + (1 << 32) + (64 << 20) <= p0 + FAR_BYTES
    return M
