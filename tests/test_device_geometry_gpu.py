"""orbx_extract_batch_device on caller memory in the caller's own geometry: unaligned, padded, at the limits and far up the
address space.  Every other extraction test goes through the host entry points, which repack the frames into the handle's own
input block (64-byte pitch, 256-byte frame step, slack behind it), or hands over one geometry only (row_stride == W a multiple
of 4, frames packed, base aligned to 256 bytes).  Expected values are the oracle's (tests/device_geometry_cases.py: once per
distinct frame), keypoints and descriptors as bit patterns and every pyramid level of the first and the last frame of a call byte
for byte; tests/test_device_geometry_cpu.py proves the cases non-vacuous.

Which kernel branch a layout reaches (nothing outside the kernels can observe it, so it is stated here; base = address of frame 0):
  l0_aligned = ((base | row_stride | frame_stride) & 3) == 0, per sub-batch (orbx_fast.hip, orbx_describe.hip launch functions)
    true   "base+0", "rs=W+0" at W % 4 == 0 only, "rs=64k+4", "fs=padded", "aligned/*": k_fast_cells' 16-byte tile load for
           the inner cells and its `else` branch for the cells at the right edge of a caller-owned level 0 (the 52 bytes of the
           wide load would leave the row: the case file demands a level-0 keypoint in the last cell column); k_describe's
           12-byte tile load
    false  every other layout: k_fast_cells' `if (l == 0 && !l0_aligned)` (one shift per row), k_describe's
           `else` of `l != 0 || l0_aligned` (8-byte loads, one shift per row)
    either k_describe's byte path for keypoints within 21 + 6 px of the right border (`fast` false) -- demanded by the case file
  level 1 from the caller's level 0 (src_end is set for every caller-owned buffer, so the CHECK = true instances run):
    scale 1.2  k_resize_linear_4x4s<true> (RESIZE_FAST6, resize_block6<0, true>)
    scale 1.5  k_resize_linear_4x4<true>
    scale 2.0  k_resize_area2 (byte loads)
    The frame base is unaligned in "base+1..3", "fs=rs*H+k" (frames 1..), "region*", "odd*": the first block of row 0 reads the dword
    BELOW the base (the old 32-bit `off - shift` wrapped there by 4 GiB).  The last frame ends off a dword in every layout the CPU
    test lists as dropped by the old guard: the last block of the last row then needs a dword that straddles src_end.  With
    tail == 0 src_end is also the end of the tensor.
  How a call is cut and ordered is the handle's choice, not the batch size's (include/orbx.h: ORBX_OPT_SUBBATCHES defaults to 1,
  ORBX_OPT_OVERLAP_PYRAMID to 0), so each path is switched on explicitly:
    test_caller_geometry_equals_oracle            the handle as created: one sub-batch whatever B is, the resize chain on the call's
                                                  stream ahead of FAST (enqueue_pyramid), one level-0 base, one l0_aligned
    test_sub_batches_on_caller_geometry           every 17-frame layout with 2, 3 and 4 sub-batches (calls below 16 frames are never
                                                  cut): make_sub_batches' own level-0 base per sub-batch -- with 3 pieces (frames 0,
                                                  5, 11) at different residues mod 4 where the frame stride is odd --, l0_aligned
                                                  evaluated per sub-batch (it has the same value in all of them: the frame stride is
                                                  part of the test), and the last frame of each sub-batch but the last through the
                                                  guarded loads of the CHECK kernels with the rest of the call behind it (endoff
                                                  large; below 2^32 here, so rs_endoff's saturation is NOT reached by any test)
    test_caller_geometry_under_the_handle_switches  two unaligned layouts per shape with ORBX_OPT_OVERLAP_PYRAMID = 1 (the chain on a
                                                  side stream beside FAST: launch_levels(..., src_end, sa)), and under
                                                  set_profiling(2) (the default path with stage events between its launches)
  The pyramid is compared for the first and the last frame of every sub-batch.
  Poison 0x00 and 0xFF fill every byte that is no pixel: a byte read beyond the pixels that leaks into a result differs between the
  two, and a valid byte replaced by zero differs from the oracle under both.

Part B places frames and outputs inside one allocation of 8 GiB + 64 MiB (uninitialised; only the rows used are written), which
always holds a multiple M of 2^32 with 4 GiB behind it: row strides and frame sizes just inside the limits of include/orbx.h
(and just outside: ORBX_E_SHAPE, nothing launched), a frame stride beyond 32 bits, bases whose low word is 0x80000001 and
0xFFFFFFFF - 100, a batch with M + 2^32 inside its middle frame, and the outputs at bit-31 addresses and, one array per call, across
M + 2^32 (only one multiple is sure to have room on both sides; arrays shorter than 8 bytes cannot lie across it), guard bytes around.
Why a case of part A fails on the old kernels is argued on numbers in the CPU test (nothing was reverted on the GPU)."""
import numpy as np
import pytest

import device_geometry_cases as G

pytestmark = pytest.mark.gpu

CASES = [(s.name, lay.name) for s in G.SHAPES.values() for lay in G.layouts(s)]


class Rig:
    """one handle per shape for the whole module, and ordinary output tensors for max_batch frames"""

    def __init__(self, orbx, shape, max_batch=17, max_height=None):
        import torch
        self.shape = shape
        self.ex = orbx.ORBextractor(G.NFEATURES, shape.scale, shape.nlevels, 20, 7, max_width=shape.W, max_height=max_height or shape.H,
                                    max_batch=max_batch)
        cap = self.cap = self.ex.cap
        dev = torch.device("cuda")
        self.k = torch.zeros((max_batch, cap, 7), dtype=torch.float32, device=dev)
        self.d = torch.zeros((max_batch, cap, 32), dtype=torch.uint8, device=dev)
        self.c = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.s = torch.zeros(max_batch, dtype=torch.int32, device=dev)

    def call(self, base, B, rs, fs, outs=None):
        import torch
        k, d, c, s = outs or (self.k.data_ptr(), self.d.data_ptr(), self.c.data_ptr(), self.s.data_ptr())
        self.c.fill_(-1)
        self.s.fill_(-1)
        torch.cuda.synchronize()
        self.ex.extract_batch_device(base, B, self.shape.W, self.shape.H, rs, fs, k, d, c, s)
        torch.cuda.synchronize()

    def outputs(self, B):
        return self.k[:B].cpu().numpy(), self.d[:B].cpu().numpy(), self.c[:B].cpu().numpy(), self.s[:B].cpu().numpy()

    def check(self, outs, B, tag, frame_of=lambda f: f % 3, pyramid_frames=None):
        k, d, c, s = outs
        want = G.oracle(self.shape.name)
        assert (s == 0).all(), "%s: status %s" % (tag, s)
        for f in range(B):
            ok, od, _, _ = want[frame_of(f)]
            n = int(c[f])
            assert n == len(ok), "%s frame %d: %d keypoints, oracle %d" % (tag, f, n, len(ok))
            assert k[f, :n].tobytes() == ok.tobytes(), "%s frame %d: keypoints differ from the oracle" % (tag, f)
            assert np.array_equal(d[f, :n], od), "%s frame %d: descriptors differ in %d rows" % (tag, f, int((d[f, :n] != od).any(axis=1).sum()))
        for f in sorted(set(pyramid_frames if pyramid_frames is not None else (0, B - 1))):
            pyr = self.ex.image_pyramid(frame=f)
            olv = want[frame_of(f)][3]
            assert len(pyr) == len(olv)
            for l, (a, b) in enumerate(zip(pyr, olv)):
                assert a.shape == b.shape
                bad = np.argwhere(a != b)
                assert bad.size == 0, "%s frame %d level %d: %d bytes differ from the oracle, first at (y, x) = %s of %s" % (
                    tag, f, l, len(bad), tuple(bad[0]), a.shape)


@pytest.fixture(scope="module")
def rigs(orbx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(orbx, G.SHAPES[name])
        return made[name]

    yield get
    for r in made.values():
        r.ex.close()


# ---------------------------------------------------------------- A. caller geometry
def run_layout(rig, lay, tag, nsub=1):
    """nsub: what the handle's ORBX_OPT_SUBBATCHES is set to by the caller; the pyramid is compared for the first and the last frame of
    every sub-batch the call is then cut into (each last frame takes the guarded loads of the CHECK kernels)"""
    import torch
    shape = rig.shape
    imgs = G.frames(shape)
    pyramid_frames = sorted({f for f0, nf in G.sub_batches(lay.B, nsub) for f in (f0, f0 + nf - 1)})
    for poison in G.POISONS:
        host = G.build(lay, shape, imgs, poison)
        t = torch.from_numpy(host).cuda()
        assert t.data_ptr() % 256 == 0 and t.numel() == G.numel(lay, shape)
        rig.call(t.data_ptr() + lay.pre, lay.B, lay.rs, lay.fs)
        rig.check(rig.outputs(lay.B), lay.B, "%s poison %#04x" % (tag, poison), pyramid_frames=pyramid_frames)
        assert np.array_equal(t.cpu().numpy(), host), "%s: the input tensor was written to" % tag
        del t


@pytest.mark.parametrize("shape_name,layout_name", CASES)
def test_caller_geometry_equals_oracle(rigs, shape_name, layout_name):
    """the handle as it is created: one sub-batch, the resize chain on the call's stream ahead of FAST (enqueue_pyramid)"""
    rig = rigs(shape_name)
    lay = next(l for l in G.layouts(rig.shape) if l.name == layout_name)
    run_layout(rig, lay, "%s %s" % (shape_name, layout_name))


@pytest.mark.parametrize("nsub", G.NSUBS)
@pytest.mark.parametrize("shape_name,layout_name", [c for c in CASES if c[1].endswith("B17") or c[1] in G.B17_NAMES])
def test_sub_batches_on_caller_geometry(rigs, shape_name, layout_name, nsub):
    """ORBX_OPT_SUBBATCHES = 2, 3, 4 on the 17-frame layouts (the default is 1, and below 16 frames a call is never cut):
    make_sub_batches gives every sub-batch its own level-0 base, stream and launches; only the last one ends at src_end, the last
    frame of each of the others takes the guarded loads with the whole rest of the call behind it."""
    rig = rigs(shape_name)
    lay = next(l for l in G.layouts(rig.shape) if l.name == layout_name)
    assert lay.B == 17 and len(G.sub_batches(lay.B, nsub)) == nsub
    rig.ex.set_subbatches(nsub)
    try:
        run_layout(rig, lay, "%s %s nsub=%d" % (shape_name, layout_name, nsub), nsub)
    finally:
        rig.ex.set_subbatches(1)


@pytest.mark.parametrize("mode", ["overlap", "profiling2"])
@pytest.mark.parametrize("layout_name", G.SWITCHED)
@pytest.mark.parametrize("shape_name", list(G.SHAPES))
def test_caller_geometry_under_the_handle_switches(rigs, shape_name, layout_name, mode):
    """overlap: ORBX_OPT_OVERLAP_PYRAMID = 1 (default 0) -- with one sub-batch the whole resize chain runs on a side stream
    (launch_levels(..., src_end, sa)) beside FAST on level 0.  profiling2: set_profiling(2) -- the default path with stage events
    dropped into the stream between its launches."""
    rig = rigs(shape_name)
    lay = next(l for l in G.layouts(rig.shape) if l.name == layout_name)
    assert lay.B < 16 and not G.l0_aligned(0, lay)
    switch = rig.ex.set_overlap_pyramid if mode == "overlap" else (lambda on: rig.ex.set_profiling(2 if on else 0))
    switch(1)
    try:
        run_layout(rig, lay, "%s %s %s" % (shape_name, layout_name, mode))
    finally:
        switch(0)


# ---------------------------------------------------------------- B. limits and far buffers
class Far:
    """one uninitialised allocation; p0 its address, M the first multiple of 2^32 inside it"""

    def __init__(self, torch):
        self.torch = torch
        self.t = torch.empty(G.FAR_BYTES, dtype=torch.uint8, device="cuda")
        self.p0 = self.t.data_ptr()
        self.M = G.far_places(self.p0)

    def put_frames(self, addr, imgs, rs, fs):
        """frame f of imgs at addr + f * fs, rows rs apart: only the pixels are written"""
        H, W = imgs[0].shape
        assert self.p0 <= addr and addr + (len(imgs) - 1) * fs + (H - 1) * rs + W <= self.p0 + G.FAR_BYTES
        for f, img in enumerate(imgs):
            self.t.as_strided((H, W), (rs, 1), addr - self.p0 + f * fs).copy_(self.torch.from_numpy(np.ascontiguousarray(img)).cuda())

    def get_frames(self, addr, n, H, W, rs, fs):
        return [self.t.as_strided((H, W), (rs, 1), addr - self.p0 + f * fs).cpu().numpy() for f in range(n)]

    def carve(self, addr, nbytes, guard=64):
        """an output array of nbytes at addr with `guard` bytes of 0xA5 on either side"""
        o = addr - self.p0
        assert 0 <= o - guard and o + nbytes + guard <= G.FAR_BYTES
        self.t[o - guard:o + nbytes + guard].fill_(0xA5)
        return o

    def read(self, o, nbytes, dtype, guard=64):
        raw = self.t[o - guard:o + nbytes + guard].cpu().numpy()
        assert (raw[:guard] == 0xA5).all() and (raw[guard + nbytes:] == 0xA5).all(), "guard bytes around an output were overwritten"
        return raw[guard:guard + nbytes].view(dtype)


@pytest.fixture(scope="module")
def far():
    import torch
    try:
        f = Far(torch)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        pytest.skip("no room for the %.2f GiB allocation of the far-buffer tests" % (G.FAR_BYTES / 2.0 ** 30))
    try:
        yield f
    finally:
        f.t = None
        del f
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def rig3(orbx):
    r = Rig(orbx, G.SHAPES["320x240"], max_batch=3)
    yield r
    r.ex.close()


def far_case(far, rig, addr, B, rs, fs, tag):
    shape = rig.shape
    imgs = [G.frames(shape)[f % 3] for f in range(B)]
    far.put_frames(addr, imgs, rs, fs)
    rig.call(addr, B, rs, fs)
    rig.check(rig.outputs(B), B, tag)
    for got, img in zip(far.get_frames(addr, B, shape.H, shape.W, rs, fs), imgs):
        assert np.array_equal(got, img), "%s: the input was written to" % tag


def test_far_allocation_holds_what_the_cases_need(far):
    print("far allocation: %d bytes (%.3f GiB) at %#x, M = %#x" % (G.FAR_BYTES, G.FAR_BYTES / 2.0 ** 30, far.p0, far.M))
    assert far.t.numel() == G.FAR_BYTES and far.p0 <= far.M and far.M + (1 << 32) + (64 << 20) <= far.p0 + G.FAR_BYTES


def test_row_stride_just_below_8_mib(far, rig3):
    """row_stride = 2^23 - 1, H = 240: one frame of 1.88 GiB with an odd pitch, byte offsets up to 2 013 265 680 (31 bits, the 24-bit
    multiplies at their limit), from an odd base"""
    far_case(far, rig3, far.M + 1, 1, (1 << 23) - 1, 0, "rs=2^23-1")


def test_frame_size_limit_from_both_sides(far, orbx):
    """row_stride = 2^22 on a handle that admits 512 rows, so that only the frame-size limit can refuse: H = 512 makes H * row_stride
    == 2^31 exactly -> ORBX_E_SHAPE with the limit's own message and nothing launched; H = 511 (2^31 - 2^22, the largest frame of
    that pitch) is extracted and equals the oracle"""
    import torch
    rig = Rig(orbx, G.TALL, max_batch=1, max_height=512)
    try:
        rig.c.fill_(-1)
        rig.s.fill_(-1)
        with pytest.raises(orbx.OrbxError) as e:
            rig.ex.extract_batch_device(far.M + 2, 1, G.TALL.W, 512, 1 << 22, 0, rig.k.data_ptr(), rig.d.data_ptr(), rig.c.data_ptr(), rig.s.data_ptr())
        assert e.value.code == orbx.ORBX_E_SHAPE and "below 2 GiB" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (rig.c.cpu().numpy() == -1).all() and (rig.s.cpu().numpy() == -1).all()
        far_case(far, rig, far.M + 2, 1, 1 << 22, 0, "rs=2^22 H=511")
    finally:
        rig.ex.close()


def test_row_stride_limit_is_refused_without_a_launch(far, rig3, orbx):
    """row_stride = 2^23 (a frame of 240 rows stays below 2 GiB, the handle admits the shape: only the stride limit can refuse)"""
    shape = rig3.shape
    rig3.c.fill_(-1)
    rig3.s.fill_(-1)
    outs = (rig3.k.data_ptr(), rig3.d.data_ptr(), rig3.c.data_ptr(), rig3.s.data_ptr())
    with pytest.raises(orbx.OrbxError) as e:
        rig3.ex.extract_batch_device(far.M, 1, shape.W, shape.H, 1 << 23, 0, *outs)
    assert e.value.code == orbx.ORBX_E_SHAPE and "below 8 MiB" in str(e.value), str(e.value)
    import torch
    torch.cuda.synchronize()
    assert (rig3.c.cpu().numpy() == -1).all() and (rig3.s.cpu().numpy() == -1).all()
    far_case(far, rig3, far.M, 1, shape.W, 0, "after the refusal")             # the handle is as good as before


def test_frame_stride_beyond_32_bits(far, rig3):
    shape = rig3.shape
    far_case(far, rig3, far.p0 + 3, 2, shape.W + 1, (1 << 32) + 5, "fs=2^32+5")


@pytest.mark.parametrize("low", [0x80000001, 0xFFFFFFFF - 100], ids=["bit31", "ends-of-4GiB"])
def test_base_with_a_high_low_word(far, rig3, low):
    """d_images' low 32 bits with bit 31 set (a half that is sign-extended when the pointer is put together again shows here), and
    100 bytes below a multiple of 2^32 (every lane offset then carries into the high word)"""
    shape = rig3.shape
    addr = far.M + low
    assert addr & 0xFFFFFFFF == low
    far_case(far, rig3, addr, 3, shape.W, shape.W * shape.H, "low word %#x" % low)


def test_multiple_of_4_gib_inside_the_middle_frame(far, rig3):
    shape = rig3.shape
    rs, fs = shape.W + 3, (shape.W + 3) * shape.H + 2
    addr = far.M + (1 << 32) - fs - fs // 2
    X, span = far.M + (1 << 32), (shape.H - 1) * rs + shape.W
    assert addr + span < X and addr + fs < X < addr + fs + span and X < addr + 2 * fs      # frame 0 below, X inside frame 1, frame 2 above
    far_case(far, rig3, addr, 3, rs, fs, "4 GiB inside frame 1")


OUTPUTS = ("keypoints", "descriptors", "counts", "status")


@pytest.mark.parametrize("which", ("bit31",) + OUTPUTS)
def test_outputs_far_up(far, rig3, which):
    """d_keypoints, d_descriptors, d_counts and d_status at addresses with bit 31 of the low word set, and each of them in turn laid
    across a multiple of 2^32 (the allocation is sure to hold only one with room on both sides, so one array per call); the input
    at an odd place of the same allocation; the guard bytes around every output survive"""
    shape = rig3.shape
    B, cap = 3, rig3.cap
    sizes = [B * cap * 28, B * cap * 32, B * 4, B * 4]
    X = far.M + (1 << 32)
    if which == "bit31":
        addrs = [far.M + 0x80000000 + 1024 + i * (8 << 20) for i in range(4)]
        assert all(a & 0x80000000 for a in addrs)
    else:
        i = OUTPUTS.index(which)
        addrs = [X + (j + 1) * (8 << 20) for j in range(4)]
        addrs[i] = X - (sizes[i] // 2 // 32 * 32 if i < 2 else 4)               # natural alignment kept
        assert addrs[i] < X < addrs[i] + sizes[i]
    offs = [far.carve(a, n) for a, n in zip(addrs, sizes)]
    in_addr = far.p0 + (16 << 20) + 1
    far.put_frames(in_addr, G.frames(shape), shape.W, shape.W * shape.H)
    rig3.call(in_addr, B, shape.W, shape.W * shape.H, outs=addrs)
    k = far.read(offs[0], sizes[0], np.float32).reshape(B, cap, 7)
    d = far.read(offs[1], sizes[1], np.uint8).reshape(B, cap, 32)
    c = far.read(offs[2], sizes[2], np.int32)
    s = far.read(offs[3], sizes[3], np.int32)
    rig3.check((k, d, c, s), B, "outputs: " + which, pyramid_frames=())


# ---------------------------------------------------------------- C. the matcher's device-pointer calls at the same addresses
class FarArgs:
    """The arrays of one device-pointer call inside the far allocation, 64 guard bytes of 0xA5 around each: all of them at addresses
    whose low word has bit 31 set, or -- straddle = i -- array i laid across M + 2^32 and the others as before (the allocation is sure
    to hold one such multiple only, so the arrays take turns)."""
    GUARD = 64

    def __init__(self, far, ins, outs, straddle=None):
        self.far = far
        self.ins = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in ins]
        self.sizes = [len(a) for a in self.ins] + [n for n, _ in outs]
        self.nin = len(ins)
        X = far.M + (1 << 32)
        cursor = far.M + 0x80000000 + (1 << 20)
        self.addr = []
        for i, n in enumerate(self.sizes):
            if i == straddle:
                a = X - (G.up(n // 2, 16) if n >= 32 else 4)
                assert a < X < a + n
            else:
                a = cursor
                cursor += G.up(n + 2 * self.GUARD, 256)
                assert a & 0x80000000 and (a + n) & 0x80000000 and a + n < X - (1 << 30)
            self.addr.append(a)
        self.off = [far.carve(a, n, self.GUARD) for a, n in zip(self.addr, self.sizes)]
        for o, a in zip(self.off, self.ins):
            if len(a):
                far.t[o:o + len(a)].copy_(far.torch.from_numpy(a))
        for o, (n, fill) in zip(self.off[self.nin:], outs):
            far.t[o:o + n].fill_(fill)

    @staticmethod
    def turns(sizes):
        """None (every array at a bit-31 address), then every array that is long enough to lie across a boundary"""
        return [None] + [i for i, n in enumerate(sizes) if n >= 8]

    def tensor(self, i, dtype):
        """array i as a torch tensor over the allocation (for the call that takes tensors)"""
        return self.far.t[self.off[i]:self.off[i] + self.sizes[i]].view(dtype)

    def results(self, dtypes):
        """the outputs, guards checked; the inputs must be as they were uploaded"""
        self.far.torch.cuda.synchronize()
        for o, a in zip(self.off, self.ins):
            assert np.array_equal(self.far.read(o, len(a), np.uint8, self.GUARD), a), "an input array was written to"
        return [self.far.read(o, n, dt, self.GUARD) for o, n, dt in zip(self.off[self.nin:], self.sizes[self.nin:], dtypes)]


def far_turns(far, ins, outs):
    sizes = [np.ascontiguousarray(a).nbytes for a in ins] + [n for n, _ in outs]
    for s in FarArgs.turns(sizes):
        yield ("bit 31" if s is None else "array %d across 4 GiB" % s), FarArgs(far, ins, outs, s)


@pytest.fixture(scope="module")
def matcher(orbx):
    m = orbx.ORBmatcher(0.9, False, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield m
    m.close()


def test_far_best2_and_match_batch(far, matcher):
    """tests/test_dense_adversarial_gpu.py's smallest device batch (the acceptance table as one pair), its expected values"""
    import dense_cases as DC
    c = DC.batch_case("accept")
    bi, bd, sd = DC.batch_reference(c)
    nb, cap = len(c["nqs"]), c["cap"]
    kp = np.zeros((nb, cap, 7), np.float32)                   # every angle equal
    ins = [c["q"], c["nqs"], c["t"], c["nts"]]
    for what, A in far_turns(far, ins, [(nb * cap * 4, 0xEE)] * 3):
        a = A.addr
        matcher.best2_batch_device(a[0], a[1], a[2], a[3], cap, nb, a[4], a[5], a[6])
        got = [r.reshape(nb, cap) for r in A.results([np.int32] * 3)]
        for g, w, name in zip(got, (bi, bd, sd), ("best_idx", "best_d", "second_d")):
            assert np.array_equal(g, w), "best2_batch_device, %s: %s differs" % (what, name)
    th, nnratio = 50, 0.9
    want_m, want_n = np.full((nb, cap), -1, np.int32), np.zeros(nb, np.int32)
    for b in range(nb):
        nq = int(c["nqs"][b])
        want_m[b, :nq], want_n[b] = DC.ref_accept(bi[b, :nq], bd[b, :nq], sd[b, :nq], th, nnratio)
    assert want_n.sum() > 0 and (want_m[0, :int(c["nqs"][0])] < 0).any()
    for what, A in far_turns(far, ins + [kp], [(nb * cap * 4, 0xEE), (nb * 4, 0xEE)]):
        a = A.addr
        matcher.match_batch_device(a[0], a[4], a[1], a[2], a[4], a[3], cap, nb, a[5], a[6], th=th)
        m12, nm = A.results([np.int32, np.int32])
        assert np.array_equal(m12.reshape(nb, cap), want_m) and np.array_equal(nm, want_n), "match_batch_device, " + what


def test_far_search_area_best2(far, orbx):
    """tests/test_search_area_ties.py's planted ties with its mask F, expected values from the oracle's grid"""
    import test_search_area_ties as SA
    fx = SA.fixture()
    sk, want = fx["masks"]["F"], fx["want"]["F"]
    nq = len(SA.NAMES)
    m = orbx.ORBmatcher(0.9, True, max_queries=64, max_train=256, max_pairs=4096)
    try:
        m.grid_build(fx["kps"], *SA.BOUNDS)
        ins = [fx[n] for n in ("q", "x", "y", "r", "mn", "mx", "t")] + [sk]
        for what, A in far_turns(far, ins, [(nq * 4, 0xEE)] * 3):
            a = A.addr
            orbx._mchk(m.L.orbm_search_area_best2_device(m.h, a[0], a[1], a[2], a[3], a[4], a[5], nq, a[6], a[7], a[8], a[9], a[10], None))
            for g, w, name in zip(A.results([np.int32] * 3), want, ("best_idx", "best_d", "second_d")):
                assert np.array_equal(g, w), "search_area_best2_device, %s: %s differs" % (what, name)
    finally:
        m.close()


def test_far_distinctive_descriptors(far, matcher):
    """the run lengths at the edges of tests/test_mappoint_gpu.py's device case (without its 1500 ordinary points), the oracle's values"""
    import mappoint_oracle as MO
    rng = np.random.default_rng(61)
    lengths = np.array([0, 300, 1, 700, 2, 64, 65, 9, 3], np.int64)
    off, desc = MO.batch_from_lengths(rng, lengths)
    eb, em = MO.distinctive_descriptors(off, desc)
    n = len(lengths)
    for what, A in far_turns(far, [off, desc], [(n * 4, 0xEE)] * 2):
        a = A.addr
        matcher.distinctive_descriptors_device(n, a[0], a[1], int(off[-1]), int(lengths.max()), a[2], a[3])
        gb, gm = A.results([np.int32] * 2)
        assert np.array_equal(gb, eb) and np.array_equal(gm, em), "distinctive_descriptors_device, " + what


def test_far_triangulate_matches(far, orbx, matcher):
    """tests/test_triangulate_gpu.py's "mixed" scene, 200 matches; statuses equal, x3D as bit patterns of the restatement's"""
    import test_triangulate_gpu as TG
    import triangulation_oracle as T
    cam1, kf1, cam2, kf2, matches = TG.scene("mixed")
    matches = np.ascontiguousarray(matches[:200], np.int32)
    off2 = np.array([0, len(kf2)], np.int32)
    est, ex = T.triangulate(cam1, kf1, [cam2], off2, kf2, matches)
    n = len(matches)
    ok = est <= 2                                             # x3D is defined for the accepted matches
    assert ok.sum() > 20 and (~ok).sum() > 20
    ins = [np.asarray(cam1, orbx.CAM_DTYPE).reshape(1), kf1.kps_un, kf1.keys_xy, kf1.u_right, kf1.depth,
           np.asarray([cam2], orbx.CAM_DTYPE).reshape(1), off2, kf2.kps_un, kf2.keys_xy, kf2.u_right, kf2.depth, matches]
    for what, A in far_turns(far, ins, [(n, 0xEE), (n * 12, 0xEE)]):
        a = A.addr
        matcher.triangulate_matches_device(a[0], a[1], a[2], a[3], a[4], len(kf1), a[5], 1, a[6], a[7], a[8], a[9], a[10], a[11], n, a[12], a[13])
        st, x = A.results([np.uint8, np.float32])
        assert np.array_equal(st, est), "triangulate_matches_device, %s: statuses differ" % what
        assert np.array_equal(x.reshape(n, 3).view(np.uint32)[ok], ex.view(np.uint32)[ok]), "triangulate_matches_device, %s: x3D differs" % what


def test_far_frustum(far, matcher):
    """tests/test_frustum_gpu.py's device case (suite scene 0) against tests/frustum_oracle.py, at that module's bar"""
    import frustum_oracle as F
    import test_frustum_gpu as FG
    sc = F.suite_scene(0)
    n = len(sc)
    want = F.frustum(*sc.args(), 0.5)
    ins = [np.array([sc.view]), sc.skip, sc.xw, sc.normal, sc.mf_max, sc.mf_min]
    outs = [(n, 0xEE)] + [(4 * n, 0xEE)] * 5
    for what, A in far_turns(far, ins, outs):
        a = A.addr
        matcher.frustum_device(a[0], n, a[1], a[2], a[3], a[4], a[5], 0.5, a[6], a[7], a[8], a[9], a[10], a[11])
        got = A.results([np.uint8, np.float32, np.float32, np.float32, np.int32, np.float32])
        FG.same_frustum(tuple(got) + (want[6],), want, "frustum_device, " + what)


def test_far_pose_optimization_batch(far, orbx, matcher):
    """tests/test_pose_batch_gpu.py's device form on the six 65-edge problems of tests/pose_cases.py, against the host path at
    pose_cases.assert_same's bar"""
    import torch
    import pose_cases as pc
    name = "single_65"
    problems = pc.cases()[name]
    want = pc.host(orbx, name)
    off, obs, ur, s2, xw, cams, T = orbx.ORBmatcher.pack_pose_problems(problems)
    B, N = len(problems), int(off[-1])
    cams_f = np.ascontiguousarray(cams.view(np.float32).reshape(B, 5))
    ins = [off, obs, ur if ur is not None else np.full(N, -1, np.float32), s2, xw, cams_f]
    dts = [torch.int32] + [torch.float32] * 5
    for what, A in far_turns(far, ins, [(B * 64, 0xEE), (N, 0xEE), (B * 4, 0xEE)]):
        d_in = [A.tensor(i, dt) for i, dt in enumerate(dts)]
        d_T, d_out, d_good = A.tensor(6, torch.float32), A.tensor(7, torch.uint8), A.tensor(8, torch.int32)
        d_T.copy_(torch.from_numpy(T.reshape(-1)))             # Tcw is in/out
        assert d_T.data_ptr() == A.addr[6] and d_in[1].data_ptr() == A.addr[1]
        matcher.pose_optimization_batch_device(B, *d_in, d_T, d_out, d_good)
        Tg, og, gg = A.results([np.float32, np.uint8, np.int32])
        assert ((og == 0) | (og == 1)).all()
        for k, (w, pr) in enumerate(zip(want, problems)):
            got = (Tg.reshape(B, 16)[k].reshape(4, 4), og[off[k]:off[k + 1]].astype(bool), int(gg[k]))
            pc.assert_same(got, w, pr, "pose_optimization_batch_device, %s, problem %d" % (what, k))
