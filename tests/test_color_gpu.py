"""Colour input formats on the GPU: a handle set to BGR / RGB / BGRA / RGBA converts the frame itself (orbx_color.hip) and must then
give, byte for byte, what a grey handle gives for the numpy oracle's grey image (tests/gray_oracle.py) -- through every way a frame
enters the library.

Images: a synth.py scene as one channel, a rolled and an inverted copy as the other two (so the channels truly differ), one corner
overwritten with the eight corners of the colour cube, random alpha for the 4-channel formats.  Shapes: widths 320..323 x height 241
(all four values of width % 4: the last quad of a row is partial for three of them), each with a tight row stride and with a stride
of width * cn + 1, which rotates the alignment of the row bases through all four phases, so the wide-load path and the byte path
both run within one frame."""
import functools

import numpy as np
import pytest

import gray_oracle as G

pytestmark = pytest.mark.gpu

H = 241
NF = 500
FORMATS = [G.FMT_BGR8, G.FMT_RGB8, G.FMT_BGRA8, G.FMT_RGBA8]
CASES = [(f, w, p) for f in FORMATS for w in (320, 321, 322, 323) for p in (0, 1)]
IDS = ["%s-w%d-%s" % ({1: "bgr", 2: "rgb", 3: "bgra", 4: "rgba"}[f], w, "stride+1" if p else "tight") for f, w, p in CASES]


@functools.lru_cache(maxsize=None)
def _rgb_planes(W, k):
    """Frame k of the test sequence as three differing planes (H, W, 3), in memory order; the cube corners sit at the top left."""
    from my_slam_amd import synth
    base = synth.texture(40 + k, W, H)
    img = np.stack([base, np.roll(base, 37 + 5 * k, axis=1), 255 - base], -1)
    img[0, :8] = [[255 * ((i >> 2) & 1), 255 * ((i >> 1) & 1), 255 * (i & 1)] for i in range(8)]
    img.setflags(write=False)
    return img


def _colour(W, fmt, k):
    """(H, W, cn) contiguous colour frame k in format fmt."""
    img = _rgb_planes(W, k)
    if G.CHANNELS[fmt] == 4:
        alpha = np.random.default_rng(1000 + k).integers(0, 256, (H, W, 1), dtype=np.uint8)
        img = np.concatenate([img, alpha], -1)
    return np.ascontiguousarray(img)


def _strided(frames, pad, gap, alloc=None):
    """The frames [B, H, W, cn] laid out with row stride W * cn + pad and `gap` bytes between frames, in a buffer with no byte behind
    the last pixel.  Returns (view [B, H, W, cn], buffer)."""
    B, _, W, cn = frames.shape
    rs = W * cn + pad
    fs = rs * H + gap
    n = (B - 1) * fs + (H - 1) * rs + W * cn
    buf = alloc(n) if alloc else np.empty(n, np.uint8)
    buf[:] = 0xA5
    view = np.lib.stride_tricks.as_strided(buf, (B, H, W, cn), (fs, rs, cn, 1))
    view[...] = frames
    return view, buf


@functools.lru_cache(maxsize=None)
def _reference(orbx_mod, W, fmt):
    """Per frame k = 0..2: (grey oracle image, keypoints, descriptors of a grey handle fed that image).  Computed once per (width,
    channel order) and shared; the arrays are read-only."""
    ex = orbx_mod.ORBextractor(NF, max_width=W, max_height=H)
    out = []
    for k in range(3):
        grey = G.to_gray(_colour(W, fmt, k), fmt)
        kps, desc = ex(grey)
        assert len(kps) > 100
        for a in (grey, kps, desc):
            a.setflags(write=False)
        out.append((grey, kps, desc))
    ex.close()
    return out


def _same(got, want, what):
    assert len(got[0]) == len(want[1]), "%s: %d keypoints, want %d" % (what, len(got[0]), len(want[1]))
    assert got[0].tobytes() == want[1].tobytes(), what + ": keypoints differ"
    assert np.array_equal(got[1], want[2]), what + ": descriptors differ"


def _level0(ex, frame=0):
    w, h = ex.level_size(0)
    a = np.zeros((h, w), np.uint8)
    import my_slam_amd as M
    M._chk(ex.L.orbx_download_level(ex.h, frame, 0, a.ctypes.data, a.strides[0], 0))
    return a


def test_oracle_separates_channel_orders():
    for W in (320, 323):
        x = _colour(W, G.FMT_BGR8, 0)
        assert not np.array_equal(G.to_gray(x, G.FMT_BGR8), G.to_gray(x, G.FMT_RGB8))
        assert (G.to_gray(x, G.FMT_BGR8) != G.to_gray(x, G.FMT_RGB8)).mean() > 0.5


@pytest.mark.parametrize("fmt,W,pad", CASES, ids=IDS)
def test_single_frame_routes(orbx, fmt, W, pad):
    """orbx_extract; orbx_extract_begin / end up to the graph replay; grey and colour alternating on one handle; the argument checks."""
    ref = _reference(orbx, W, fmt)
    cn = G.CHANNELS[fmt]
    view, _buf = _strided(np.stack([_colour(W, fmt, k) for k in range(2)]), pad, 0)
    img = view[0]
    ex = orbx.ORBextractor(NF, max_width=W, max_height=H)
    assert ex.input_format == orbx.ORBX_FMT_GRAY8
    ex.set_input_format(fmt)
    assert ex.input_format == fmt
    # 1, 2: the blocking call; level 0 is the oracle's grey image
    _same(ex(img), ref[0], "orbx_extract")
    assert np.array_equal(_level0(ex), ref[0][0]), "level 0 differs from the oracle"
    # 3: begin / end three times (the third replays the captured graph), on another frame in between
    for rep in range(3):
        ex.extract_begin(img)
        _same(ex.extract_end(), ref[0], "begin/end call %d" % rep)
    ex.extract_begin(view[1])
    _same(ex.extract_end(), ref[1], "begin/end replay on frame 1")
    assert np.array_equal(_level0(ex), ref[1][0])
    # ... then grey, colour, grey, colour on the same handle
    for rep in range(2):
        ex.set_input_format(orbx.ORBX_FMT_GRAY8)
        ex.extract_begin(ref[1][0])
        _same(ex.extract_end(), ref[1], "grey after colour (%d)" % rep)
        ex.set_input_format(fmt)
        ex.set_input_format(fmt)               # the current value: nothing happens
        ex.extract_begin(img)
        _same(ex.extract_end(), ref[0], "colour after grey (%d)" % rep)
        assert np.array_equal(_level0(ex), ref[0][0])
    # 7: a stride below width * cn; a 2-D array on a colour handle; the setter while a call is in flight
    kps = np.zeros(ex.cap, orbx.KP_DTYPE); desc = np.zeros((ex.cap, 32), np.uint8)
    import ctypes as C
    n = C.c_int()
    tight = np.ascontiguousarray(img)
    for bad in (W * cn - 1, W):
        assert ex.L.orbx_extract(ex.h, tight.ctypes.data, W, H, bad, kps.ctypes.data, desc.ctypes.data, ex.cap, C.byref(n)) == orbx.ORBX_E_INVALID
        assert ex.L.orbx_extract_begin(ex.h, tight.ctypes.data, W, H, bad) == orbx.ORBX_E_INVALID
    with pytest.raises(orbx.OrbxError):
        ex(ref[0][0])
    with pytest.raises(orbx.OrbxError):
        ex(_colour(W, G.FMT_BGR8 if cn == 4 else G.FMT_BGRA8, 0))
    ex.extract_begin(img)
    assert ex.L.orbx_set_input_format(ex.h, orbx.ORBX_FMT_GRAY8) == orbx.ORBX_E_INVALID
    assert ex.input_format == fmt
    _same(ex.extract_end(), ref[0], "the call in flight while the setter was refused")
    assert ex.L.orbx_set_input_format(ex.h, 5) == orbx.ORBX_E_INVALID and ex.L.orbx_set_input_format(ex.h, -1) == orbx.ORBX_E_INVALID
    ex.set_input_format(orbx.ORBX_FMT_GRAY8)
    with pytest.raises(orbx.OrbxError):
        ex(tight)                              # a 3-D array on a grey handle
    _same(ex(ref[0][0]), ref[0], "grey at the end")
    ex.close()


@pytest.mark.parametrize("fmt,W,pad", CASES, ids=IDS)
def test_batch_routes(orbx, fmt, W, pad):
    """orbx_extract_batch from pageable and from page-locked memory, in one piece and in chunks; orbx_extract_batch_device;
    orbx_extract_batch_multi."""
    import torch
    ref = _reference(orbx, W, fmt)
    cn = G.CHANNELS[fmt]
    frames = np.stack([_colour(W, fmt, k) for k in range(3)])
    pageable, _b0 = _strided(frames, pad, 13)
    pinned, _b1 = _strided(frames, pad, 13, alloc=lambda n: torch.empty(n, dtype=torch.uint8).pin_memory().numpy())
    ex = orbx.ORBextractor(NF, max_width=W, max_height=H, max_batch=3)
    ex.set_input_format(fmt)

    def check(src, what):
        kps, desc, counts = ex.extract_batch_raw(src)
        for k in range(3):
            _same((kps[k, :counts[k]], desc[k, :counts[k]]), ref[k], "%s, frame %d" % (what, k))
            assert np.array_equal(_level0(ex, k), ref[k][0]), "%s: level 0 of frame %d" % (what, k)

    # 4: chunk 2 -- with 3 frames the library's rule (a batch of fewer than 2 * chunk frames goes in one piece) keeps the batch whole;
    # chunk 1 cuts the same 3 frames into 3 chunks: the first call of a shape plans it, the second captures the chunks' graphs, the
    # third replays them
    for chunk in (2, 1):
        ex.set_batch_chunk(chunk)
        for rep in range(3):
            check(pageable, "chunk %d, pageable, call %d" % (chunk, rep))
        for rep in range(2):
            check(pinned, "chunk %d, page-locked, call %d" % (chunk, rep))
    rs = W * cn + pad
    kps = np.zeros((3, ex.cap), orbx.KP_DTYPE); desc = np.zeros((3, ex.cap, 32), np.uint8); counts = np.zeros(3, np.int32)
    assert ex.L.orbx_extract_batch(ex.h, pageable.ctypes.data, 3, W, H, W * cn - 1, rs * H + 13, kps.ctypes.data, desc.ctypes.data, ex.cap,
                                   counts.ctypes.data) == orbx.ORBX_E_INVALID

    # 5: device-resident frames; level 0 is the handle's own grey plane, not the caller's buffer
    dview, dbuf = _strided(frames[:2], pad, 13)
    d_in = torch.from_numpy(dbuf).cuda()
    cap = ex.cap
    dk = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda"); dd = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    dc = torch.zeros(2, dtype=torch.int32, device="cuda"); ds = torch.full((2,), -99, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    ex.extract_batch_device(d_in.data_ptr(), 2, W, H, rs, rs * H + 13, dk.data_ptr(), dd.data_ptr(), dc.data_ptr(), ds.data_ptr(), st.cuda_stream)
    st.synchronize()
    d_in.zero_()
    torch.cuda.synchronize()
    assert ds.tolist() == [0, 0]
    for k in range(2):
        n = int(dc[k])
        got = (dk[k, :n].cpu().numpy().view(np.uint8).reshape(-1).view(orbx.KP_DTYPE), dd[k, :n].cpu().numpy())
        _same(got, ref[k], "orbx_extract_batch_device, frame %d" % k)
    assert np.array_equal(_level0(ex, 1), ref[1][0]), "level 0 of a colour handle must be the handle's grey plane"
    with pytest.raises(orbx.OrbxError) as ei:
        ex.extract_batch_device(d_in.data_ptr(), 2, W, H, W * cn - 1, rs * H + 13, dk.data_ptr(), dd.data_ptr(), dc.data_ptr(), ds.data_ptr(), st.cuda_stream)
    assert ei.value.code == orbx.ORBX_E_INVALID
    with pytest.raises(orbx.OrbxError) as ei:   # the kernel's indexing limit, on the colour stride
        ex.extract_batch_device(d_in.data_ptr(), 2, W, H, 1 << 23, 1 << 31, dk.data_ptr(), dd.data_ptr(), dc.data_ptr(), ds.data_ptr(), st.cuda_stream)
    assert ei.value.code == orbx.ORBX_E_SHAPE

    # 6: two handles on device 0
    ex2 = orbx.ORBextractor(NF, max_width=W, max_height=H, max_batch=3)
    ex2.set_input_format({G.FMT_BGR8: G.FMT_RGB8, G.FMT_RGB8: G.FMT_BGRA8, G.FMT_BGRA8: G.FMT_GRAY8, G.FMT_RGBA8: G.FMT_BGRA8}[fmt])
    with pytest.raises(orbx.OrbxError) as ei:
        orbx.extract_batch_multi([ex, ex2], frames)
    assert ei.value.code == orbx.ORBX_E_INVALID
    ex2.set_input_format(fmt)
    kps, desc, counts = orbx.extract_batch_multi([ex, ex2], frames)
    for k in range(3):
        _same((kps[k, :counts[k]], desc[k, :counts[k]]), ref[k], "orbx_extract_batch_multi, frame %d" % k)
    ex.close(); ex2.close()


def test_stereo_matches_on_colour_handles(orbx):
    """orbx_stereo_matches reads the pyramids of the two handles' last calls: two colour handles == two grey handles fed the converted
    images."""
    import stereo_cases as S
    W, Hs = 640, 480
    left, right, _ = S.stereo_scene(181, W, Hs)
    fmt = G.FMT_BGRA8
    rng = np.random.default_rng(3)

    def colour(g):
        return np.ascontiguousarray(np.stack([g, np.roll(g, 3, axis=1), 255 - g, rng.integers(0, 256, g.shape, dtype=np.uint8)], -1))

    cl, cr = colour(left), colour(right)
    gl, gr = G.to_gray(cl, fmt), G.to_gray(cr, fmt)
    mb, mbf = S.rig(500.0)
    res = []
    for f, a, b in [(orbx.ORBX_FMT_GRAY8, gl, gr), (fmt, cl, cr)]:
        exl = orbx.ORBextractor(NF, max_width=W, max_height=Hs); exr = orbx.ORBextractor(NF, max_width=W, max_height=Hs)
        exl.set_input_format(f); exr.set_input_format(f)
        kl, dl = exl(a)
        kr, dr = exr(b)
        u, d = orbx.ComputeStereoMatches(exl, exr, kl, dl, kr, dr, mb, mbf)
        res.append((kl, dl, kr, dr, u, d))
        exl.close(); exr.close()
    for x, y in zip(*res):
        assert x.tobytes() == y.tobytes()
    assert (res[0][4] >= 0).sum() > 0          # the comparison above was not between two empty results
