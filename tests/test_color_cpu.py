"""Colour input formats, the checks that need no GPU: the numpy statement of the grey arithmetic (tests/gray_oracle.py) against hand
values and against the integer formula over every 24-bit colour, and the argument checks of the new C-ABI entry points that are
reachable without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gray_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def _px(fmt, r, g, b, a=255):
    v = {G.FMT_BGR8: [b, g, r], G.FMT_RGB8: [r, g, b], G.FMT_BGRA8: [b, g, r, a], G.FMT_RGBA8: [r, g, b, a]}[fmt]
    return np.array(v, np.uint8).reshape(1, 1, -1)


@pytest.mark.parametrize("fmt", [G.FMT_BGR8, G.FMT_RGB8, G.FMT_BGRA8, G.FMT_RGBA8])
def test_hand_values(fmt):
    """(4899 * 255 + 8192) >> 14 = 76, (9617 * 255 + 8192) >> 14 = 150, (1868 * 255 + 8192) >> 14 = 29, (16384 * 255 + 8192) >> 14 = 255."""
    for (r, g, b), want in [((255, 0, 0), 76), ((0, 255, 0), 150), ((0, 0, 255), 29), ((255, 255, 255), 255), ((0, 0, 0), 0)]:
        assert int(G.to_gray(_px(fmt, r, g, b), fmt)[0, 0]) == want, (fmt, r, g, b)


def test_every_colour_equals_the_integer_formula():
    """All 2^24 colours, in both channel orders: 0 <= grey <= 255 before the cast to a byte, and the oracle returns that value."""
    assert G.R2Y + G.G2Y + G.B2Y == 1 << 14
    v = np.arange(1 << 24, dtype=np.int64)
    r, g, b = v >> 16, (v >> 8) & 255, v & 255
    want = (4899 * r + 9617 * g + 1868 * b + 8192) // 16384          # int64, no wrap-around, no cast
    assert want.min() == 0 and want.max() == 255
    rgb = np.stack([r, g, b], -1).astype(np.uint8).reshape(4096, 4096, 3)
    assert np.array_equal(G.to_gray(rgb, G.FMT_RGB8).ravel(), want)
    assert np.array_equal(G.to_gray(rgb[..., ::-1], G.FMT_BGR8).ravel(), want)


def test_alpha_has_no_influence():
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    for fmt3, fmt4 in [(G.FMT_BGR8, G.FMT_BGRA8), (G.FMT_RGB8, G.FMT_RGBA8)]:
        want = G.to_gray(rgb, fmt3)
        for alpha in (0, 255, None):
            a = rng.integers(0, 256, (64, 64, 1), dtype=np.uint8) if alpha is None else np.full((64, 64, 1), alpha, np.uint8)
            assert np.array_equal(G.to_gray(np.concatenate([rgb, a], -1), fmt4), want)
    assert np.array_equal(G.to_gray(rgb[..., 0], G.FMT_GRAY8), rgb[..., 0])


def test_channel_order_matters():
    x = _px(G.FMT_BGR8, 200, 100, 10)
    assert int(G.to_gray(x, G.FMT_BGR8)[0, 0]) != int(G.to_gray(x, G.FMT_RGB8)[0, 0])


def test_format_entry_points_exist_and_check_arguments(built):
    L = C.CDLL(built.LIB_PATH)
    for name in ("orbx_set_input_format", "orbx_get_input_format"):
        assert hasattr(L, name), name
    L.orbx_set_input_format.argtypes = [C.c_void_p, C.c_int]
    L.orbx_get_input_format.argtypes = [C.c_void_p]
    L.orbx_last_error.restype = C.c_char_p
    for fmt in (G.FMT_GRAY8, G.FMT_BGR8, G.FMT_RGBA8, 99):
        assert L.orbx_set_input_format(None, fmt) == built.ORBX_E_INVALID
        assert b"NULL handle" in L.orbx_last_error()
    assert L.orbx_get_input_format(None) == built.ORBX_E_INVALID


def test_python_constants_match_the_header(built):
    text = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name in ("GRAY8", "BGR8", "RGB8", "BGRA8", "RGBA8"):
        assert "ORBX_FMT_%s = %d" % (name, getattr(built, "ORBX_FMT_" + name)) in text
        assert getattr(built, "ORBX_FMT_" + name) == getattr(G, "FMT_" + name)


def test_batch_multi_refuses_null_handles_before_reading_formats(built):
    L = built.lib()
    hs = (C.c_void_p * 2)(None, None)
    counts = np.zeros(2, np.int32)
    assert L.orbx_extract_batch_multi(hs, 2, None, 2, 8, 8, 8, 64, None, None, 0, counts.ctypes.data_as(C.c_void_p)) == built.ORBX_E_INVALID


def test_compat_header_models_colour_mats(tmp_path):
    """orbx_cv_compat.h: CV_8UC3 / CV_8UC4 carry OpenCV's values, a colour Mat has cols * channels bytes per row, channels() reports
    the count -- and an element access still names its type, as with OpenCV."""
    src = tmp_path / "c.cc"
    src.write_text('#include "orbx_cv_compat.h"\n'
                   "static_assert(CV_8UC1 == 0 && CV_8UC3 == 16 && CV_8UC4 == 24 && CV_32FC1 == 5, \"OpenCV's type codes\");\n"
                   "int main() { cv::Mat a(5, 7, CV_8UC3), b(5, 7, CV_8UC4), c(5, 7, CV_8UC1), d = a.clone();\n"
                   "  return !(a.channels() == 3 && a.step == 21 && a.elemSize() == 3 && b.channels() == 4 && b.step == 28 && c.channels() == 1 && c.step == 7\n"
                   "           && d.step == 21 && d.type() == CV_8UC3 && a.isContinuous()); }\n")
    exe = str(tmp_path / "c")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "my-slam_amd", "host"), str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0
