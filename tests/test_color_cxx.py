"""ORBextractor::ExtractColor (my-slam_amd/host/ORBextractor.h) from a Tracking.cc-shaped caller (tests/cxx/color_callsites.cc):
CV_8UC3 / CV_8UC4 frames in either channel order give what operator() gives for the oracle's grey image, CV_8UC1 passes through,
operator() still refuses a colour image, and mvImagePyramid[0] is the grey image."""
import os
import subprocess

import numpy as np
import pytest

import gray_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
INC = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "include")]


def _build(orbx, out):
    if not os.path.exists(orbx.LIB_PATH):
        orbx.build()
    libdir = os.path.dirname(orbx.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + INC +
                          [os.path.join(CXX, "color_callsites.cc"), "-o", out, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    return out


def test_color_callsites_compile_and_link(orbx, tmp_path):
    exe = _build(orbx, str(tmp_path / "color_callsites"))
    assert subprocess.run([exe, "compile-only"]).returncode == 0


@pytest.mark.gpu
def test_extract_color_equals_operator_on_the_grey_image(orbx, synth, tmp_path):
    exe = _build(orbx, str(tmp_path / "color_callsites"))
    W, H = 323, 241
    base = synth.texture(7, W, H)
    c3 = np.ascontiguousarray(np.stack([base, np.roll(base, 29, axis=1), 255 - base], -1))
    c4 = np.concatenate([c3, np.random.default_rng(2).integers(0, 256, (H, W, 1), dtype=np.uint8)], -1)
    g_bgr, g_rgb = G.to_gray(c3, G.FMT_BGR8), G.to_gray(c3, G.FMT_RGB8)
    assert not np.array_equal(g_bgr, g_rgb)
    paths = []
    for name, a in [("c3", c3), ("c4", c4), ("g_bgr", g_bgr), ("g_rgb", g_rgb)]:
        paths.append(str(tmp_path / (name + ".u8")))
        np.ascontiguousarray(a).tofile(paths[-1])
    p = subprocess.run([exe] + paths + [str(W), str(H)], capture_output=True, text=True)
    rows = dict(ln.split() for ln in p.stdout.splitlines() if ln.strip())
    assert p.returncode == 0 and len(rows) == 10 and all(v == "1" for v in rows.values()), p.stdout + p.stderr
