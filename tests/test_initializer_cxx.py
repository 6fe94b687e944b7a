"""my-slam_amd/host/Initializer.h at its call sites: tests/cxx/initializer_callsites.cc holds the Initializer lines of
Tracking::MonocularInitialization (src/Tracking.cc:589, :623) verbatim, on tests/cxx/slam_shims/ and orbx_cv_compat.h.
tests/cxx/init_asan_main.cc drives orbp_init_* stand-alone under AddressSanitizer and UBSan on the CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "initializer_callsites.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "initializer_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "slam_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_the_reference_lines_compile_verbatim_and_run_on_the_host(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for line in ("mpInitializer =  new Initializer(mCurrentFrame,1.0,200);",
                 "if(mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated))"):
        assert line in text, line
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    # without a GPU: every hypothesis on the host; the planted motion comes back on both routes, the rotation-only pair is refused
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "initializer_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_host_solver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "init_asan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cxx", "init_asan_main.cc"), os.path.join(CSRC, "orbp_init.cc"), os.path.join(CSRC, "orbp.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "init_asan_main ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
def test_gpu_and_host_runs_agree_call_by_call(orbx, tmp_path):
    """the two lines with both GPU calls against the same lines on the host: R21, t21, vP3D and vbTriangulated byte for byte, on the
    fundamental route, the homography route, the refused rotation and the refused 7 matches"""
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "initializer_callsites ok" in r.stdout and "FAILED" not in r.stdout
    assert r.stdout.count("GPU and host runs agree") == 5
