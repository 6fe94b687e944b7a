"""Optimizer::BundleAdjustment / GlobalBundleAdjustemnt of my-slam_amd/host/PnPsolver.h at their call sites:
tests/cxx/ba_callsites.cc holds the lines src/Tracking.cc:695 and src/LoopClosing.cc:651 verbatim on the classes of
tests/cxx/ba_shims/ and compares the object graph after each with what the flat call orbp_bundle_adjustment dictates, for
nLoopKF == 0 and nLoopKF != 0.  The same program, built stand-alone over orbp_ba.cc, orbp_lba.cc and orbp.cc, runs the gather, the
host solver and the scatter under AddressSanitizer and UBSan on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "ba_callsites.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")
INC = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "ba_shims"), "-I" + os.path.join(ROOT, "include")]


def check(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ba_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "nLoopKF 0: 5 key frames, 59 points, 58 written" in r.stdout and "nLoopKF 7: 5 key frames, 59 points, 58 written" in r.stdout
    return r


def test_the_reference_lines_compile_verbatim_and_the_object_graph_is_what_the_flat_call_dictates(orbx, tmp_path):
    orbx.build()
    exe = str(tmp_path / "ba_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + INC +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    text = open(SRC).read()
    assert "Optimizer::GlobalBundleAdjustemnt(mpMap,20);" in text
    assert "Optimizer::GlobalBundleAdjustemnt(mpMap,10,&mbStopGBA,nLoopKF,false);" in text
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    check(exe)


def test_gather_host_solver_and_scatter_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "ba_callsites_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-DBA_CALLSITES_STANDALONE"] + INC +
                          [SRC, os.path.join(CSRC, "orbp_ba.cc"), os.path.join(CSRC, "orbp_lba.cc"), os.path.join(CSRC, "orbp.cc"), "-o", exe])
    r = check(exe)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
