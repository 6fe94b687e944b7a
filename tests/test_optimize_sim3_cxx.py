"""Optimizer::OptimizeSim3 of my-slam_amd/host/PnPsolver.h at its call site: tests/cxx/optimize_sim3_callsites.cc holds the line
src/LoopClosing.cc:327 verbatim inside the loop :287-343, and that loop rewritten round by round with one
Optimizer::OptimizeSim3Batch call, on the classes of tests/cxx/slam_shims/.
tests/cxx/optimize_sim3_asan_main.cc drives orbp_optimize_sim3 stand-alone under AddressSanitizer and UBSan on the CPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "optimize_sim3_callsites.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "optimize_sim3_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "slam_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_the_reference_line_compiles_verbatim_and_runs_on_the_host(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for line in ("const int nInliers = Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale);",
                 "cv::Mat Scm  = pSolver->iterate(5,bNoMore,vbInliers,nInliers);",
                 "matcher.SearchBySim3(mpCurrentKF,pKF,vpMapPointMatches,s,R,t,7.5);",
                 "if(nInliers>=20)",
                 "Optimizer::OptimizeSim3Batch(matcher.Handle(), vProblems, &err);"):
        assert line in text, line
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    # without a GPU: the line :327 on the RANSAC inliers; candidate 0 is rejected by the optimisation, candidate 1 wins
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "optimize_sim3_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("candidate 1 after 2 optimisations") == 2


def test_the_host_solver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "optimize_sim3_asan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cxx", "optimize_sim3_asan_main.cc"), os.path.join(CSRC, "orbp_sim3opt.cc"),
                           os.path.join(CSRC, "orbp.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "optimize_sim3_asan_main ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
def test_both_loop_forms_agree(orbx, tmp_path):
    """:287-343 as written (OptimizeSim3 on the host, candidate by candidate) and round by round with one OptimizeSim3Batch: the
    same mpMatchedKF, the same mvpCurrentMatchedPoints, gScm within the bar of tests/golden/sim3opt/tolerance.json"""
    bar = json.load(open(os.path.join(ROOT, "tests", "golden", "sim3opt", "tolerance.json")))["bar"]
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe] + [repr(bar[k]) for k in ("quaternion", "translation", "scale")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "optimize_sim3_callsites ok" in r.stdout and "FAILED" not in r.stdout
    assert r.stdout.count("both loop forms, candidate 1") == 2
