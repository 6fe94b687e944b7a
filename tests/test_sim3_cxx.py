"""my-slam_amd/host/Sim3Solver.h at its call sites: tests/cxx/sim3_callsites.cc holds the Sim3Solver lines of LoopClosing::ComputeSim3
(src/LoopClosing.cc:275-276, :301-302, :321-323) verbatim, on the classes of tests/cxx/slam_shims/ and orbx_cv_compat.h, plus the one
added line Sim3Solver::EvaluateAll(vpSim3Solvers, matcher).  tests/cxx/sim3_asan_main.cc drives orbp_sim3_* stand-alone under
AddressSanitizer and UBSan on the CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "sim3_callsites.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "sim3_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "slam_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_the_reference_lines_compile_verbatim_and_run_on_the_host(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for line in ("Sim3Solver* pSolver = new Sim3Solver(mpCurrentKF,pKF,vvpMapPointMatches[i],mbFixScale);",
                 "pSolver->SetRansacParameters(0.99,20,300);",
                 "Sim3Solver* pSolver = vpSim3Solvers[i];",
                 "cv::Mat Scm  = pSolver->iterate(5,bNoMore,vbInliers,nInliers);",
                 "cv::Mat R = pSolver->GetEstimatedRotation();",
                 "cv::Mat t = pSolver->GetEstimatedTranslation();",
                 "const float s = pSolver->GetEstimatedScale();",
                 "Sim3Solver::EvaluateAll(dev, matcher, &err);"):
        assert line in text, line
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    # without a GPU: every hypothesis on the host; the inlier flags land on the vpMatched12 indices of the planted inliers
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sim3_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_host_solver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sim3_asan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cxx", "sim3_asan_main.cc"), os.path.join(CSRC, "orbp_sim3.cc"), os.path.join(CSRC, "orbp.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sim3_asan_main ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
def test_evaluate_all_then_iterate_equals_the_host_run(orbx, tmp_path):
    """constructor -> EvaluateAll -> iterate on the GPU: call by call the same poses, counts and flags as the all-host run, the flags
    on the vpMatched12 indices of the planted inliers although vpMatched12 holds NULL, bad and index-less entries"""
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "sim3_callsites ok" in r.stdout and "FAILED" not in r.stdout
    assert r.stdout.count("EvaluateAll + replay") == 2
