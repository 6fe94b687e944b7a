"""my-slam_amd/host/PnPsolver.h at its call site: tests/cxx/pnp_callsites.cc holds the PnPsolver lines of Tracking::Relocalization
(src/Tracking.cc:1377-1418) on the classes of tests/cxx/slam_shims/ and orbx_cv_compat.h, plus the one added line
PnPsolver::EvaluateAll(vpPnPsolvers, matcher) in front of the RANSAC loop."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "pnp_callsites.cc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "pnp_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "slam_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_the_relocalization_lines_compile_and_run_on_the_host(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for line in ("PnPsolver* pSolver = NewPnPsolver(mCurrentFrame,cands[i].vpMapPointMatches);",
                 "pSolver->SetRansacParameters(0.99,10,300,cands[i].minSet,0.5,5.991);",
                 "PnPsolver* pSolver = vpPnPsolvers[i];",
                 "pSolver->iterate(5,bNoMore,vbInliers,nInliers);",
                 "PnPsolver::EvaluateAll(dev, matcher, 5, &err);",
                 "PnPsolver::EvaluateAll(raw, m);"):
        assert line in text, line
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    # without a GPU: every hypothesis on the host; the inlier flags land on the frame's feature indices of the right matches
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pnp_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_evaluate_all_then_iterate_equals_the_host_run(orbx, tmp_path):
    """constructor -> EvaluateAll -> iterate on the GPU: call by call the same poses, counts and flags as the all-host run, with a
    discarded candidate's NULL slot, a candidate no pose comes back for and one with 6-point samples; through the ORBmatcher and
    through a C handle"""
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pnp_callsites ok" in r.stdout and "FAILED" not in r.stdout
    assert r.stdout.count("EvaluateAll + replay") == 2
