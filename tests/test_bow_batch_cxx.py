"""The batched SearchByBoW overloads of my-slam_amd/host/ORBmatcher.h at their call sites: tests/cxx/bow_batch_callsites.cc writes
the candidate loops of Tracking::Relocalization (src/Tracking.cc:1377-1398) and LoopClosing::ComputeSim3 (src/LoopClosing.cc:253-281)
as the reference has them and as INTEGRATION.md section 3j rewrites them, on the classes of tests/cxx/slam_shims/, and compares per
candidate the tables (as pointers), the counts and the keep / discard decisions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "bow_batch_callsites.cc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "bow_batch_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "slam_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_call_sites_compile_with_the_batched_overloads(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for expr in ("matcher.SearchByBoW(pKF,mCurrentFrame,vvpMapPointMatchesA[i]);", "matcher.SearchByBoW(mpCurrentKF,pKF,vvpMapPointMatchesA[i]);",
                 "matcher.SearchByBoW(vpCandidateKFs,mCurrentFrame,vvpMapPointMatches,vnMatches);",
                 "matcher.SearchByBoW(mpCurrentKF,mvpEnoughConsistentCandidates,vvpMapPointMatches,vnMatches);",
                 "if(nmatches<15)", "if(nmatches<20)", "int nmatches = vnMatches[i];"):
        assert expr in text
    assert subprocess.run([exe, "compile-only"]).returncode == 0


@pytest.mark.gpu
def test_both_loops_give_the_same_tables_and_decisions(orbx, tmp_path):
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bow_batch_callsites ok" in r.stdout and "FAILED" not in r.stdout
    # five candidates: the bad one and the NULL one are not searched (-1), the sparse one is below both thresholds
    five = [l for l in r.stdout.splitlines() if l.startswith("five candidates")]
    assert len(five) == 2 and all(l.split("matches")[1].split()[1:3] == ["-1", "-1"] for l in five), r.stdout
    assert "five candidates: relocalization candidates 2 of 5" in r.stdout and "five candidates: loop candidates 2 of 5" in r.stdout, r.stdout
    assert "empty frame: relocalization candidates 0 of 5, matches 0 -1 -1 0 0" in r.stdout
    assert "no candidate: relocalization candidates 0 of 0" in r.stdout and "no candidate: loop candidates 0 of 0" in r.stdout
