"""The Fuse overload over a list of target key frames (my-slam_amd/host/ORBmatcher.h) at its call site:
tests/cxx/fuse_views_callsites.cc writes both halves of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:484-516) as the
reference has them and as INTEGRATION.md section 3k rewrites them, on the classes of tests/cxx/fuse_shims/ (whose Replace updates
the survivor's descriptor and whose KeyFrame has GetFeaturesInArea), and compares the two object graphs, the per-view counts and
the return values."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "fuse_views_callsites.cc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "fuse_views_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "fuse_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_call_sites_compile_and_do_nothing_without_a_device(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for expr in ("matcher.Fuse(pKFi,vpMapPointMatches)", "matcher.Fuse(mpCurrentKeyFrame,vpFuseCandidates);",
                 "matcher.Fuse(vpTargetKFs,vpMapPointMatches,3.0,&vnFused,&nReselected);",
                 "matcher.Fuse(vector<KeyFrame*>(1,mpCurrentKeyFrame),vpFuseCandidates,3.0,&vnReverse,&nReselectedReverse);",
                 "if(pMP->isBad() || pMP->mnFuseCandidateForKF == mpCurrentKeyFrame->mnId)"):
        assert expr in text
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    r = subprocess.run([exe, "no-device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert "graph untouched" in r.stdout or "a device is present" in r.stdout


def test_the_existing_shims_still_compile_against_the_header(orbx, tmp_path):
    """the overload is a template: a tree whose classes lack GetFeaturesInArea / GetDistanceRange compiles as long as it does not
    call it (tests/cxx/slam_shims/ has neither)"""
    src = tmp_path / "old_shims.cc"
    src.write_text('#include "ORBextractor.h"\n#include "ORBmatcher.h"\nint main() { ORB_SLAM2::ORBmatcher m; return m.TH_LOW == 50 ? 0 : 1; }\n')
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "slam_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall"] + inc + [str(src), "-o", str(tmp_path / "old_shims"), "-L" + libdir, "-lorbx",
                                                                       "-Wl,-rpath," + libdir, "-pthread"])


@pytest.mark.gpu
def test_both_loops_leave_the_same_graph(orbx, tmp_path):
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuse_views_callsites ok" in r.stdout and "FAILED" not in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("forward fused")][0].replace(",", "").split()
    forward, reverse, res_f, res_r, changed = int(line[2]), int(line[5]), int(line[7]), int(line[9]), int(line[16])
    # the scene is worth the comparison: both halves fuse, the loop rewrites a good part of the graph, and descriptors change between
    # key frames so that the host re-selection runs
    assert forward >= 20 and reverse >= 1 and changed >= 20 and res_f + res_r >= 1, r.stdout
    per = [l for l in r.stdout.splitlines() if l.startswith("per target:")][0].split()[2:]
    assert len(per) == 7 and per[-1] == "0/0" and sum(p != "0/0" for p in per) >= 4, r.stdout
