"""Optimizer::OptimizeEssentialGraph of my-slam_amd/host/PnPsolver.h at its call site: tests/cxx/eg_callsites.cc holds the line
src/LoopClosing.cc:568 verbatim on the classes of tests/cxx/eg_shims/, compares the gathered edge list with a hand-written walk of
src/Optimizer.cc:852-983 over the same objects (the minFeat exception for the (current, loop) pair, the sInsertedEdges skip, the
parent / child / loop-edge skips, a bad and a NULL covisible) and the object graph afterwards with what the flat call
orbp_optimize_essential_graph dictates.  The same program, built stand-alone over orbp_eg.cc, orbp_sim3opt.cc and orbp.cc, runs
the gather, the host solver and the scatter under AddressSanitizer and UBSan on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "eg_callsites.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")
INC = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "eg_shims"), "-I" + os.path.join(ROOT, "include")]


def check(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "eg_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "9 key frames, 17 edges, 11 points" in r.stdout
    return r


def test_the_reference_line_compiles_verbatim_and_the_object_graph_is_what_the_flat_call_dictates(orbx, tmp_path):
    orbx.build()
    exe = str(tmp_path / "eg_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + INC +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    text = open(SRC).read()
    assert ("Optimizer::OptimizeEssentialGraph(mpMap, mpMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, mbFixScale);"
            in text)
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    check(exe)


def test_gather_host_solver_and_scatter_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "eg_callsites_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-DEG_CALLSITES_STANDALONE", "-pthread"] + INC +
                          [SRC, os.path.join(CSRC, "orbp_eg.cc"), os.path.join(CSRC, "orbp_sim3opt.cc"), os.path.join(CSRC, "orbp.cc"), "-o", exe])
    r = check(exe)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
