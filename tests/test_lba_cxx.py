"""Optimizer::LocalBundleAdjustment of my-slam_amd/host/PnPsolver.h at its call site: tests/cxx/lba_callsites.cc holds the line
src/LocalMapping.cc:82 verbatim on the classes of tests/cxx/lba_shims/ and compares the object graph after it with what the flat
call orbp_local_bundle_adjustment dictates.  tests/cxx/lba_asan_main.cc drives orbp_local_bundle_adjustment stand-alone under
AddressSanitizer and UBSan on the CPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "lba_callsites.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "lba_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "lba_shims"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir, "-pthread"])
    return exe


def test_the_reference_line_compiles_verbatim_and_the_object_graph_is_what_the_flat_call_dictates(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    assert "Optimizer::LocalBundleAdjustment(mpCurrentKeyFrame,&mbAbortBA, mpMap);" in open(SRC).read()
    assert subprocess.run([exe, "compile-only"]).returncode == 0
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lba_callsites ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "host: 4 local, 2 fixed, 119 points" in r.stdout


def test_the_host_solver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lba_asan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cxx", "lba_asan_main.cc"), os.path.join(CSRC, "orbp_lba.cc"),
                           os.path.join(CSRC, "orbp.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lba_asan_main ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
def test_the_handle_overload_agrees_with_the_host_form(orbx, tmp_path):
    """the same call site through orbm_local_bundle_adjustment: the same erased pairs, poses and positions within the bar of
    tests/golden/lba/tolerance.json"""
    bar = json.load(open(os.path.join(ROOT, "tests", "golden", "lba", "tolerance.json")))["bar"]
    exe = compile_callsites(orbx, tmp_path)
    r = subprocess.run([exe, "gpu"] + [repr(bar[k]) for k in ("rotation", "translation", "point")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "lba_callsites ok" in r.stdout and "FAILED" not in r.stdout
