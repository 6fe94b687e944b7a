"""The C++ adapter Optimizer::PoseOptimizationBatch (my-slam_amd/host/PnPsolver.h) at the call site: tests/cxx/pose_batch_check.cc
runs Optimizer::PoseOptimization (the host path) on every problem of a case file and PoseOptimizationBatch on all of them in one
launch, and compares poses (2e-6), flags and return values."""
import os
import subprocess

import numpy as np
import pytest

import pose_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "pose_batch_check.cc")


def compile_check(orbx, tmp_path):
    exe = str(tmp_path / "pose_batch_check")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    return exe


def write_case(path, problems):
    with open(path, "wb") as f:
        f.write(np.array([len(problems)], np.int32).tobytes())
        for obs, inv_s2, xw, fx, fy, cx, cy, T0, ur, bf in problems:
            f.write(np.array([len(obs), ur is not None], np.int32).tobytes())
            f.write(np.array([fx, fy, cx, cy, bf], np.float32).tobytes())
            f.write(np.ascontiguousarray(T0, np.float32).tobytes())
            for a in (obs, inv_s2, xw) + ((ur,) if ur is not None else ()):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())


def test_adapter_compiles_and_refuses_a_null_matcher(orbx, tmp_path):
    orbx.build()
    exe = compile_check(orbx, tmp_path)
    text = open(os.path.join(ROOT, "my-slam_amd", "host", "PnPsolver.h")).read()
    assert "static int PoseOptimizationBatch(orbm_matcher *matcher, std::vector<PoseProblem> &problems" in text
    r = subprocess.run([exe, "compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "NULL matcher: status" in r.stdout


@pytest.mark.gpu
def test_batch_adapter_equals_the_host_adapter(orbx, tmp_path):
    exe = compile_check(orbx, tmp_path)
    problems = pc.cases()["mixed"] + pc.cases()["all_outliers"] + pc.cases()["fixed_point"]
    case = str(tmp_path / "case.bin")
    write_case(case, problems)
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d problems, 0 differences" % len(problems) in r.stdout
