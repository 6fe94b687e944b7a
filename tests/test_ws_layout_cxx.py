"""WsLayout (my-slam_amd/csrc/ws_layout.h), the one typed carve of the optimizers' workspace block: tests/cxx/ws_layout_check.cc,
built stand-alone under AddressSanitizer and UBSan on the CPU, binds mixed element types (double, float, int32_t, uint8_t) with
counts of 0, 1, 7 and 8 and an odd byte count and checks that every pointer is base + k * 64, that consecutive parts neither overlap
nor leave the block, that bytes() is the sum of the rounded sizes, that an empty part gets the next part's address and that a second
bind moves every field."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "ws_layout_check.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


def test_the_workspace_carve_is_aligned_disjoint_and_rebinds_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "ws_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ws_layout_check ok: 13 parts, 704 bytes" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
