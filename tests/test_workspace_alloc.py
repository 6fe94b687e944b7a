"""Creation-failure sweep of the handles' device memory, streams and events on the CPU: tests/cxx/workspace_alloc_sweep.cc supplies
the HIP calls itself (malloc behind them, every creation made to fail in turn) and runs under AddressSanitizer + UBSan as a
stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_workspace_allocation_failure_sweep(tmp_path):
    exe = str(tmp_path / "workspace_alloc_sweep")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cxx", "workspace_alloc_sweep.cc"),
                           os.path.join(CSRC, "orbm_workspace.cc"), os.path.join(CSRC, "orbv_workspace.cc"),
                           os.path.join(CSRC, "orbk_workspace.cc"), os.path.join(CSRC, "orbx_workspace.cc"),
                           os.path.join(CSRC, "orbx_plan.cc"), "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "sweep ok" in out.stdout and "ERROR" not in out.stderr and "runtime error" not in out.stderr
    for case in ("orbm_reserve", "orbm_grow", "grid ensure", "ensure_partials", "dd_scratch growth", "orbm_arena_begin",
                 "orbv feature buffers", "orbk ensure_io", "orbk make_room",
                 "orbx_create", "orbx colour buffers", "orbx pyramid staging", "orbx chunk events", "orbx ring events"):
        assert "ok " + case in out.stdout, case
