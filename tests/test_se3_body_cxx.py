"""The quaternion / SE3 group every optimizer shares (my-slam_amd/csrc/orbp_se3_body.h): tests/cxx/se3_body_check.cc, built
stand-alone under AddressSanitizer and UBSan on the CPU, checks quat_from_R bit for bit against Eigen's index form on rotations of
0, 1e-6, 0.3, 2.2, 2.9, 3.1 and pi rad about axes at and 0.05 off x, y and z (all four branches taken and counted), that
quat_normalize flips a negative w, se3_exp on either side of theta = 1e-5 and up to 3 (quat_to_R(exp) orthonormal, exp(u) * exp(-u)
the identity) and se3_mul against the 4 x 4 product in long double, each within a bound derived in the source from the count of
roundings."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "se3_body_check.cc")
CSRC = os.path.join(ROOT, "my-slam_amd", "csrc")


def test_the_se3_group_against_eigens_index_form_and_the_matrix_product_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "se3_body_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "se3_body_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
