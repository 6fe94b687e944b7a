"""Regenerates tests/golden/mapping/: the requests of tests/ref_mapping.py's pinned cases, the responses oracle/_ref/ref_mapping (the
reference's own src/MapPoint.cc, Frame::isInFrustum and LocalMapping::CreateNewMapPoints) gives for them, the inputs on which its UBSan
copy reports the undefined int conversion, and tolerance.json.  Data only: the requests are this project's, the responses are flags,
levels, float values and descriptors.  Needs the reference tree (make -C oracle/ref mapping measure).

    python tests/golden/make_golden_mapping.py
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ref_mapping as R      # noqa: E402


def main():
    if not (R.ensure(variants=("", "_ubsan", "_b")) and R.ensure_loop(variants=("", "_ubsan", "_b"))):
        sys.exit("oracle/_ref/ref_mapping is not built and the reference tree is not present")
    tol = R.record_fixtures()
    R.record_loop_fixtures()
    for kind in R.KINDS + R.LOOP_KINDS:
        print("%s: %d bytes" % (kind, os.path.getsize(R.fixture_path(kind))))
    print("x3D of the SVD: spread C / B %.3e over %d pairs, tolerance %.3e" % (tol["spread_c_b"], tol["pairs"], tol["tolerance"]))


if __name__ == "__main__":
    main()
