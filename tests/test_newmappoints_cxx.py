"""The C++ adapter my-slam_amd/host/NewMapPoints.h at the call site: tests/cxx/newmappoints_callsites.cc runs
LocalMapping::CreateNewMapPoints as INTEGRATION.md 3h writes it, on repo-authored KeyFrame / MapPoint / Map classes
(tests/cxx/newmappoints_shims/), and compares the object graph with a replay of src/LocalMapping.cc:436-451 over the accepted
list of tests/triangulation_oracle.py, which this file writes into the case file."""
import os
import subprocess

import numpy as np
import pytest

import triangulation_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "newmappoints_callsites.cc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "newmappoints_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "newmappoints_shims"),
           "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    return exe


def write_case(path, cam1, kf1, cam2, kf2, matches, status, x3d, rng):
    with open(path, "wb") as f:
        f.write(np.array([len(kf1), len(kf2), len(matches)], np.int32).tobytes())
        for cam, kf in ((cam1, kf1), (cam2, kf2)):
            f.write(np.asarray(cam, T.CAM_DTYPE).tobytes())
            for a in (kf.kps_un, kf.keys_xy, kf.u_right, kf.depth, rng.integers(0, 256, (len(kf), 32), dtype=np.uint8)):
                f.write(np.ascontiguousarray(a).tobytes())
        f.write(np.ascontiguousarray(matches[:, :2], np.int32).tobytes())
        f.write(status.tobytes())
        f.write(x3d.tobytes())


def test_call_site_compiles_the_reference_expressions(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for expr in ("MapPoint *pMP = new MapPoint(x3D[ikp], mpCurrentKeyFrame, mpMap);", "pMP->AddObservation(mpCurrentKeyFrame, idx1);",
                 "pMP->AddObservation(pKF2, idx2);", "mpCurrentKeyFrame->AddMapPoint(pMP, idx1);", "pKF2->AddMapPoint(pMP, idx2);",
                 "pMP->UpdateNormalAndDepth();", "mpMap->AddMapPoint(pMP);", "mlpRecentAddedMapPoints.push_back(pMP);",
                 "TriangulateMatches(mpCurrentKeyFrame, pKF2, vMatchedIndices, status, x3D, &err)", "ComputeDistinctiveDescriptors(vpNewMapPoints"):
        assert expr in text
    assert subprocess.run([exe, "compile-only"]).returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", [(71, dict()), (72, dict(stereo1=0, stereo2=0, baseline=2.0)), (73, dict(stereo1=1, stereo2=1, baseline=0.05))])
def test_create_new_map_points_object_graph(orbx, tmp_path, seed, kw):
    exe = compile_callsites(orbx, tmp_path)
    rng = np.random.default_rng(seed)
    cam1, kf1, cam2, kf2, matches = T.make_pair(rng, 800, outliers=0.0, **kw)
    # SearchForTriangulation gives every feature of key frame 1 at most one partner, in ascending idx1
    matches = matches[np.argsort(matches[:, 0])]
    status, x3d = T.triangulate(cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)
    assert (status <= T.STEREO2).sum() > 100 and (status > T.STEREO2).sum() > 50
    case = str(tmp_path / "case.bin")
    write_case(case, cam1, kf1, cam2, kf2, matches, status, x3d, rng)
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d new MapPoints" % int((status <= T.STEREO2).sum()) in r.stdout
