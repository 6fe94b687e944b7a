"""The C++ adapter my-slam_amd/host/LocalPoints.h at the call site: tests/cxx/localpoints_callsites.cc runs the second half of
Tracking::SearchLocalPoints (src/Tracking.cc:1171-1199) twice on the same object graph (tests/cxx/localpoints_shims/) -- the
reference's isInFrustum loop on the host followed by the matcher, and ORB_SLAM2::SearchLocalPoints as INTEGRATION.md 3i writes
it -- and compares every mTrack* member, the visible counters and F.mvpMapPoints.

The host loop takes its logarithm from the C library, the kernel the correctly rounded one: the two may
disagree on the level of a point whose level quotient lies within |q| * 2^-21 of an integer (tests/test_frustum_cpu.py), so the
case generator leaves such points out (none on these seeds so far; the count is asserted to stay small)."""
import os
import subprocess

import numpy as np
import pytest

import frustum_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "localpoints_callsites.cc")


def compile_callsites(orbx, tmp_path):
    exe = str(tmp_path / "localpoints_callsites")
    libdir = os.path.dirname(orbx.LIB_PATH)
    inc = ["-I" + os.path.join(ROOT, "my-slam_amd", "host"), "-I" + os.path.join(ROOT, "tests", "cxx", "localpoints_shims"),
           "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter"] + inc +
                          [SRC, "-o", exe, "-L" + libdir, "-lorbx", "-Wl,-rpath," + libdir])
    return exe


def write_case(path, sc, fr, kind, frame_id=7):
    with open(path, "wb") as f:
        f.write(np.array([len(sc), len(fr.kps), frame_id], np.int32).tobytes())
        f.write(np.asarray(sc.view, F.VIEW_DTYPE).tobytes())
        for a in (kind.astype(np.uint8), sc.xw, sc.normal, sc.mf_max, sc.mf_min, fr.mp_desc, fr.mp_obs, fr.kps, fr.desc, fr.u_right, fr.cur_obs):
            f.write(np.ascontiguousarray(a).tobytes())


def test_call_site_compiles_the_reference_expressions(orbx, tmp_path):
    orbx.build()
    exe = compile_callsites(orbx, tmp_path)
    text = open(SRC).read()
    for expr in ("if (pMP->mnLastFrameSeen == mCurrentFrame.mnId)", "if (pMP->isBad())", "if (mCurrentFrame.isInFrustum(pMP, 0.5)) {",
                 "pMP->IncreaseVisible();", "nToMatch++;", "if (nToMatch > 0) {",
                 "ORB_SLAM2::SearchLocalPoints(mCurrentFrame, mvpLocalMapPoints, th, 0.8f, &err)"):
        assert expr in text
    shim = open(os.path.join(ROOT, "tests", "cxx", "localpoints_shims", "MapPoint.h")).read()
    assert "void GetDistanceRange(float &mfMax, float &mfMin)" in shim
    assert "GetDistanceRange" in open(os.path.join(ROOT, "my-slam_amd", "host", "LocalPoints.h")).read()
    assert subprocess.run([exe, "compile-only"]).returncode == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th,kw", [(81, 1.0, dict()), (82, 3.0, dict(stereo=False)), (83, 5.0, dict(turn=0.4, wild_share=0.5)),
                                        (84, 3.0, dict(scale_factor=1.0, nlevels=1, degenerate_share=0.0))])
def test_search_local_points_object_graph(orbx, tmp_path, seed, th, kw):
    exe = compile_callsites(orbx, tmp_path)
    rng = np.random.default_rng(seed)
    kw = dict(dict(degenerate_share=0.0), **kw)         # the host loop's int conversion of a non-finite quotient is undefined: not comparable
    sc = F.make_scene(rng, 3000, **kw)
    dist = F.distance(sc.view, sc.xw)
    with np.errstate(all="ignore"):
        q = np.log((sc.mf_max / dist).astype(np.longdouble)) / np.longdouble(sc.view["log_scale_factor"])
        tie = np.isfinite(q) & (np.abs(q - np.rint(q)) <= np.abs(q) * np.longdouble(2.0) ** -21)
    assert tie.sum() < 5
    keep = ~tie
    sc = F.Scene(sc.view, sc.skip[keep], sc.xw[keep], sc.normal[keep], sc.mf_max[keep], sc.mf_min[keep])
    fr = F.make_frame(rng, sc)
    kind = np.where(sc.skip != 0, rng.integers(1, 3, len(sc)), 0)       # skipped: seen in this frame already, or bad
    st = F.frustum(*sc.args(), 0.5)
    if kw.get("nlevels") == 1:
        # mfLogScaleFactor = 0: every quotient is inf or nan, which the host's (int) conversion cannot be compared on; keep the
        # points that never reach PredictScale
        keep = st[0] != F.UNDEFINED
        sc = F.Scene(sc.view, sc.skip[keep], sc.xw[keep], sc.normal[keep], sc.mf_max[keep], sc.mf_min[keep])
        fr.mp_desc, fr.mp_obs, kind = fr.mp_desc[keep], fr.mp_obs[keep], kind[keep]
        st = F.frustum(*sc.args(), 0.5)
    case = str(tmp_path / "case.bin")
    write_case(case, sc, fr, kind)
    r = subprocess.run([exe, case, str(th)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nToMatch %d," % st[6] in r.stdout and " 0 differences" in r.stdout
    if kw.get("nlevels") != 1:
        assert st[6] > 300
