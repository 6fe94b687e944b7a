"""No-GPU checks of the CreateNewMapPoints per-match loop (include/orbm.h, orbm_triangulate_matches): hand-built cases of the
restatement tests/triangulation_oracle.py for every status, with the expected value worked out in the comment; the two quirks
of the reference the library keeps; the fp64 Jacobi against numpy.linalg.svd; both exports; the argument checks made before
any device work; and the loud failure without a GPU.

The hand-built rig: fx = fy = 100, principal point (320, 240), key frame 1 at the origin looking down z, key frame 2 with the
same orientation one metre to its right (tcw2 = (-1, 0, 0)).  mbf = 200, so mb = 2.  A point (X, Y, Z) is seen at
u1 = 320 + 100 X / Z and u2 = 320 + 100 (X - 1) / Z."""
import ctypes as C

import numpy as np
import pytest

import triangulation_oracle as T

f32 = np.float32


def rig(t2=(-1, 0, 0), mbf2=200, sigma1=None, sigma2=None):
    cam1 = T.make_camera(np.eye(3), [0, 0, 0], 100, 100, 320, 240, 200, level_sigma2=sigma1)
    cam2 = T.make_camera(np.eye(3), t2, 100, 100, 320, 240, mbf2, level_sigma2=sigma2)
    return cam1, cam2


def feature(u, v, octave=0, ur=-1, depth=-1, raw=None):
    kp = np.zeros(1, T.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = u, v, octave
    return T.KeyFrame(kp, [raw if raw is not None else (u, v)], [ur], [depth])


def one(cam1, f1, cam2, f2):
    st, x = T.triangulate(cam1, f1, [cam2], [0, 1], f2, [[0, 0, 0]])
    return int(st[0]), x[0]


def test_accepted_by_svd():
    # (0.5, 0, 5): u1 = 330, u2 = 310.  Rays (0.1, 0, 1) and (-0.1, 0, 1): cos = 0.99 / 1.01 = 0.980 < 0.9998.  Both depths 5,
    # distances equal, octaves equal: accepted, and the two lines meet in the point itself
    cam1, cam2 = rig()
    st, x = one(cam1, feature(330, 240), cam2, feature(310, 240))
    assert st == T.SVD and np.allclose(x, [0.5, 0, 5], atol=1e-5)


def test_low_parallax():
    # the same point at Z = 500: u = 320.1 and 319.9, rays 0.002 rad apart, cos = 0.999998 >= 0.9998, nobody is stereo
    cam1, cam2 = rig()
    st, x = one(cam1, feature(320.1, 240), cam2, feature(319.9, 240))
    assert st == T.LOW_PARALLAX and not x.any()


def test_unproject_stereo_of_view_1():
    # Z = 500 again, the first feature stereo: cosParallaxStereo1 = cos(2 atan2(1, 500)) = cos(0.004) = 0.999992 < the rays'
    # 0.999998, so no triangulation, and :342 takes UnprojectStereo(idx1) = ((320.1 - 320) * 500 / 100, 0, 500).
    # uRight = u - mbf / Z = 320.1 - 0.4 keeps the stereo test of :387 at zero
    cam1, cam2 = rig()
    st, x = one(cam1, feature(320.1, 240, ur=319.7, depth=500), cam2, feature(319.9, 240))
    assert st == T.STEREO1 and np.allclose(x, [0.5, 0, 500], atol=1e-2)


def test_unproject_stereo_of_view_2():
    # the mirror image: ((319.9 - 320) * 500 / 100, 0, 500) in camera 2 = (-0.5 + 1, 0, 500) in the world
    cam1, cam2 = rig()
    st, x = one(cam1, feature(320.1, 240), cam2, feature(319.9, 240, ur=319.5, depth=500))
    assert st == T.STEREO2 and np.allclose(x, [0.5, 0, 500], atol=1e-2)


def test_quirk_else_if_ignores_the_second_stereo_angle():
    # both stereo, the second feature claiming a depth of 1 m: cos(2 atan2(1, 1)) = 0 would be the minimum and :346 would
    # unproject view 2 to Z = 1.  `else if(bStereo2)` (:315) never looks at it once view 1 is stereo: cosParallaxStereo2 stays
    # cosParallaxRays + 1 and :342 wins.  u2_r = 319.9 - 200 / 500 = 319.5
    cam1, cam2 = rig()
    st, x = one(cam1, feature(320.1, 240, ur=319.7, depth=500), cam2, feature(319.9, 240, ur=319.5, depth=1))
    assert st == T.STEREO1 and np.allclose(x, [0.5, 0, 500], atol=1e-2)


def test_quirk_second_stereo_test_uses_the_first_key_frames_mbf():
    # key frame 2 with mbf = 2000: its own right coordinate of the point would be 319.9 - 2000 / 500 = 315.9, but :408 predicts
    # 319.9 - 200 / 500 = 319.5 with mpCurrentKeyFrame->mbf.  A feature at 319.5 passes; one at 315.9 is 3.6 px off: 12.96 > 7.8
    cam1, cam2 = rig(mbf2=2000)
    f1 = feature(320.1, 240, ur=319.7, depth=500)
    assert one(cam1, f1, cam2, feature(319.9, 240, ur=319.5, depth=500))[0] == T.STEREO1
    assert one(cam1, f1, cam2, feature(319.9, 240, ur=315.9, depth=500))[0] == T.REPROJ2


def test_quirk_unproject_stereo_reads_the_raw_key():
    # mvKeys 10 px right of mvKeysUn: UnprojectStereo gives X = (330.1 - 320) * 500 / 100 = 50.5, not 0.5, and the projection
    # lands 10 px from mvKeysUn: 100 > 7.8.  With a wide gate (sigma^2 = 10^4) the point is accepted as it is
    cam1, cam2 = rig()
    f1 = feature(320.1, 240, ur=319.7, depth=500, raw=(330.1, 240))
    assert one(cam1, f1, cam2, feature(319.9, 240))[0] == T.REPROJ1
    wide = np.full(T.MAX_LEVELS, 1e4)
    cam1, cam2 = rig(sigma1=wide, sigma2=wide)
    st, x = one(cam1, f1, cam2, feature(319.9, 240))
    assert st == T.STEREO1 and np.allclose(x, [50.5, 0, 500], atol=1e-2)


def test_behind_camera_1():
    # the two features swapped (310 / 330): x = -0.1 z and x - 1 = 0.1 z meet at z = -5
    cam1, cam2 = rig()
    assert one(cam1, feature(310, 240), cam2, feature(330, 240))[0] == T.BEHIND1


def test_behind_camera_2():
    # key frame 2 ten metres AHEAD (tcw2 = (0, 0, -10)); rays (0.1, 0, 1) and (-0.1, 0, 1) meet at (0.5, 0, 5): z1 = 5, z2 = -5
    cam1, cam2 = rig(t2=(0, 0, -10))
    assert one(cam1, feature(330, 240), cam2, feature(310, 240))[0] == T.BEHIND2


def test_reprojection_gates():
    # the accepted pair with the first feature 20 px too low: the rays miss each other, the point lands about 10 px from
    # either feature, 100 > 5.991.  The first gate fires first; with the first gate wide open the second fires
    cam1, cam2 = rig()
    assert one(cam1, feature(330, 260), cam2, feature(310, 240))[0] == T.REPROJ1
    cam1, cam2 = rig(sigma1=np.full(T.MAX_LEVELS, 1e4))
    assert one(cam1, feature(330, 260), cam2, feature(310, 240))[0] == T.REPROJ2


def test_scale_consistency():
    # the accepted pair, equal distances, octaves 0 and 7: ratioOctave = 1 / 1.2^7 = 0.279, and 1 > 0.279 * 1.8 = 0.50
    cam1, cam2 = rig()
    assert one(cam1, feature(330, 240, octave=0), cam2, feature(310, 240, octave=7))[0] == T.SCALE
    assert one(cam1, feature(330, 240, octave=7), cam2, feature(310, 240, octave=0))[0] == T.SCALE     # 1 * 1.8 < 3.58
    assert one(cam1, feature(330, 240, octave=3), cam2, feature(310, 240, octave=5))[0] == T.SVD        # 0.69: inside


def test_undefined_case_has_its_own_status():
    # a stereo feature (uRight >= 0) with depth 0: atan2(1, 0) = pi/2, cos(pi) = -1, :342 calls UnprojectStereo, which
    # returns an empty matrix that :353 then reads.  Rejected with its own status; nothing is compared
    cam1, cam2 = rig()
    st, x = one(cam1, feature(330, 240, ur=300, depth=0), cam2, feature(310, 240))
    assert st == T.UNDEFINED and not x.any()
    assert one(cam1, feature(330, 240), cam2, feature(310, 240, ur=300, depth=-1))[0] == T.UNDEFINED


def test_zero_distance_and_w_zero_inputs_reach_their_lines():
    for make, code in ((T.zero_distance_cases, T.ZERO_DIST), (T.w_zero_cases, T.W_ZERO)):
        cam1, kf1, cam2, kf2, m = make()
        st, x = T.triangulate(cam1, kf1, [cam2], [0, len(kf2)], kf2, m)
        assert len(st) >= 20 and (st == code).all() and not x.any()


def test_w_zero_by_hand():
    # the degenerate second view of w_zero_cases: A = [[-1, 0, x, 0], [0, -1, y, 0], [0, 0, 0, 1], [0, 0, 0, 2]], whose null
    # vector is (x, y, 1, 0) / norm
    cam1, kf1, cam2, kf2, m = T.w_zero_cases(3)
    st, x, det = T.triangulate(cam1, kf1, [cam2], [0, 3], kf2, m, return_details=True)
    A, v = det["A"][0], det["v"][0]
    assert np.array_equal(A[2:], [[0, 0, 0, 1], [0, 0, 0, 2]]) and np.array_equal(A[:2, 3], [0, 0])
    assert v[3] == 0 and np.allclose(v[:3] / v[2], [A[0, 2], A[1, 2], 1], rtol=1e-12)


def test_cos_stereo_is_the_correctly_rounded_float_pair():
    # atan2f then cosf, each rounded once: compared with mpmath-free exact knowledge at three points
    assert T.cos_stereo(f32([2.0]), f32([0.0]))[0] == f32(-1)                     # cos(2 * float(pi / 2)) rounds to -1
    assert T.cos_stereo(f32([2.0]), f32([1.0]))[0] == f32(np.cos(np.longdouble(f32(2) * f32(np.pi / 4))))
    big = T.cos_stereo(f32([0.5]), f32([1e6]))[0]
    assert big == f32(1) or big == np.nextafter(f32(1), f32(0))


# ---- the fp64 Jacobi against LAPACK

def _svd_accepted(seed, **kw):
    rng = np.random.default_rng(seed)
    cam1, kf1, cam2, kf2, m = T.make_pair(rng, 4000, **kw)
    st, x, det = T.triangulate(cam1, kf1, [cam2], [0, len(kf2)], kf2, m, return_details=True)
    keep = st == T.SVD
    return det["A"][keep], x[keep]


@pytest.mark.parametrize("seed,kw", [(1, dict(stereo1=0, stereo2=0)), (2, dict(baseline=5.0)), (3, dict(baseline=0.2, stereo1=0.2, stereo2=0.2)),
                                     (4, dict(stereo1=0, stereo2=0, baseline=1.5, depth=(1.0, 120.0), noise=1.5))])
def test_jacobi_equals_lapack_svd_rounded_to_float(seed, kw):
    """On the same float matrices numpy.linalg.svd in float64 gives the same x3D after the one rounding to float: within 1 ulp
    per coordinate on every SVD-accepted match, bit-equal on at least 99 % (the cap covers round-to-float ties between two fp64
    algorithms)."""
    A, x = _svd_accepted(seed, **kw)
    assert len(A) >= 300
    vt = np.linalg.svd(A.astype(np.float64))[2][:, 3, :]
    ref = (vt[:, :3] / vt[:, 3:4]).astype(f32)
    ulps = np.abs(ref.view(np.int32).astype(np.int64) - x.view(np.int32).astype(np.int64))
    print("matches %d, max ulp %d, bit-equal share %.5f" % (len(A), ulps.max(), (ulps.max(1) == 0).mean()))
    assert ulps.max() <= 1
    assert (ulps.max(1) == 0).mean() >= 0.99


def test_jacobi_needs_far_fewer_sweeps_than_its_bound():
    A, _ = _svd_accepted(5)
    v, sweeps = T.smallest_right_singular_vector(A, return_sweeps=True)
    assert sweeps.max() <= T.MAX_SWEEPS - 4
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-12)


def test_several_views_equal_single_view_calls():
    rng = np.random.default_rng(9)
    pairs = [T.make_pair(rng, 150, baseline=b) for b in (0.1, 1.0, 3.0)]
    cam1, kf1 = pairs[0][0], pairs[0][1]
    singles = [T.triangulate(cam1, kf1, [p[2]], [0, len(p[3])], p[3], p[4]) for p in pairs]
    off2, kf2 = T.concat_keyframes([p[3] for p in pairs])
    m = np.concatenate([np.concatenate([p[4][:, :2], np.full((len(p[4]), 1), v, np.int32)], 1) for v, p in enumerate(pairs)])
    order = rng.permutation(len(m))
    st, x = T.triangulate(cam1, kf1, np.array([p[2] for p in pairs]), off2, kf2, m[order])
    assert np.array_equal(st, np.concatenate([s[0] for s in singles])[order])
    assert np.array_equal(x.view(np.uint32), np.concatenate([s[1] for s in singles])[order].view(np.uint32))


# ---- the library without a GPU

@pytest.fixture(scope="module")
def built(orbx):
    orbx.build()
    return orbx


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_both_symbols_are_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    assert hasattr(lib, "orbm_triangulate_matches") and hasattr(lib, "orbm_triangulate_matches_device")
    assert hasattr(built.ORBmatcher, "triangulate_matches") and hasattr(built.ORBmatcher, "triangulate_matches_device")
    assert built.CAM_DTYPE == T.CAM_DTYPE and built.KP_DTYPE == T.KP_DTYPE


def _args(built, n=40, seed=3):
    cam1, kf1, cam2, kf2, m = T.make_pair(np.random.default_rng(seed), n)
    a = dict(cam1=np.array([cam1]), k1=kf1.kps_un.copy(), x1=kf1.keys_xy, u1=kf1.u_right, d1=kf1.depth, cams2=np.array([cam2]),
             off2=np.array([0, n], np.int32), k2=kf2.kps_un.copy(), x2=kf2.keys_xy, u2=kf2.u_right, d2=kf2.depth, m=m.copy(),
             st=np.full(n, 77, np.uint8), x=np.full((n, 3), 77, f32), n=n)
    return a


def _call(Lb, a, handle=None, n=None, n1=None, ncams2=None):
    return Lb.orbm_triangulate_matches(handle, p(a["cam1"]), p(a["k1"]), p(a["x1"]), p(a["u1"]), p(a["d1"]), a["n"] if n1 is None else n1,
                                       p(a["cams2"]), 1 if ncams2 is None else ncams2, p(a["off2"]), p(a["k2"]), p(a["x2"]),
                                       p(a["u2"]), p(a["d2"]), p(a["m"]), a["n"] if n is None else n, p(a["st"]), p(a["x"]))


def test_argument_checks_come_before_any_device_work(built):
    """With a NULL handle (none can be made without a GPU) every bad argument still gets ORBX_E_INVALID and a text."""
    Lb = built.lib()
    E = built.ORBX_E_INVALID
    a = _args(built)
    assert _call(Lb, a, n=-1) == E and b"n=-1" in Lb.orbm_last_error()
    assert _call(Lb, a, n=0) == built.ORBX_OK
    assert Lb.orbm_triangulate_matches(None, *([None] * 5), 0, None, 0, *([None] * 6), 0, None, None) == built.ORBX_OK
    assert _call(Lb, a, ncams2=0) == E and b"ncams2" in Lb.orbm_last_error()
    for key in ("cam1", "k1", "x1", "u1", "d1", "cams2", "off2", "k2", "x2", "u2", "d2", "m", "st", "x"):
        b = dict(a)
        b[key] = None
        assert _call(Lb, b) == E and b"NULL" in Lb.orbm_last_error(), key

    def bad(mutate, text):
        b = _args(built)
        mutate(b)
        assert _call(Lb, b) == E and text in Lb.orbm_last_error(), Lb.orbm_last_error()
        assert (b["st"] == 77).all() and (b["x"] == 77).all()

    bad(lambda b: b["m"].__setitem__((5, 0), 40), b"feature index 40")
    bad(lambda b: b["m"].__setitem__((5, 0), -1), b"feature index -1")
    bad(lambda b: b["m"].__setitem__((7, 1), 40), b"feature index 40")
    bad(lambda b: b["m"].__setitem__((7, 2), 1), b"view 1")
    bad(lambda b: b["m"].__setitem__((7, 2), -1), b"view -1")
    bad(lambda b: b["k1"]["octave"].__setitem__(slice(None), 8), b"octave 8")
    bad(lambda b: b["k2"]["octave"].__setitem__(slice(None), -1), b"octave -1")
    bad(lambda b: b["off2"].__setitem__(0, 1), b"off2[0]")
    bad(lambda b: b["off2"].__setitem__(1, -3), b"monotone")
    bad(lambda b: b["cam1"]["nlevels"].__setitem__(0, 17), b"nlevels=17")
    bad(lambda b: b["cams2"]["nlevels"].__setitem__(0, 0), b"nlevels=0")
    g = Lb.orbm_triangulate_matches_device
    assert g(None, *([None] * 5), 0, None, 0, *([None] * 6), 0, None, None, None) == built.ORBX_OK
    assert g(None, *([None] * 5), 0, None, 0, *([None] * 6), -2, None, None, None) == E
    assert g(None, *([None] * 5), 5, None, 1, *([None] * 6), 3, None, None, None) == E and b"NULL" in Lb.orbm_last_error()


def test_the_host_array_entry_point_fails_loudly_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    Lb = built.lib()
    a = _args(built)
    assert _call(Lb, a) == built.ORBX_E_HIP
    assert b"no CPU path" in Lb.orbm_last_error()
    assert (a["st"] == 77).all() and (a["x"] == 77).all()                # no half answer
    with pytest.raises(built.OrbxError) as ei:
        built.ORBmatcher()
    assert ei.value.code == built.ORBX_E_HIP
