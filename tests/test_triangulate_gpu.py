"""The CreateNewMapPoints per-match loop on the MI355X (orbm_triangulate_matches, include/orbm.h) against the restatement
tests/triangulation_oracle.py: statuses equal, x3D equal as bit patterns.  The undefined case is compared as a status only (both
sides reject it).  Every test here needs the symbol, so all of them fail on a library built without
my-slam_amd/csrc/orbm_triangulate.hip."""
import numpy as np
import pytest

import triangulation_oracle as T

pytestmark = pytest.mark.gpu

# the scenes of the suite: monocular pairs, the four bStereo1 x bStereo2 combinations, baselines short enough that :342 / :346 take
# UnprojectStereo and long enough that the triangulation wins, outlier shares
SCENES = [
    ("mono", 11, dict(stereo1=0, stereo2=0)),
    ("mono-wide", 12, dict(stereo1=0, stereo2=0, baseline=4.0, outliers=0.3)),
    ("stereo-stereo-short", 13, dict(stereo1=1, stereo2=1, baseline=0.05)),
    ("stereo-stereo-wide", 14, dict(stereo1=1, stereo2=1, baseline=5.0)),
    ("mono-stereo-short", 15, dict(stereo1=0, stereo2=1, baseline=0.03)),
    ("mono-stereo-wide", 16, dict(stereo1=0, stereo2=1, baseline=3.0, mbf2=200.0)),
    ("stereo-mono-short", 17, dict(stereo1=1, stereo2=0, baseline=0.04)),
    ("stereo-mono-wide", 18, dict(stereo1=1, stereo2=0, baseline=5.0)),
    ("mixed", 19, dict()),
    ("mixed-far", 20, dict(baseline=0.02, stereo1=0.3, stereo2=0.3, depth=(1.0, 80.0))),
    ("mixed-outliers", 21, dict(outliers=0.5, noise=2.0, consistent_octaves=0.3)),
]
N_SCENE = 1500


def scene(name):
    for s in SCENES:
        if s[0] == name:
            return T.make_pair(np.random.default_rng(s[1]), N_SCENE, **s[2])
    raise KeyError(name)


def run(m, cam1, kf1, cams2, off2, kf2, matches):
    return m.triangulate_matches(cam1, kf1.kps_un, kf1.keys_xy, kf1.u_right, kf1.depth, cams2, off2, kf2.kps_un, kf2.keys_xy,
                                 kf2.u_right, kf2.depth, matches)


def check(m, cam1, kf1, cams2, off2, kf2, matches):
    st, x = run(m, cam1, kf1, cams2, off2, kf2, matches)
    est, ex = T.triangulate(cam1, kf1, cams2, off2, kf2, matches)
    assert st.dtype == np.uint8 and x.dtype == np.float32 and x.shape == (len(est), 3)
    bad = np.nonzero(st != est)[0]
    assert len(bad) == 0, "matches %s: status %s, expected %s" % (bad[:8], st[bad[:8]], est[bad[:8]])
    diff = np.nonzero((x.view(np.uint32) != ex.view(np.uint32)).any(1))[0]
    assert len(diff) == 0, "matches %s (status %s): x3D %s, expected %s" % (diff[:4], est[diff[:4]], x[diff[:4]], ex[diff[:4]])
    return st, x


@pytest.fixture()
def matcher(orbx):
    m = orbx.ORBmatcher()
    yield m
    m.close()


def test_every_status_occurs_in_the_suites_inputs():
    """On the oracle's output, so that no test passes by never reaching a branch."""
    total = np.zeros(13, np.int64)
    for name, _, _ in SCENES:
        cam1, kf1, cam2, kf2, matches = scene(name)
        total += np.bincount(T.triangulate(cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)[0], minlength=13)
    for make in (T.zero_distance_cases, T.w_zero_cases):
        cam1, kf1, cam2, kf2, matches = make()
        total += np.bincount(T.triangulate(cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)[0], minlength=13)
    print(dict(zip(T.STATUS_NAMES, total)))
    for code in range(T.UNDEFINED + 1):
        assert total[code] >= 20, (T.STATUS_NAMES[code], total)
    assert total[T.BAD_INDEX] == 0


@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_scene_equals_oracle(matcher, name):
    cam1, kf1, cam2, kf2, matches = scene(name)
    check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)


def test_unproject_winners_of_both_views_occur(matcher):
    """depths that make each of :342 and :346 win, in the scenes built for it"""
    for name, code in (("stereo-mono-short", T.STEREO1), ("mono-stereo-short", T.STEREO2), ("stereo-stereo-short", T.STEREO1)):
        cam1, kf1, cam2, kf2, matches = scene(name)
        st, _ = check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)
        assert (st == code).sum() > 500


@pytest.mark.parametrize("make", [T.zero_distance_cases, T.w_zero_cases], ids=["zero-distance", "w-zero"])
def test_degenerate_inputs_equal_oracle(matcher, make):
    cam1, kf1, cam2, kf2, matches = make()
    st, _ = check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)
    assert len(set(st)) == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_wave_edges(matcher, n):
    cam1, kf1, cam2, kf2, matches = scene("mixed")
    check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches[:n])


def test_no_matches_is_a_success_that_touches_nothing(orbx, matcher):
    cam1, kf1, cam2, kf2, matches = scene("mixed")
    st, x = run(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches[:0])
    assert len(st) == 0 and x.shape == (0, 3)
    L = orbx.lib()
    assert L.orbm_triangulate_matches(matcher.h, *([None] * 5), 0, None, 0, *([None] * 6), 0, None, None) == orbx.ORBX_OK
    assert L.orbm_triangulate_matches_device(matcher.h, *([None] * 5), 0, None, 0, *([None] * 6), 0, None, None, None) == orbx.ORBX_OK


def _three_views(rng):
    pairs = [T.make_pair(rng, 400, baseline=b, stereo1=0.5, stereo2=s2) for b, s2 in ((0.05, 1.0), (1.0, 0.5), (4.0, 0.0))]
    cam1, kf1 = pairs[0][0], pairs[0][1]
    off2, kf2 = T.concat_keyframes([p[3] for p in pairs])
    cams2 = np.array([p[2] for p in pairs])
    parts = [np.concatenate([p[4][:, :2], np.full((len(p[4]), 1), v, np.int32)], 1) for v, p in enumerate(pairs)]
    return cam1, kf1, cams2, off2, kf2, parts, pairs


def test_several_second_views_equal_single_view_calls(matcher):
    rng = np.random.default_rng(31)
    cam1, kf1, cams2, off2, kf2, parts, pairs = _three_views(rng)
    singles = [run(matcher, cam1, kf1, [p[2]], [0, len(p[3])], p[3], p[4]) for p in pairs]
    joined = np.concatenate(parts)
    st, x = check(matcher, cam1, kf1, cams2, off2, kf2, joined)              # view by view: every wave but two sees one view
    assert np.array_equal(st, np.concatenate([s[0] for s in singles]))
    assert np.array_equal(x.view(np.uint32), np.concatenate([s[1] for s in singles]).view(np.uint32))
    order = rng.permutation(len(joined))                                     # shuffled: every wave sees all three
    st2, x2 = check(matcher, cam1, kf1, cams2, off2, kf2, joined[order])
    assert np.array_equal(st2, st[order]) and np.array_equal(x2.view(np.uint32), x[order].view(np.uint32))


def _device_call(orbx, m, cam1, kf1, cams2, off2, kf2, matches, stream=None):
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    cams2 = np.ascontiguousarray(cams2, orbx.CAM_DTYPE).reshape(-1)
    matches = np.ascontiguousarray(matches, np.int32).reshape(-1, 3)
    n = len(matches)
    d = [dev(np.asarray(cam1, orbx.CAM_DTYPE).reshape(1)), dev(kf1.kps_un), dev(kf1.keys_xy), dev(kf1.u_right), dev(kf1.depth),
         dev(cams2), dev(np.asarray(off2, np.int32)), dev(kf2.kps_un), dev(kf2.keys_xy), dev(kf2.u_right), dev(kf2.depth), dev(matches)]
    d_st = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    d_x = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream() if stream is None else stream
    m.triangulate_matches_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), len(kf1),
                                 d[5].data_ptr(), len(cams2), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d[9].data_ptr(),
                                 d[10].data_ptr(), d[11].data_ptr(), n, d_st.data_ptr(), d_x.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    return d_st.cpu().numpy(), d_x.cpu().numpy()


def test_device_pointer_variant_equals_host_variant(orbx, matcher):
    rng = np.random.default_rng(41)
    cam1, kf1, cams2, off2, kf2, parts, _ = _three_views(rng)
    matches = np.concatenate(parts)[rng.permutation(1200)]
    hst, hx = check(matcher, cam1, kf1, cams2, off2, kf2, matches)
    dst, dx = _device_call(orbx, matcher, cam1, kf1, cams2, off2, kf2, matches)
    assert np.array_equal(dst, hst) and np.array_equal(dx.view(np.uint32), hx.view(np.uint32))


def test_device_pointer_variant_marks_what_the_host_variant_refuses(orbx, matcher):
    """Indices the host cannot see: the kernel reads nothing through them and says so."""
    cam1, kf1, cam2, kf2, matches = scene("mixed")
    matches = matches[:200].copy()
    est, ex = T.triangulate(cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)
    wrong = {3: (0, N_SCENE), 40: (0, -1), 64: (1, N_SCENE), 65: (1, -5), 130: (2, 1), 199: (2, -1)}
    for k, (col, val) in wrong.items():
        matches[k, col] = val
    kf1.kps_un["octave"][matches[7, 0]] = 8
    kf2.kps_un["octave"][matches[9, 1]] = -1
    touched = np.isin(matches[:, 0], [matches[7, 0]]) | np.isin(matches[:, 1], [matches[9, 1]])
    touched[list(wrong)] = True
    st, x = _device_call(orbx, matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)
    assert (st[touched] == T.BAD_INDEX).all() and not x[touched].any()
    assert np.array_equal(st[~touched], est[~touched]) and np.array_equal(x[~touched].view(np.uint32), ex[~touched].view(np.uint32))


def test_call_larger_than_the_handle_grows_it(orbx):
    m = orbx.ORBmatcher(max_queries=64, max_train=64, max_pairs=64)
    try:
        cam1, kf1, cam2, kf2, matches = scene("mixed")
        check(m, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches[:40])
        big = np.concatenate([matches] * 4)                                   # 6000 matches, 1500 features a side
        check(m, cam1, kf1, [cam2], [0, len(kf2)], kf2, big)
        check(m, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches[:40])
    finally:
        m.close()


def test_after_other_matcher_calls_on_the_same_handle(orbx, matcher):
    """A grid search, the call, the same grid search: the handle's grid and buffers are as they were."""
    rng = np.random.default_rng(51)
    n = 1500
    kps = np.zeros(n, orbx.KP_DTYPE)
    kps["x"] = rng.uniform(0, 640, n).astype(np.float32); kps["y"] = rng.uniform(0, 480, n).astype(np.float32)
    kps["octave"] = rng.integers(0, 8, n)
    train = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q = train[rng.integers(0, n, 300)].copy()
    x = rng.uniform(0, 640, 300).astype(np.float32); y = rng.uniform(0, 480, 300).astype(np.float32)
    r = np.full(300, 40, np.float32); lo = np.full(300, -1, np.int32)
    L = orbx.lib()

    def search():
        bi, bd, sd = (np.zeros(300, np.int32) for _ in range(3))
        rc = L.orbm_search_area_best2(matcher.h, q.ctypes.data, x.ctypes.data, y.ctypes.data, r.ctypes.data, lo.ctypes.data, lo.ctypes.data,
                                      300, train.ctypes.data, None, bi.ctypes.data, bd.ctypes.data, sd.ctypes.data)
        assert rc == 0, L.orbm_last_error()
        return bi, bd, sd
    assert L.orbm_grid_build(matcher.h, kps.ctypes.data, n, 0.0, 640.0, 0.0, 480.0) == 0
    before = search()
    d = matcher.distances(q, train)
    cam1, kf1, cam2, kf2, matches = scene("mixed-outliers")
    check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches)
    assert L.orbm_grid_count(matcher.h) == n
    after = search()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(matcher.distances(q, train), d)
    check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches[:100])


def test_argument_errors(orbx, matcher):
    cam1, kf1, cam2, kf2, matches = scene("mixed")

    def refused(text, cams2=None, off2=None, m=None, k1=None):
        with pytest.raises(orbx.OrbxError) as ei:
            matcher.triangulate_matches(cam1, kf1.kps_un if k1 is None else k1, kf1.keys_xy, kf1.u_right, kf1.depth,
                                        [cam2] if cams2 is None else cams2, [0, len(kf2)] if off2 is None else off2, kf2.kps_un,
                                        kf2.keys_xy, kf2.u_right, kf2.depth, matches[:50] if m is None else m)
        assert ei.value.code == orbx.ORBX_E_INVALID and text in str(ei.value), str(ei.value)
    bad = matches[:50].copy(); bad[10, 0] = N_SCENE
    refused("feature index", m=bad)
    bad = matches[:50].copy(); bad[10, 1] = -1
    refused("feature index", m=bad)
    bad = matches[:50].copy(); bad[49, 2] = 1
    refused("view 1", m=bad)
    k1 = kf1.kps_un.copy(); k1["octave"] = 8
    refused("octave 8", k1=k1)
    c = np.array([cam2]); c["nlevels"] = 17
    refused("nlevels=17", cams2=c)
    refused("array lengths", off2=[0, len(kf2) - 1])
    check(matcher, cam1, kf1, [cam2], [0, len(kf2)], kf2, matches[:50])          # the handle is still good
