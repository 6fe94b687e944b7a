"""orbm_frustum / orbm_frustum_device / orbm_search_local_points, orbm_distinctive_descriptors[_device] and
orbm_triangulate_matches[_device] on the GPU against the reference's own records (tests/golden/mapping/, made by
oracle/_ref/ref_mapping from the reference's own src/MapPoint.cc, Frame::isInFrustum and LocalMapping::CreateNewMapPoints), with no
step through the numpy restatements: what is compared and how is ref_mapping.frustum_check, dd_check and tri_check, the same
functions tests/test_reference_pin_mapping_cpu.py holds the restatements to.  Where the binaries are present the records are taken
from a fresh run of them, which must equal the fixtures.

The whole loop: orbm_create_new_map_points against the list of new MapPoints that the reference's own loop, with its own
SearchForTriangulation, made (tests/golden/mapping/loop.npz).

Of a refused pair the reference shows only that it was refused, so the library's status of a refused pair is not compared; accepted
or not, the UnprojectStereo path and the feature-without-depth status are."""
import numpy as np
import pytest

import frustum_oracle as fo
import ref_mapping as rm

pytestmark = pytest.mark.gpu
FIXTURES = rm.load_fixtures()
TOL = rm.load_tolerance()
FRUSTUM = sorted(n for k, n in FIXTURES if k == "frustum")
TRI = sorted(n for k, n in FIXTURES if k == "newpoints")
GUARD = 24          # elements of padding on either side of every device array


@pytest.fixture(scope="module")
def m(orbx):
    h = orbx.ORBmatcher(0.8, True, max_queries=8192, max_train=8192, max_pairs=1 << 21)
    yield h
    h.close()


@pytest.fixture(scope="module")
def records():
    """{(kind, name): fixture} with the response of a fresh run where the binaries are present"""
    if not rm.ensure(allow_build=False, variants=("",)):
        return FIXTURES
    keys = sorted(FIXTURES)
    res = rm.run_many([(FIXTURES[k]["req"], "") for k in keys])
    for k, (rc, data, err) in zip(keys, res):
        assert rc == 0 and data == FIXTURES[k]["rsp"], (k, err)
    return FIXTURES


class Padded:
    """device arrays inside larger buffers: GUARD elements of a sentinel before and after, which no call may touch"""

    def __init__(self):
        import torch
        self.torch = torch
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        raw = a.view(np.uint8).reshape(-1)
        item = max(a.dtype.itemsize, 4)
        host = np.full(len(raw) + 2 * GUARD * item, 0xA5, np.uint8)
        host[GUARD * item:GUARD * item + len(raw)] = raw
        d = self.torch.from_numpy(host).cuda()
        self.bufs.append((d, GUARD * item, len(raw), a.dtype, a.shape))
        return d.data_ptr() + GUARD * item

    def out(self, n, dtype):
        return self.put(np.full(n, 0x5A, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype))

    def get(self, k):
        d, off, nbytes, dtype, shape = self.bufs[k]
        host = d.cpu().numpy()
        assert (host[:off] == 0xA5).all() and (host[off + nbytes:] == 0xA5).all(), "a guard element was written"
        return host[off:off + nbytes].view(dtype).reshape(shape)


# ---- Frame::isInFrustum

@pytest.mark.parametrize("name", FRUSTUM)
def test_frustum_equals_the_reference(m, records, name):
    fx = records[("frustum", name)]
    sc, limit = rm.frustum_scene(rm.Records(fx["full"]))
    got = m.frustum(*sc.args(), limit)
    rm.frustum_check(fx, got, name)
    out = got[0] != fo.IN_VIEW
    assert not (got[1][out].any() or got[2][out].any() or got[3][out].any() or got[4][out].any() or got[5][out].any())


def test_frustum_device_on_padded_buffers_equals_the_reference(m, records):
    import torch
    for name in FRUSTUM:
        fx = records[("frustum", name)]
        sc, limit = rm.frustum_scene(rm.Records(fx["full"]))
        n = len(sc)
        if n == 0:
            m.frustum_device(None, 0, *([None] * 5), limit, *([None] * 6))
            continue
        p = Padded()
        ins = [p.put(a) for a in (np.array([sc.view]), sc.skip, sc.xw, sc.normal, sc.mf_max, sc.mf_min)]
        outs = [p.out(n, t) for t in (np.uint8, np.float32, np.float32, np.float32, np.int32, np.float32)]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        m.frustum_device(ins[0], n, *ins[1:], limit, *outs, stream.cuda_stream)
        stream.synchronize()
        got = [p.get(6 + k) for k in range(6)]
        for k in range(6):
            p.get(k)
        rm.frustum_check(fx, tuple(got) + (int((got[0] == fo.IN_VIEW).sum()),), name)


@pytest.mark.parametrize("name,th", [("scene: stereo n=65", 3.0), ("scene: mono n=64", 3.0), ("scene: stereo n=63", 1.0),
                                      ("gates: stereo 12 levels, limit 0.9", 5.0), ("gates: mono, limit 0.9", 3.0),
                                      ("gates: degenerate distances", 3.0), ("gates: mfLogScaleFactor = 0", 3.0)])
def test_search_local_points_equals_the_reference_and_the_pinned_search(m, records, name, th):
    """the frustum half against the records; the matches against orbm_search_by_projection_map (pinned to the reference's
    src/ORBmatcher.cc by tests/test_reference_pin_matcher_gpu.py) fed the reference's recorded projections"""
    fx = records[("frustum", name)]
    sc, limit = rm.frustum_scene(rm.Records(fx["full"]))
    rsp, d = rm.Records(fx["rsp"]), ~fx["undef"]
    fr = fo.make_frame(np.random.default_rng(len(name)), sc, n_clutter=150)
    stereo = bool(sc.view["mbf"] > 0)
    full = {}
    for tag, dt in (("flag", np.uint8), ("projx", np.float32), ("projy", np.float32), ("projxr", np.float32), ("level", np.int32), ("viewcos", np.float32)):
        full[tag] = np.zeros(len(sc), dt)
        full[tag][d] = rsp.one(tag).reshape(-1)
    b = tuple(float(x) for x in sc.view["bounds"])
    want_cur = fr.cur_obs.copy()
    m.grid_build(fr.kps, *b)
    want_cm, want_nm = m.SearchByProjectionMap(full["flag"], full["projx"], full["projy"], full["level"], full["viewcos"], fr.mp_desc, fr.mp_obs,
                                               sc.view["scale_factors"][:int(sc.view["nlevels"])], fr.kps, fr.desc, want_cur, th,
                                               full["projxr"] if stereo else None, fr.u_right if stereo else None) if full["flag"].any() \
        else (np.full(len(fr.kps), -1, np.int32), 0)
    cur = fr.cur_obs.copy()
    m.grid_build(fr.kps, *b)
    out = m.search_local_points(*sc.args(), fr.mp_desc, fr.mp_obs, fr.kps, fr.desc, cur, th, fr.u_right if stereo else None, limit)
    rm.frustum_check(fx, out[:7], name)
    assert out[8] == want_nm and np.array_equal(out[7], want_cm) and np.array_equal(cur, want_cur)
    if name.startswith("scene"):
        assert want_nm >= 5


# ---- MapPoint::ComputeDistinctiveDescriptors

def test_distinctive_descriptors_mixed_batch_and_each_point_alone(m, records):
    fx = records[("mappoint", "batch")]
    req, rsp = rm.Records(fx["req"]), rm.Records(fx["rsp"])
    off, desc = rm.dd_library_input(req)
    best, _ = m.distinctive_descriptors(off, desc)
    rm.dd_check(req, rsp, best)
    assert set(rm.DD_SIZES) <= set(np.diff(off).tolist())
    for p in range(len(off) - 1):                               # alone: the size class decides the kernel
        alone, _ = m.distinctive_descriptors(np.array([0, off[p + 1] - off[p]], np.int32), desc[off[p]:off[p + 1]])
        assert alone[0] == best[p], p
    pts = rm.dd_points()
    for p, (name, rows, kfbad, mpbad, want) in enumerate(pts):
        if want is not None:
            assert best[p] == want, name


def test_distinctive_descriptors_device_form(m, records):
    import torch
    fx = records[("mappoint", "batch")]
    req, rsp = rm.Records(fx["req"]), rm.Records(fx["rsp"])
    off, desc = rm.dd_library_input(req)
    n = len(off) - 1
    p = Padded()
    d_off, d_desc = p.put(off), p.put(desc)
    d_best, d_med = p.out(n, np.int32), p.out(n, np.int32)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m.distinctive_descriptors_device(n, d_off, d_desc, int(off[-1]), int(np.diff(off).max()), d_best, d_med, stream=st.cuda_stream)
    st.synchronize()
    rm.dd_check(req, rsp, p.get(2))
    p.get(0), p.get(1), p.get(3)


# ---- CreateNewMapPoints, pairs given

@pytest.mark.parametrize("name", TRI)
def test_triangulate_matches_equals_the_reference(m, records, name):
    fx = records[("newpoints", name)]
    cam1, kf1, cams2, off2, kf2, pairs = rm.tri_inputs(rm.Records(fx["req"]))
    status, x3d = m.triangulate_matches(cam1, kf1.kps_un, kf1.keys_xy, kf1.u_right, kf1.depth, cams2, off2, kf2.kps_un, kf2.keys_xy, kf2.u_right,
                                        kf2.depth, pairs)
    dev = rm.tri_check(rm.Records(fx["rsp"]), status, x3d, TOL["tolerance"], pairs[:, 2])
    print(name, "x3D deviates %.3g of %.3g" % (dev, TOL["tolerance"]))


def test_triangulate_matches_device_form(m, orbx, records):
    import torch
    for name in TRI:
        fx = records[("newpoints", name)]
        cam1, kf1, cams2, off2, kf2, pairs = rm.tri_inputs(rm.Records(fx["req"]))
        n = len(pairs)
        if n == 0:
            continue
        p = Padded()
        d = [p.put(a) for a in (np.asarray(cam1, orbx.CAM_DTYPE).reshape(1), kf1.kps_un, kf1.keys_xy, kf1.u_right, kf1.depth,
                                np.ascontiguousarray(cams2, orbx.CAM_DTYPE), np.asarray(off2, np.int32), kf2.kps_un, kf2.keys_xy, kf2.u_right,
                                kf2.depth, np.ascontiguousarray(pairs, np.int32))]
        d_st, d_x = p.out(n, np.uint8), p.out(3 * n, np.float32)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        m.triangulate_matches_device(d[0], d[1], d[2], d[3], d[4], len(kf1), d[5], len(cams2), d[6], d[7], d[8], d[9], d[10], d[11], n, d_st, d_x,
                                     stream=st.cuda_stream)
        st.synchronize()
        status, x3d = p.get(12), p.get(13).reshape(-1, 3)
        ok = status <= 2
        rm.tri_check(rm.Records(fx["rsp"]), status, np.where(ok[:, None], x3d, 0), TOL["tolerance"], pairs[:, 2])
        for k in range(12):
            p.get(k)


# ---- CreateNewMapPoints, the whole loop

LOOP = rm.load_loop_fixtures()


@pytest.mark.parametrize("name", sorted(rm.LOOP_CASES))
def test_create_new_map_points_replayed_equals_the_reference_loop(m, name):
    """orbm_create_new_map_points on the neighbours that passed the reference's gates, with the reference's F12; the replay rule of
    include/orbm.h applied to its dense output (the slots of view v in ascending idx1 whose feature holds no MapPoint yet) must give the
    reference's new MapPoints in the reference's order"""
    import newmappoints_batch_oracle as nb
    sc, mono, depths = rm.loop_scene(name)
    fx = LOOP[name]
    assert fx["req"] == rm.loop_requests(sc, mono, depths)[0], name
    s2, live = rm.surviving_scene(sc, rm.Records(fx["gate_rsp"]))
    dense = m.create_new_map_points(*s2.batch_args())
    dev = rm.loop_check(rm.Records(fx["rsp"]), live, nb.replay(s2, dense), TOL["tolerance"])
    print(name, "x3D deviates %.3g of %.3g" % (dev, TOL["tolerance"]))
