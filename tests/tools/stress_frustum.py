#!/usr/bin/env python3
"""Randomised GPU-vs-restatement sweep of Frame::isInFrustum and Tracking::SearchLocalPoints (orbm_frustum, orbm_frustum_device,
orbm_search_local_points; src/Frame.cc:269-325, src/Tracking.cc:1174-1199): random sizes, poses, calibrations, level counts, scale
factors, skip and degenerate shares, viewingCosLimit and th through all three entry points, fresh and reused handles.  Every call
must give the restatement's (tests/frustum_oracle.py) status for every point, its four floats bit for bit (any NaN equals any NaN),
its levels and nToMatch, and the fused call the C oracle's matches on top; the first call that does not is written to
profiles/stress_frustum_fail.npz and the tool stops.  One process.
usage: stress_frustum.py [seconds] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import conftest  # noqa
import frustum_oracle as F
import oracle_lib as O
import my_slam_amd as M

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t0 = time.time()
n_calls = n_device = n_fused = n_matches = 0
by_status = np.zeros(8, np.int64)
CAL = [dict(), dict(W=640, H=480, fx=517.3, fy=516.5, cx=318.6, cy=255.3), dict(W=1920, H=1080, fx=1400.0, fy=1400.0, cx=960.0, cy=540.0)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def bits(a):
    a = np.asarray(a)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)) if a.dtype == np.float32 else a


def same(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got[:6], want[:6]))


def fail(what, sc, got, want):
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    np.savez(os.path.join(ROOT, "profiles", "stress_frustum_fail.npz"), view=sc.view, skip=sc.skip, xw=sc.xw, normal=sc.normal, mf_max=sc.mf_max,
             mf_min=sc.mf_min, **{"got%d" % i: np.asarray(g) for i, g in enumerate(got)}, **{"want%d" % i: np.asarray(w) for i, w in enumerate(want)})
    print("stress_frustum: MISMATCH in call %d (%s)" % (n_calls, what))
    sys.exit(1)


m = M.ORBmatcher(0.8)
while time.time() - t0 < budget:
    n = int(rng.choice([1, 30, 63, 64, 65, 300, 1000, 3000, 5000, 12000]))
    nlevels = int(rng.choice([1, 4, 8, 12, 16]))
    kw = dict(stereo=bool(rng.integers(0, 2)), scale_factor=float(rng.choice([1.0, 1.1, 1.2, 1.44, 2.0])) if nlevels > 1 else 1.2, nlevels=nlevels,
              skip_share=float(rng.choice([0, 0.1, 0.5, 1.0])), wild_share=float(rng.choice([0, 0.2, 0.6])),
              degenerate_share=float(rng.choice([0, 0.02, 0.2])), turn=float(rng.choice([0, 0, 0.4, 1.5, 3.1])), **CAL[int(rng.integers(0, 3))])
    sc = F.make_scene(np.random.default_rng(int(rng.integers(1 << 30))), n, **kw)
    limit = float(rng.choice([0.5, 0.5, 0.0, 0.9]))
    want = F.frustum(*sc.args(), limit)
    if rng.integers(0, 8) == 0:
        m.close(); m = M.ORBmatcher(0.8, max_queries=64, max_train=64, max_pairs=64)
    kind = int(rng.integers(0, 3))
    if kind == 0:
        got = m.frustum(*sc.args(), limit)
        if not same(got, want) or got[6] != want[6]:
            fail("orbm_frustum %s" % kw, sc, got, want)
    elif kind == 1:
        d = [dev(np.array([sc.view])), dev(sc.skip), dev(sc.xw), dev(sc.normal), dev(sc.mf_max), dev(sc.mf_min)]
        o = [torch.full((n,), 99, dtype=torch.uint8, device="cuda")] + [torch.full((n,), -7.0, device="cuda") for _ in range(3)] + \
            [torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7.0, device="cuda")]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        m.frustum_device(d[0].data_ptr(), n, *[t.data_ptr() for t in d[1:]], limit, *[t.data_ptr() for t in o], stream=s.cuda_stream)
        s.synchronize()
        got = [t.cpu().numpy() for t in o]
        if not same(got, want):
            fail("orbm_frustum_device %s" % kw, sc, got, want)
        n_device += 1
    else:
        fr = F.make_frame(np.random.default_rng(int(rng.integers(1 << 30))), sc, n_clutter=int(rng.choice([0, 50, 600])),
                          occupied_share=float(rng.choice([0, 0.15, 0.6])))
        th = float(rng.choice([1.0, 3.0, 5.0]))
        stereo = sc.view["mbf"] > 0
        bounds = tuple(float(b) for b in sc.view["bounds"])
        sf = sc.view["scale_factors"][:nlevels]
        wcur, wcm, wnm = fr.cur_obs.copy(), np.full(len(fr.kps), -1, np.int32), 0
        if want[6] > 0 and len(fr.kps) > 0:
            og = O.FrameGrid(fr.kps, *bounds)
            wcm, wnm = O.search_by_projection_map((want[0] == F.IN_VIEW).astype(np.uint8), want[1], want[2], want[4], want[5], fr.mp_desc, fr.mp_obs,
                                                  sf, og, fr.desc, wcur, th, 0.8, want[3] if stereo else None, fr.u_right if stereo else None)
        cur = fr.cur_obs.copy()
        if len(fr.kps) > 0:
            m.grid_build(fr.kps, *bounds)
        got = m.search_local_points(*sc.args(), fr.mp_desc, fr.mp_obs, fr.kps, fr.desc, cur, th, fr.u_right if stereo else None, limit)
        if not same(got, want) or got[6] != want[6] or got[8] != wnm or not np.array_equal(got[7], wcm) or not np.array_equal(cur, wcur):
            fail("orbm_search_local_points %s th=%g" % (kw, th), sc, got, want + (wcm, wnm))
        n_fused += 1; n_matches += wnm
    n_calls += 1
    by_status += np.bincount(want[0], minlength=8)
print("stress_frustum: %d random calls (%d through the device-pointer entry point, %d through orbm_search_local_points with %d matches), "
      "%d points identical to the restatement in status, float bits, level and nToMatch in %.0f s, 0 mismatches; points per status %s"
      % (n_calls, n_device, n_fused, n_matches, by_status.sum(), time.time() - t0,
         ", ".join("%s %d" % (F.STATUS_NAMES[c], by_status[c]) for c in range(8))))
