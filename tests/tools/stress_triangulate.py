#!/usr/bin/env python3
"""Randomised GPU-vs-restatement sweep of the CreateNewMapPoints per-match loop (orbm_triangulate_matches,
src/LocalMapping.cc:288-434): random match counts, stereo shares of either key frame, baselines from centimetres to metres, depth
ranges, pixel noise, outlier shares, octave consistency, a second key frame with another mbf, one to four second views in a call,
the host-array and the device-pointer entry point, fresh and reused handles.  Every call must give the restatement's
(tests/triangulation_oracle.py) status for every match and its x3D bit for bit; the first call that does not is written to
profiles/stress_triangulate_fail.npz and the tool stops.
usage: stress_triangulate.py [seconds] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import conftest  # noqa
import triangulation_oracle as T
import my_slam_amd as M

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t0 = time.time()
n_calls = n_device = n_multi = 0
by_status = np.zeros(13, np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


m = M.ORBmatcher()
while time.time() - t0 < budget:
    nviews = int(rng.choice([1, 1, 1, 2, 4]))
    n = int(rng.choice([1, 30, 64, 65, 300, 1000, 3000]))
    kw = dict(stereo1=float(rng.choice([0, 0.5, 1])), baseline=float(10 ** rng.uniform(-2, 0.9)), noise=float(rng.choice([0.0, 0.7, 2.0])),
              outliers=float(rng.choice([0, 0.1, 0.5])), consistent_octaves=float(rng.choice([0.3, 0.8, 1.0])),
              depth=(float(rng.choice([0.5, 2.0])), float(rng.choice([10.0, 40.0, 200.0]))), bad_depth=float(rng.choice([0, 0.02, 0.2])))
    pairs = [T.make_pair(np.random.default_rng(int(rng.integers(1 << 30))), n, stereo2=float(rng.choice([0, 0.5, 1])),
                         mbf2=float(rng.choice([T.KITTI["mbf"], 200.0])), **kw) for _ in range(nviews)]
    cam1, kf1 = pairs[0][0], pairs[0][1]
    # every pair was drawn with its own first key frame: the matches of views >= 1 meet key frame 1's features as outliers do
    off2, kf2 = T.concat_keyframes([p[3] for p in pairs])
    cams2 = np.array([p[2] for p in pairs])
    matches = np.concatenate([np.concatenate([p[4][:, :2], np.full((n, 1), v, np.int32)], 1) for v, p in enumerate(pairs)])
    matches = matches[rng.permutation(len(matches))]
    if rng.integers(0, 8) == 0:
        m.close(); m = M.ORBmatcher(max_queries=64, max_train=64, max_pairs=64)
    est, ex = T.triangulate(cam1, kf1, cams2, off2, kf2, matches)
    if rng.integers(0, 3) == 0:
        d = [dev(np.asarray(cam1, M.CAM_DTYPE).reshape(1)), dev(kf1.kps_un), dev(kf1.keys_xy), dev(kf1.u_right), dev(kf1.depth), dev(cams2),
             dev(off2), dev(kf2.kps_un), dev(kf2.keys_xy), dev(kf2.u_right), dev(kf2.depth), dev(matches)]
        d_st = torch.full((len(matches),), 99, dtype=torch.uint8, device="cuda"); d_x = torch.full((len(matches), 3), -7.0, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        m.triangulate_matches_device(*[t.data_ptr() for t in d[:5]], len(kf1), d[5].data_ptr(), nviews, *[t.data_ptr() for t in d[6:]],
                                     len(matches), d_st.data_ptr(), d_x.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        st, x = d_st.cpu().numpy(), d_x.cpu().numpy()
        n_device += 1
    else:
        st, x = m.triangulate_matches(cam1, kf1.kps_un, kf1.keys_xy, kf1.u_right, kf1.depth, cams2, off2, kf2.kps_un, kf2.keys_xy,
                                      kf2.u_right, kf2.depth, matches)
    if not (np.array_equal(st, est) and np.array_equal(x.view(np.uint32), ex.view(np.uint32))):
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        np.savez(os.path.join(ROOT, "profiles", "stress_triangulate_fail.npz"), cam1=cam1, cams2=cams2, off2=off2, k1=kf1.kps_un, x1=kf1.keys_xy,
                 u1=kf1.u_right, d1=kf1.depth, k2=kf2.kps_un, x2=kf2.keys_xy, u2=kf2.u_right, d2=kf2.depth, matches=matches, st=st, x=x, est=est, ex=ex)
        bad = np.nonzero((st != est) | (x.view(np.uint32) != ex.view(np.uint32)).any(1))[0]
        print("stress_triangulate: MISMATCH in call %d (%s, %d views): %d matches, first %d: got %d %s, expected %d %s"
              % (n_calls, kw, nviews, len(bad), bad[0], st[bad[0]], x[bad[0]], est[bad[0]], ex[bad[0]]))
        sys.exit(1)
    n_calls += 1; n_multi += nviews > 1
    by_status += np.bincount(est, minlength=13)
print("stress_triangulate: %d random calls (%d through the device-pointer entry point, %d with several second views), %d matches identical "
      "to the restatement in status and x3D bits in %.0f s, 0 mismatches; matches per status %s"
      % (n_calls, n_device, n_multi, by_status.sum(), time.time() - t0,
         ", ".join("%s %d" % (T.STATUS_NAMES[c], by_status[c]) for c in range(12))))
