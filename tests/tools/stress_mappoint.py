#!/usr/bin/env python3
"""Randomised GPU-vs-restatement sweep of the batched MapPoint::ComputeDistinctiveDescriptors (orbm_distinctive_descriptors,
src/MapPoint.cc:242-307): random batch sizes, run-length distributions (key-frame shaped, all short, uniform over a range that
crosses every size class, a few very long runs, empty runs mixed in), near-duplicate and uniformly random descriptors, the
host-pointer and the device-pointer entry point, fresh and reused handles.  Every batch must give the restatement's
(tests/mappoint_oracle.py) index and median for every point; the first batch that does not is written to
profiles/stress_mappoint_fail.npz (off, desc, got and expected) and the tool stops.
usage: stress_mappoint.py [seconds] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import conftest  # noqa
import mappoint_oracle as MO
import my_slam_amd as M

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t0 = time.time()
n_batches = n_points = n_rows = n_device = 0
by_class = np.zeros(5, np.int64)                      # N <= 2, <= 16, <= 64, <= 256, beyond
m = M.ORBmatcher()
while time.time() - t0 < budget:
    shape = int(rng.integers(0, 6))
    npts = int(rng.choice([1, 7, 100, 500, 2000]))
    if shape == 0:
        lengths = MO.run_lengths_keyframe(rng, npts)
    elif shape == 1:
        lengths = rng.integers(0, 4, npts)
    elif shape == 2:
        lengths = rng.integers(0, int(rng.choice([18, 70, 270])), min(npts, 500))
    elif shape == 3:
        lengths = np.concatenate([rng.integers(0, 12, min(npts, 100)), rng.integers(250, 1800, int(rng.integers(1, 4)))])
        rng.shuffle(lengths)
    elif shape == 4:
        lengths = rng.choice([1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 258], min(npts, 100))
    else:
        lengths = MO.run_lengths_keyframe(rng, npts, tail=(17, 1200), tail_share=0.01)
        lengths[rng.random(len(lengths)) < 0.1] = 0
    flips = [None, 1, 3, 6, 12][int(rng.integers(0, 5))]
    off, desc = MO.batch_from_lengths(rng, lengths, flips=flips)
    if rng.integers(0, 8) == 0:
        m.close(); m = M.ORBmatcher()
    if rng.integers(0, 3) == 0 and len(desc) > 0:
        d_off, d_desc = torch.from_numpy(off).cuda(), torch.from_numpy(desc).cuda()
        d_best = torch.full((len(lengths),), -7, dtype=torch.int32, device="cuda"); d_med = d_best.clone()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        m.distinctive_descriptors_device(len(lengths), d_off.data_ptr(), d_desc.data_ptr(), int(off[-1]),
                                         int(lengths.max()) + int(rng.integers(0, 2)) * 300 if int(off[-1]) >= int(lengths.max()) + 300 else int(lengths.max()),
                                         d_best.data_ptr(), d_med.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        best, med = d_best.cpu().numpy(), d_med.cpu().numpy()
        n_device += 1
    else:
        best, med = m.distinctive_descriptors(off, desc)
    eb, em = MO.distinctive_descriptors(off, desc)
    if not (np.array_equal(best, eb) and np.array_equal(med, em)):
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        np.savez(os.path.join(ROOT, "profiles", "stress_mappoint_fail.npz"), off=off, desc=desc, best=best, med=med, eb=eb, em=em)
        bad = np.nonzero((best != eb) | (med != em))[0]
        print("stress_mappoint: MISMATCH in batch %d (shape %d, flips %s): %d points, first %d with N = %d: got %d / %d, expected %d / %d"
              % (n_batches, shape, flips, len(bad), bad[0], lengths[bad[0]], best[bad[0]], med[bad[0]], eb[bad[0]], em[bad[0]]))
        sys.exit(1)
    n_batches += 1; n_points += len(lengths); n_rows += int(off[-1])
    by_class += np.histogram(lengths, bins=[0, 3, 17, 65, 257, 1 << 30])[0]
print("stress_mappoint: %d random batches (%d through the device-pointer entry point), %d MapPoints, %d descriptors identical to the "
      "restatement in index and median in %.0f s, 0 mismatches; points per size class N<=2 / <=16 / <=64 / <=256 / beyond: %s"
      % (n_batches, n_device, n_points, n_rows, time.time() - t0, " / ".join(str(int(c)) for c in by_class)))
