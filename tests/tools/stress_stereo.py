#!/usr/bin/env python3
"""Randomised GPU-vs-oracle sweep of Frame::ComputeStereoMatches (k_stereo + the host median cull): random image sizes,
pyramids, feature counts and FAST thresholds per side, rigs (maxD from 20 to 2000 px), scenes (tests/stereo_cases.py
stereo_scene) and subsets / permutations of the right keypoints; mvuRight and mvDepth must be bit-identical.
usage: stress_stereo.py [seconds] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa
import conftest  # noqa
import oracle_lib as O
import ref_pin as R
import stereo_cases as S
import my_slam_amd as M

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t0 = time.time(); n_ok = 0; nm_tot = 0; n_sub = 0
while time.time() - t0 < budget:
    W, H = int(rng.integers(160, 1400)), int(rng.integers(120, 800))
    sf = float(rng.choice([1.1, 1.2, 1.2, 1.5, 2.0])); nl = int(rng.integers(1, 9))
    while nl > 1 and R.undefined_levels(W, H, sf, nl):
        nl -= 1
    if R.undefined_levels(W, H, sf, nl):
        continue
    left, right, _ = S.stereo_scene(int(rng.integers(1, 1 << 30)), W, H, max_disp=int(rng.integers(4, 80)), noise=int(rng.integers(0, 4)))
    nfL, nfR = int(rng.choice([50, 300, 1000, 2000, 4000])), int(rng.choice([50, 300, 1000, 2000, 4000]))
    thR = (int(rng.integers(8, 30)), int(rng.integers(3, 8)))
    try:
        exL = M.ORBextractor(nfL, sf, nl, max_width=W, max_height=H)
        exR = M.ORBextractor(nfR, sf, nl, thR[0], thR[1], max_width=W, max_height=H)
        kl, dl = exL(left); kr, dr = exR(right)
    except M.OrbxError:
        continue
    if len(kr) and rng.random() < 0.4:
        sel = rng.choice(len(kr), int(rng.integers(1, len(kr) + 1)), replace=False)
        kr, dr = kr[sel], dr[sel]; n_sub += 1
    mb, mbf = S.rig(float(rng.choice([20.0, 40.0, 300.0, 500.0, 718.0, 2000.0])), float(rng.uniform(0.05, 0.6)))
    u, d = M.ComputeStereoMatches(exL, exR, kl, dl, kr, dr, mb, mbf)
    ex = O.Extractor(500, sf, nl)
    ou, od = O.stereo_matches(ex, kl, dl, kr, dr, ex.pyramid(left), ex.pyramid(right), mb, mbf)
    if u.tobytes() != ou.tobytes() or d.tobytes() != od.tobytes():
        print("MISMATCH", dict(W=W, H=H, sf=sf, nl=nl, nfL=nfL, nfR=nfR, thR=thR, mb=mb, mbf=mbf, nl_kps=len(kl), nr_kps=len(kr)))
        sys.exit(1)
    n_ok += 1; nm_tot += int((u >= 0).sum())
    exL.close(); exR.close()
print("stress_stereo: %d random cases identical to the oracle in %.0f s (%d matches in total, %d cases with a subset / permutation of the right keypoints)"
      % (n_ok, time.time() - t0, nm_tot, n_sub))
