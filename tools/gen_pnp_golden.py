"""Records tests/golden/pnp/epnp_parent.npz: the bytes orbp_epnp and orbp_pnp_iterate produce.

MEANT TO BE RUN AT THE PARENT COMMIT of the change that moved EPnP's arithmetic from csrc/orbp.cc into csrc/orbp_epnp_body.h
(git checkout <that commit>^ -- my-slam_amd/csrc/orbp.cc, or a worktree of it): the file pins that refactor, so regenerating it
from a later orbp.cc records whatever that orbp.cc computes and pins nothing.  tests/test_pnp_batch_cpu.py compares the current
library with these bytes using == on the raw bytes.

The script builds orbp.cc alone with g++ (the host flags of my-slam_amd/Makefile) into a temporary shared object, so it needs
neither hipcc nor a GPU, and stores inputs next to outputs so that the test does not depend on numpy's generators:
  epnp_<k>_{pws,us,K}  ->  epnp_<k>_{R,t,err}      n = 4, 5, 6, 8, 12, 50, exact and noisy; epnp_coplanar4_*: four points of the
                                                    world plane z = 0, whose cross-covariance has an exactly zero column, so
                                                    estimate_R_and_t takes its rank-deficient branch
  tr<k>_{p2d,sigma2,p3d,K,params,seed}  ->  tr<k>_{ret,no_more,n_inliers,iterations,masks,T}
                                                    iterate(5) until bNoMore under the Lcg of tests/test_pose.py, iterating on
                                                    after a returned pose

usage: python tools/gen_pnp_golden.py [--src my-slam_amd/csrc/orbp.cc] [--out tests/golden/pnp/epnp_parent.npz]
"""
import argparse
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, FY, CX, CY = 718.856, 718.856, 607.1928, 185.2157
SIGMA2 = (1.2 ** np.arange(8)) ** 2
RAND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
LCG_MAX = 2147483647


class Lcg:
    def __init__(self, seed):
        self.s = seed

    def __call__(self):
        self.s = (self.s * 1103515245 + 12345) & 0x7FFFFFFF
        return self.s


def scene(rng, n, noise=0.0, n_wrong=0, planar=False):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0, 0.5)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
    t = rng.uniform(-1, 1, 3)
    if planar:
        pw = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2, 2, n), np.zeros(n)], 1)
        t = t + np.array([0, 0, 10.0])
        pc = pw @ R.T + t
    else:
        pc = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2, 2, n), rng.uniform(4, 20, n)], 1)
        pw = (pc - t) @ R
    u = np.stack([FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY], 1) + rng.normal(size=(n, 2)) * noise
    if n_wrong:
        u[:n_wrong] += rng.uniform(30, 80, (n_wrong, 2)) * rng.choice([-1, 1], (n_wrong, 2))
    return np.ascontiguousarray(pw), np.ascontiguousarray(u)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def load(src, tmp):
    so = os.path.join(tmp, "orbp_parent.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", src, "-o", so])
    L = C.CDLL(so)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.orbp_epnp.argtypes = [C.c_int, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp]
    L.orbp_epnp.restype = C.c_double
    L.orbp_pnp_create.argtypes = [C.POINTER(vp), C.c_int, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float]
    L.orbp_pnp_destroy.argtypes = [vp]
    L.orbp_pnp_destroy.restype = None
    L.orbp_pnp_set_rand.argtypes = [vp, RAND_FN, vp, C.c_int]
    L.orbp_pnp_set_rand.restype = None
    L.orbp_pnp_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    L.orbp_pnp_get_ransac_state.argtypes = [vp, ip, ip, C.POINTER(C.c_float), ip]
    L.orbp_pnp_get_ransac_state.restype = None
    L.orbp_pnp_iterate.argtypes = [vp, C.c_int, ip, vp, ip, vp]
    return L


def epnp_cases():
    rng = np.random.default_rng(20261)
    out = []
    for n in (4, 5, 6, 8, 12, 50):
        for noise in (0.0, 0.6):
            out.append(("n%d_%s" % (n, "noisy" if noise else "exact"),) + scene(rng, n, noise))
    out.append(("coplanar4",) + scene(rng, 4, 0.0, planar=True))
    return out


# (N, wrong matches, min_set, min_inliers, max_iterations, Lcg seed, generator seed)
TRANSCRIPTS = ((60, 24, 4, 10, 300, 42, 911), (150, 60, 6, 10, 300, 7, 912), (60, 24, 4, 33, 300, 5, 913))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "my-slam_amd", "csrc", "orbp.cc"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pnp", "epnp_parent.npz"))
    a = ap.parse_args()
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = load(a.src, tmp)
        names = []
        for name, pw, u in epnp_cases():
            R, t = np.zeros(9), np.zeros(3)
            err = L.orbp_epnp(len(pw), p(pw), p(u), FX, FY, CX, CY, p(R), p(t))
            assert err >= 0
            names.append(name)
            data.update({"epnp_%s_pws" % name: pw, "epnp_%s_us" % name: u, "epnp_%s_K" % name: np.array([FX, FY, CX, CY]),
                         "epnp_%s_R" % name: R, "epnp_%s_t" % name: t, "epnp_%s_err" % name: np.array([err])})
        data["epnp_names"] = np.array(names)
        for k, (N, n_wrong, min_set, min_inl, max_its, lseed, gseed) in enumerate(TRANSCRIPTS):
            rng = np.random.default_rng(gseed)
            pw, u = scene(rng, N, 0.5, n_wrong)
            p2d, p3d = u.astype(np.float32), pw.astype(np.float32)
            s2 = SIGMA2[rng.integers(0, 8, N)].astype(np.float32)
            K = np.array([FX, FY, CX, CY], np.float32)
            h = C.c_void_p()
            assert L.orbp_pnp_create(C.byref(h), N, p(p2d), p(s2), p(p3d), *[float(v) for v in K]) == 0
            lcg = Lcg(lseed)
            cb = RAND_FN(lambda ctx: lcg())
            L.orbp_pnp_set_rand(h, cb, None, LCG_MAX)
            assert L.orbp_pnp_set_ransac_parameters(h, 0.99, min_inl, max_its, min_set, 0.5, 5.991) == 0
            ret, nm, ninl, its, masks, Ts = [], [], [], [], [], []
            for call in range(200):
                no_more, n, it = C.c_int(), C.c_int(), C.c_int()
                inl, T = np.zeros(N, np.uint8), np.zeros(16, np.float32)
                r = L.orbp_pnp_iterate(h, 5, C.byref(no_more), p(inl), C.byref(n), p(T))
                L.orbp_pnp_get_ransac_state(h, None, None, None, C.byref(it))
                ret.append(r); nm.append(no_more.value); ninl.append(n.value); its.append(it.value); masks.append(inl); Ts.append(T)
                if no_more.value:
                    break
            assert nm[-1], "transcript %d does not end" % k
            L.orbp_pnp_destroy(h)
            data.update({"tr%d_p2d" % k: p2d, "tr%d_sigma2" % k: s2, "tr%d_p3d" % k: p3d, "tr%d_K" % k: K,
                         "tr%d_params" % k: np.array([0.99, min_inl, max_its, min_set, 0.5, 5.991]), "tr%d_seed" % k: np.array([lseed]),
                         "tr%d_ret" % k: np.array(ret, np.int32), "tr%d_no_more" % k: np.array(nm, np.int32),
                         "tr%d_n_inliers" % k: np.array(ninl, np.int32), "tr%d_iterations" % k: np.array(its, np.int32),
                         "tr%d_masks" % k: np.stack(masks), "tr%d_T" % k: np.stack(Ts)})
            print("transcript %d: %d calls, poses returned on %s" % (k, len(ret), [i for i, r in enumerate(ret) if r]))
        data["n_transcripts"] = np.array([len(TRANSCRIPTS)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **data)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
