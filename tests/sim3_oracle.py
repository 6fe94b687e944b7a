"""fp64 restatement of Sim3Solver (src/Sim3Solver.cc of the reference) in numpy: Horn's closed form with the Rodrigues
round trip of ComputeSim3 (:226-337), CheckInliers / Project (:340-403) with the integer-truncated thresholds of
include/Sim3Solver.h:78-79, SetRansacParameters (:114-138) and the iterate state machine (:140-207).  Everything is
double precision and uses numpy's eigh / libm: it is what the float path of the library is measured against."""
import math

import numpy as np


def max_error(sigma2):
    """mvnMaxError: std::vector<size_t>::push_back(9.210 * sigmaSquare) -- the double product truncated to an integer"""
    return float(int(9.210 * float(np.float32(sigma2))))


def rodrigues(rv):
    th = float(np.linalg.norm(rv))
    if th < 2.220446049250313e-16:
        return np.eye(3)
    r = np.asarray(rv, np.float64) / th
    rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    return math.cos(th) * np.eye(3) + (1 - math.cos(th)) * np.outer(r, r) + math.sin(th) * rx


def compute_sim3(P1, P2, fix_scale):
    """P1 / P2: the three sampled points in camera 1 / 2 as rows -> (s12, R12, t12)"""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(0), P2.mean(0)
    Pr1, Pr2 = (P1 - O1).T, (P2 - O2).T
    M = Pr2 @ Pr1.T
    N11 = M[0, 0] + M[1, 1] + M[2, 2]; N12 = M[1, 2] - M[2, 1]; N13 = M[2, 0] - M[0, 2]; N14 = M[0, 1] - M[1, 0]
    N22 = M[0, 0] - M[1, 1] - M[2, 2]; N23 = M[0, 1] + M[1, 0]; N24 = M[2, 0] + M[0, 2]
    N33 = -M[0, 0] + M[1, 1] - M[2, 2]; N34 = M[1, 2] + M[2, 1]
    N44 = -M[0, 0] - M[1, 1] + M[2, 2]
    N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]])
    w, v = np.linalg.eigh(N)
    q = v[:, np.argmax(w)]
    vec = q[1:]
    nrm = float(np.linalg.norm(vec))
    ang = math.atan2(nrm, q[0])
    R = rodrigues(2 * ang * vec / nrm)
    P3 = R @ Pr2
    s = float((Pr1 * P3).sum() / (P3 * P3).sum()) if not fix_scale else 1.0
    t = O1 - s * (R @ O2)
    return s, R, t


def project(x, K):
    return np.stack([K[0] * x[:, 0] / x[:, 2] + K[2], K[1] * x[:, 1] / x[:, 2] + K[3]], 1)


def errors(s, R, t, x1, x2, K1, K2):
    """err1, err2 of every correspondence (CheckInliers): squared pixel distances in image 1 and image 2"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    x2in1 = s * (x2 @ R.T) + t
    x1in2 = ((x1 - t) @ R) / s
    d1 = project(x1, K1) - project(x2in1, K1)
    d2 = project(x1in2, K2) - project(x2, K2)
    return (d1 * d1).sum(1), (d2 * d2).sum(1)


def check_inliers(s, R, t, x1, x2, K1, K2, e1, e2):
    err1, err2 = errors(s, R, t, x1, x2, K1, K2)
    return (err1 < e1) & (err2 < e2)


def ransac_epsilon(N, min_inliers):
    """float epsilon = (float)mRansacMinInliers / N (:125), for N > 0"""
    return np.float32(min_inliers) / np.float32(N)


def ransac_iterations(N, probability, min_inliers, max_iterations):
    """mRansacMaxIts after SetRansacParameters; N < minInliers is defined as one iteration (include/orbp.h)"""
    if min_inliers >= N:
        nit = 1
    else:
        eps = float(ransac_epsilon(N, min_inliers))
        den = math.log(1 - eps ** 3) if eps ** 3 < 1 else float("nan")
        v = float("nan") if den == 0 or den != den else math.ceil(math.log(1 - probability) / den)
        # a double beyond int's range converts to INT_MIN in the reference's x86 build (cvttsd2si), which the clamp turns into 1
        nit = int(v) if -2.0 ** 31 <= v <= 2.0 ** 31 - 1 else -2 ** 31
    return max(1, min(nit, max_iterations))


def draw_triple(N, rand, rand_max):
    """:163-177 -- RandomInt(0, size - 1), swap with back, pop"""
    avail, tri = list(range(N)), []
    for _ in range(3):
        r = int((rand() / (rand_max + 1.0)) * len(avail))
        tri.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return tri


class Solver:
    """The state machine of Sim3Solver::iterate over the fp64 hypothesis"""

    def __init__(self, x1, x2, sigma2_1, sigma2_2, K1, K2, fix_scale, rand, rand_max):
        self.x1, self.x2 = np.asarray(x1, np.float64).reshape(-1, 3), np.asarray(x2, np.float64).reshape(-1, 3)
        self.e1 = np.array([max_error(v) for v in sigma2_1], np.float64)
        self.e2 = np.array([max_error(v) for v in sigma2_2], np.float64)
        self.K1, self.K2, self.fix, self.rand, self.rand_max = K1, K2, fix_scale, rand, rand_max
        self.N = len(self.x1)
        self.n_best, self.best = 0, None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.min_inliers = minInliers
        self.max_its = ransac_iterations(self.N, probability, minInliers, maxIterations)
        self.n_iter = 0

    def hypothesis(self, tri):
        s, R, t = compute_sim3(self.x1[tri], self.x2[tri], self.fix)
        return s, R, t, check_inliers(s, R, t, self.x1, self.x2, self.K1, self.K2, self.e1, self.e2)

    def iterate(self, n_iterations):
        """-> (T12 4x4 or None, no_more, flags, n_inliers), with include/orbp.h's two definitions: N < minInliers (or N < 3) sets
        no_more at once, and no_more is also set on a call that returns a pose at mRansacMaxIts"""
        flags = np.zeros(self.N, bool)
        if self.N < self.min_inliers or self.N < 3:
            return None, True, flags, 0
        cur = 0
        while self.n_iter < self.max_its and cur < n_iterations:
            cur += 1
            self.n_iter += 1
            tri = draw_triple(self.N, self.rand, self.rand_max)
            s, R, t, inl = self.hypothesis(tri)
            n = int(inl.sum())
            if n >= self.n_best:
                self.n_best, self.best = n, (s, R, t)
                if n > self.min_inliers:
                    T = np.eye(4)
                    T[:3, :3], T[:3, 3] = s * R, t
                    return T, self.n_iter >= self.max_its, inl, n
        return None, self.n_iter >= self.max_its, flags, 0
