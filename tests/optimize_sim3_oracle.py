"""An independent numpy restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241 of the reference, on g2o), in the
spirit of oracle/pose_oracle.py.  PARITY UNPINNED: g2o needs Eigen, which is not available, so nothing here (nor the product) has
been run against the reference binary; the oracle follows the cited lines, and what it checks is that a second, differently built
restatement of those lines agrees with the product.

What differs from the product (my-slam_amd/csrc/orbp_sim3opt_body.h) on purpose:
  * a rotation is kept as a 3 x 3 matrix where g2o::Sim3 and the product keep a quaternion; Sim3(update) still passes its
    R = I + Omega + Omega^2 (sim3.h:99, 117) through Quaterniond(R) (sim3.h:136), as the reference does, and keeps the matrix of that
    quaternion.  The two agree while the quaternion is a unit one to rounding, which holds when the starting value's is
  * every edge stores its own error (g2o's _error), where the product keeps one estimate for all of them
  * the dense solve is LAPACK's (numpy.linalg.solve), where the product runs its own LDL^T
  * the sums over the edges run over all edges of the graph in one sequence, forward (g2o's edge order: e12 of pair 0, e21 of pair
    0, e12 of pair 1, ...) or reverse; the spread between the two is what tests/tools/measure_sim3opt_spread.py measures

What is kept (each at its line): the numeric Jacobian with delta = 1e-9 scaled by 1 / (2 delta), the vertex pushed, updated and
popped per column, only the Sim3 vertex differentiated (base_binary_edge.hpp:147-196); update[6] = 0 under _fix_scale and
Sim3(update) * estimate without normalisation (types_seven_dof_expmap.h:60-69); the four branches of Sim3(Vector7d) on eps = 1e-5
(sim3.h:70-142); map, inverse, operator* (sim3.h:144-146, 233-236, 266-272); deltaHuber as a float (:1095); the information
(double)(float)invSigma2; chi2() > th2 of a double against a float; a rejected trial's errors staying on the edges; optimize(5), then
optimize(10) when a pair was removed, else optimize(5); a problem without edges optimising nothing; the Levenberg loop of
optimization_algorithm_levenberg.cpp:66-170 with this fork's _nBad stop."""
import math

import numpy as np

DELTA = 1e-9


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def quat_from_R(R):
    """Eigen's Quaterniond(Matrix3d) -> (x, y, z, w)"""
    q = np.zeros(4)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        r = math.sqrt(tr + 1.0)
        q[3] = 0.5 * r
        r = 0.5 / r
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * r, (R[0, 2] - R[2, 0]) * r, (R[1, 0] - R[0, 1]) * r
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        r = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * r
        r = 0.5 / r
        q[3] = (R[k, j] - R[j, k]) * r
        q[j] = (R[j, i] + R[i, j]) * r
        q[k] = (R[k, i] + R[i, k]) * r
    return q


def quat_to_M(q):
    """the linear map of Eigen's Quaterniond * Vector3d, v + w uv + vec x uv with uv = 2 vec x v, as a matrix"""
    V = skew(q[:3])
    return np.eye(3) + 2 * q[3] * V + 2 * (V @ V)


class Sim3:
    def __init__(self, R, t, s):
        self.R, self.t, self.s = np.asarray(R, np.float64), np.asarray(t, np.float64), float(s)

    @staticmethod
    def from_vector8(S12):
        S12 = np.asarray(S12, np.float64)
        return Sim3(quat_to_M(S12[:4]), S12[4:7].copy(), S12[7])

    def vector8(self):
        return np.concatenate([quat_from_R(self.R), self.t, [self.s]])

    @staticmethod
    def exp(u):                                               # sim3.h:70-142
        omega, upsilon, sigma = u[:3], u[3:6], u[6]
        theta = math.sqrt(omega @ omega)
        Om = skew(omega)
        Om2 = Om @ Om
        s = math.exp(sigma)
        I = np.eye(3)
        eps = 0.00001
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B = 1. / 2., 1. / 6.
                R = I + Om + Om2
            else:
                A = (1 - math.cos(theta)) / theta ** 2
                B = (theta - math.sin(theta)) / theta ** 3
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
        else:
            C = (s - 1) / sigma
            if theta < eps:
                A = ((sigma - 1) * s + 1) / sigma ** 2
                B = ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3
                R = I + Om + Om2
            else:
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
                a, b = s * math.sin(theta), s * math.cos(theta)
                c = theta ** 2 + sigma ** 2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
        W = A * Om + B * Om2 + C * I
        return Sim3(quat_to_M(quat_from_R(R)), W @ upsilon, s)      # r = Quaterniond(R) (sim3.h:136)

    def map(self, X):                                         # sim3.h:144-146, X [n, 3]
        return self.s * (X @ self.R.T) + self.t

    def inverse(self):                                        # sim3.h:233-236
        return Sim3(self.R.T, self.R.T @ ((-1. / self.s) * self.t), 1. / self.s)

    def __mul__(self, o):                                     # sim3.h:266-272
        return Sim3(self.R @ o.R, self.s * (self.R @ o.t) + self.t, self.s * o.s)


def ordered_sum(rows, order):
    """the rows added one after another in the given order (numpy's cumsum is sequential; its sum is pairwise)"""
    if len(rows) == 0:
        return np.zeros(rows.shape[1:])
    if order == "reverse":
        rows = rows[::-1]
    return np.cumsum(rows, axis=0)[-1]


class Problem:
    """the graph of OptimizeSim3: one VertexSim3Expmap, and per correspondence an EdgeSim3ProjectXYZ and an
    EdgeInverseSim3ProjectXYZ over fixed points.  Edge 2i is e12 of pair i, edge 2i + 1 its e21."""

    def __init__(self, x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale, S12, order="forward"):
        f32 = lambda a, w: np.asarray(a, np.float32).reshape(-1, w).astype(np.float64)
        self.x1c, self.x2c, self.obs1, self.obs2 = f32(x1c, 3), f32(x2c, 3), f32(obs1, 2), f32(obs2, 2)
        self.n = len(self.x1c)
        self.K1, self.K2 = np.asarray(K1, np.float32).astype(np.float64), np.asarray(K2, np.float32).astype(np.float64)
        self.th2 = float(np.float32(th2))
        self.delta = float(np.float32(math.sqrt(np.float32(th2))))            # const float deltaHuber (:1095)
        self.fix_scale = bool(fix_scale)
        self.order = order
        info = np.stack([f32(inv_sigma2_1, 1)[:, 0], f32(inv_sigma2_2, 1)[:, 0]], 1)
        self.info = info.reshape(-1)                                          # per edge
        self.active = np.ones(2 * self.n, bool)
        self.err = np.zeros((2 * self.n, 2))                                  # _error of every edge
        self.est = Sim3.from_vector8(S12)
        self.margin = math.inf                # the closest any flagged-on chi2 came to th2, relative to th2

    def errors(self, S):
        """computeError of all edges at S -> [2n, 2] (types_seven_dof_expmap.h:138-145, 160-167)"""
        e = np.zeros((2 * self.n, 2))
        if self.n == 0:
            return e
        p = S.map(self.x2c)
        e[0::2] = self.obs1 - (p[:, :2] / p[:, 2:3] * self.K1[:2] + self.K1[2:])
        p = S.inverse().map(self.x1c)
        e[1::2] = self.obs2 - (p[:, :2] / p[:, 2:3] * self.K2[:2] + self.K2[2:])
        return e

    def oplus(self, S, update):                               # types_seven_dof_expmap.h:60-69
        u = np.array(update, np.float64)
        if self.fix_scale:
            u[6] = 0
        return Sim3.exp(u) * S

    def chi2(self):
        return (self.err ** 2).sum(1) * self.info

    def huber(self, c2):                                      # robust_kernel_impl.cpp:78-91
        dsqr = self.delta * self.delta
        s = np.sqrt(np.maximum(c2, 1e-300))
        inl = c2 <= dsqr
        return np.where(inl, c2, 2 * s * self.delta - dsqr), np.where(inl, 1.0, self.delta / s)

    def compute_active_errors(self):
        self.err[self.active] = self.errors(self.est)[self.active]

    def active_robust_chi2(self):
        rho0, _ = self.huber(self.chi2())
        return float(ordered_sum(rho0[self.active][:, None], self.order)[0])

    def build_system(self):
        """linearizeOplus (numeric, base_binary_edge.hpp:147-196) + constructQuadraticForm (:55-120) of the active edges"""
        J = np.zeros((2 * self.n, 2, 7))
        scalar = 1.0 / (2 * DELTA)
        for d in range(7):
            add = np.zeros(7)
            add[d] = DELTA
            ep = self.errors(self.oplus(self.est, add))       # push, oplus, computeError, pop
            add[d] = -DELTA
            em = self.errors(self.oplus(self.est, add))
            J[:, :, d] = scalar * (ep - em)
        _, rho1 = self.huber(self.chi2())
        w = rho1 * self.info
        omega_r = -(self.info[:, None] * self.err) * rho1[:, None]
        b_rows = np.einsum("ekd,ek->ed", J, omega_r)
        H_rows = np.einsum("ekr,e,ekc->erc", J, w, J)
        rows = np.concatenate([H_rows.reshape(-1, 49), b_rows], 1)[self.active]
        tot = ordered_sum(rows, self.order)
        return tot[:49].reshape(7, 7), tot[49:]

    def optimize(self, iterations):
        if not self.active.any():
            return
        lam, ni, n_bad = 0.0, 2.0, 0
        for it in range(iterations):
            self.compute_active_errors()
            current = self.active_robust_chi2()
            ini = current
            H, b = self.build_system()
            if it == 0:
                lam, ni, n_bad = 1e-5 * float(np.abs(np.diag(H)).max()), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = self.est
                try:
                    x = np.linalg.solve(H + lam * np.eye(7), b)
                    ok2 = bool(np.isfinite(x).all())
                except np.linalg.LinAlgError:
                    x, ok2 = np.zeros(7), False
                if not ok2:
                    x = np.zeros(7)
                self.est = self.oplus(self.est, x)
                self.compute_active_errors()
                temp = self.active_robust_chi2() if ok2 else np.finfo(np.float64).max
                rho = current - temp
                scale = float(sum(x[j] * (lam * x[j] + b[j]) for j in range(7))) + 1e-3
                rho /= scale
                if rho > 0 and math.isfinite(temp):
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current = temp
                else:
                    lam *= ni
                    ni *= 2
                    self.est = backup                         # the edges keep the trial's errors
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                return
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                return

    def note_margin(self, c2):
        if len(c2):
            self.margin = min(self.margin, float(np.abs(c2 - self.th2).min() / self.th2))

    def run(self):
        """-> (S12 [8], flags bool[n], nIn); S12 is None where the reference returns before it writes g2oS12"""
        flags = np.zeros(self.n, bool)
        self.optimize(5)                                                      # :1182
        c2 = self.chi2()
        self.note_margin(c2)
        bad = (c2[0::2] > self.th2) | (c2[1::2] > self.th2)                   # :1193
        flags |= bad
        self.active = np.repeat(~bad, 2)                                      # removeEdge (:1197-1198)
        n_bad = int(bad.sum())
        if self.n - n_bad < 10:                                               # :1211-1212
            return None, flags, 0
        self.optimize(10 if n_bad > 0 else 5)                                 # :1205-1217
        c2 = self.chi2()
        self.note_margin(c2[self.active])
        bad2 = ((c2[0::2] > self.th2) | (c2[1::2] > self.th2)) & ~bad         # :1227
        flags |= bad2
        return self.est.vector8(), flags, int((~flags).sum())


def optimize_sim3(x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale, S12, order="forward"):
    """-> (S12 or None, flags, nIn, margin)"""
    P = Problem(x1c, x2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale, S12, order)
    S, flags, n_in = P.run()
    return S, flags, n_in, P.margin
