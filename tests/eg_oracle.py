"""A numpy fp64 restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044 on g2o) for the tests of
orbp_optimize_essential_graph / orbm_optimize_essential_graph.  Vectorised over edges and perturbations, full dense H, LAPACK for
the 3 x 3 W.lu().solve(t) and for the 7N x 7N system: not the product's text.  Cited lines (Thirdparty/g2o/g2o unless src/):
  Sim3(Vector7d)  types/sim3.h:70-142        Sim3::log  types/sim3.h:148-230        operator*, inverse, map  :266-272, :233-236, :144-146
  EdgeSim3::computeError  types/types_seven_dof_expmap.h:106-114        VertexSim3Expmap::oplusImpl  :60-69
  numeric linearizeOplus  core/base_binary_edge.hpp:130-205              constructQuadraticForm  core/base_binary_edge.hpp:55-90
  Levenberg  core/optimization_algorithm_levenberg.cpp:61-189 with setUserLambdaInit(1e-16) (src/Optimizer.cc:794)
  measurements  src/Optimizer.cc:857-867, :889-972        write-back  src/Optimizer.cc:992-1043

Two switches measure what two correct implementations may differ by (tests/tools/measure_eg_spread.py):
  order = "forward" / "reverse": the order of every sum over edges (H, b, chi2) and of computeScale's sum over the unknowns;
  nudge = 0 / +1 / -1: every result of acos, sin, cos, log and exp inside Sim3 log / exp moves by that many ulp (np.nextafter).
The numeric Jacobian divides differences of log() by 2e-9, so one ulp in a transcendental becomes about 1e-7 in J.

optimize_essential_graph() returns a dict: Scw float64 [n, 8], Tcw float64 [n, 4, 4], xw float64 [P, 3], stats (iterations, trials,
lambda, chi2_initial, chi2_final), transcript = [(iteration, trial, accepted)], decisions = [(kind, value)] with kind "rho" (rho
against 0 in every trial: accept / reject, the trial loop's end, the rho == 0 termination) or "nbad" (((iniChi - currentChi) * 1e3 -
iniChi) / iniChi against 0, which feeds _nBad), in the order they were taken, margin = the smallest |value| among them (the distance
of the closest decision from its boundary, as tests/ba_oracle.py reports it)."""
import math

import numpy as np

EPS = 0.00001
DELTA = 1e-9
DBL_MAX = 1.7976931348623157e308
_nudge = 0


def _n(x):
    """a transcendental's result, moved by the nudge"""
    if _nudge == 0:
        return x
    return np.nextafter(x, np.inf if _nudge > 0 else -np.inf)


def quat_from_R(R):
    """Eigen's Quaterniond(Matrix3d) on [..., 3, 3] -> x, y, z, w"""
    with np.errstate(invalid="ignore", divide="ignore"):
        tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
        t = np.sqrt(tr + 1.0)
        q0 = np.stack([(R[..., 2, 1] - R[..., 1, 2]) * (0.5 / t), (R[..., 0, 2] - R[..., 2, 0]) * (0.5 / t),
                       (R[..., 1, 0] - R[..., 0, 1]) * (0.5 / t), 0.5 * t], -1)
        i = np.zeros(tr.shape, int)
        i = np.where(R[..., 1, 1] > R[..., 0, 0], 1, i)
        i = np.where(R[..., 2, 2] > np.where(i == 1, R[..., 1, 1], R[..., 0, 0]), 2, i)
        out = q0
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            t = np.sqrt(R[..., a, a] - R[..., b, b] - R[..., c, c] + 1.0)
            q = np.zeros(R.shape[:-2] + (4,))
            q[..., a] = 0.5 * t
            t = 0.5 / t
            q[..., 3] = (R[..., c, b] - R[..., b, c]) * t
            q[..., b] = (R[..., b, a] + R[..., a, b]) * t
            q[..., c] = (R[..., c, a] + R[..., a, c]) * t
            out = np.where(((tr <= 0) & (i == a))[..., None], q, out)
    return out


def quat_to_R(q):
    """Eigen's toRotationMatrix, nothing normalised"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def rotate(q, v):
    """Eigen's Quaterniond * Vector3d"""
    uv = 2 * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * uv + np.cross(q[..., :3], uv)


def smap(S, x):
    return S[..., 7:8] * rotate(S[..., :4], x) + S[..., 4:7]


def mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                  aw * bw - ax * bx - ay * by - az * bz], -1)
    a, b = np.broadcast_arrays(a, b)
    return np.concatenate([q, smap(a, b[..., 4:7]), a[..., 7:8] * b[..., 7:8]], -1)


def inverse(a):
    q = a[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([q, rotate(q, (-1.0 / a[..., 7:8]) * a[..., 4:7]), 1.0 / a[..., 7:8]], -1)


def skew(w):
    z = np.zeros(w.shape[:-1])
    return np.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).reshape(w.shape[:-1] + (3, 3))


def sim3_exp(u):
    """Sim3(const Vector7d &) (sim3.h:70-142) on [..., 7]"""
    omega, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt((omega * omega).sum(-1))
    O = skew(omega)
    O2 = O @ O
    s = _n(np.exp(sigma))
    I = np.eye(3)
    small_s, small_t = np.abs(sigma) < EPS, theta < EPS
    with np.errstate(invalid="ignore", divide="ignore"):
        sn, cs = _n(np.sin(theta)), _n(np.cos(theta))
        theta2, sigma2 = theta * theta, sigma * sigma
        R_small = I + O + O2
        R_big = I + (sn / theta)[..., None, None] * O + ((1 - cs) / (theta * theta))[..., None, None] * O2
        R = np.where(small_t[..., None, None], R_small, R_big)
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        a, b, c = s * sn, s * cs, theta2 + sigma2
        A = np.where(small_s, np.where(small_t, 0.5, (1 - cs) / theta2),
                     np.where(small_t, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small_s, np.where(small_t, 1.0 / 6.0, (theta - sn) / (theta2 * theta)),
                     np.where(small_t, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2))
    W = A[..., None, None] * O + B[..., None, None] * O2 + C[..., None, None] * I
    t = (W @ ups[..., None])[..., 0]
    return np.concatenate([quat_from_R(R), t, s[..., None]], -1)


def sim3_log(S):
    """Sim3::log (sim3.h:148-230) on [..., 8]"""
    s = S[..., 7]
    sigma = _n(np.log(s))
    R = quat_to_R(S[..., :4])
    d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    small_s, small_t = np.abs(sigma) < EPS, d > 1 - EPS
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = _n(np.arccos(d))
        sn, cs = _n(np.sin(theta)), _n(np.cos(theta))
        theta2, sigma2 = theta * theta, sigma * sigma
        f = np.where(small_t, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        a, b, c = s * sn, s * cs, theta2 + sigma2
        A = np.where(small_s, np.where(small_t, 0.5, (1 - cs) / theta2),
                     np.where(small_t, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small_s, np.where(small_t, 1.0 / 6.0, (theta - sn) / (theta2 * theta)),
                     np.where(small_t, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2))
    omega = f[..., None] * dR
    O = skew(omega)
    W = A[..., None, None] * O + B[..., None, None] * (O @ O) + C[..., None, None] * np.eye(3)
    ups = np.linalg.solve(W, S[..., 4:7, None])[..., 0]
    return np.concatenate([omega, ups, sigma[..., None]], -1)


def oplus(S, u, fix_scale):
    """VertexSim3Expmap::oplusImpl"""
    if fix_scale:
        u = u.copy()
        u[..., 6] = 0.0
    return mul(sim3_exp(u), S)


def edge_errors(C, Si, Sj):
    """EdgeSim3::computeError"""
    return sim3_log(mul(mul(C, Si), inverse(Sj)))


def log_branches(pr):
    """(|sigma| < eps, d > 1 - eps) of Sim3::log for every edge's error at the input estimates"""
    g = Graph(pr, "forward")
    S = mul(mul(g.meas, g.est[g.ei]), inverse(g.est[g.ej]))
    R = quat_to_R(S[..., :4])
    d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    return np.abs(np.log(S[..., 7])) < EPS, d > 1 - EPS


class Graph:
    def __init__(self, pr, order):
        self.order = order
        self.Scw = np.asarray(pr["Scw"], np.float64).reshape(-1, 8)
        self.Snc = np.asarray(pr["Snc"] if pr.get("Snc") is not None else pr["Scw"], np.float64).reshape(-1, 8)
        self.n = len(self.Scw)
        self.fixed = int(pr.get("fixed", -1))
        self.fix_scale = bool(pr.get("fix_scale"))
        self.ei = np.asarray(pr["edge_i"], int).reshape(-1)
        self.ej = np.asarray(pr["edge_j"], int).reshape(-1)
        corr = np.asarray(pr["edge_corrected"], bool).reshape(-1)
        self.E = len(self.ei)
        self.est = self.Scw.copy()
        src_i = np.where(corr[:, None], self.Scw[self.ei], self.Snc[self.ei])
        src_j = np.where(corr[:, None], self.Scw[self.ej], self.Snc[self.ej])
        self.meas = mul(src_j, inverse(src_i)) if self.E else np.zeros((0, 8))      # Sji = Sjw * Swi
        self.free_of = np.full(self.n, -1)
        free = [k for k in range(self.n) if k != self.fixed]
        self.free_of[free] = np.arange(len(free))
        self.free = np.array(free, int)
        self.N = 7 * len(free)
        self.transcript, self.decisions = [], []

    def ordered_sum(self, terms):
        s = 0.0
        for t in (terms[::-1] if self.order == "reverse" else terms):
            s += float(t)
        return s

    def chi2(self):
        e = edge_errors(self.meas, self.est[self.ei], self.est[self.ej])
        self.err = e
        return self.ordered_sum((e * e).sum(-1))

    def build(self):
        """linearizeOplus (numeric) + constructQuadraticForm over the edges: dense H and b"""
        U = np.zeros((14, 7))
        for d in range(7):
            U[2 * d, d], U[2 * d + 1, d] = DELTA, -DELTA
        C, Si, Sj = self.meas[:, None, :], self.est[self.ei][:, None, :], self.est[self.ej][:, None, :]
        scalar = 1.0 / (2 * DELTA)
        ei_p = edge_errors(C, oplus(np.broadcast_to(Si, (self.E, 14, 8)), np.broadcast_to(U, (self.E, 14, 7)), self.fix_scale), Sj)
        ej_p = edge_errors(C, Si, oplus(np.broadcast_to(Sj, (self.E, 14, 8)), np.broadcast_to(U, (self.E, 14, 7)), self.fix_scale))
        A = scalar * np.swapaxes(ei_p[:, 0::2, :] - ei_p[:, 1::2, :], 1, 2)      # [E, 7 (error), 7 (axis)]
        B = scalar * np.swapaxes(ej_p[:, 0::2, :] - ej_p[:, 1::2, :], 1, 2)
        H, b = np.zeros((self.N, self.N)), np.zeros(self.N)
        edges = range(self.E - 1, -1, -1) if self.order == "reverse" else range(self.E)
        for e in edges:
            fi, fj = self.free_of[self.ei[e]], self.free_of[self.ej[e]]
            r = -self.err[e]                                                      # omega_r = -Omega e
            if fi >= 0:
                H[7 * fi:7 * fi + 7, 7 * fi:7 * fi + 7] += A[e].T @ A[e]
                b[7 * fi:7 * fi + 7] += A[e].T @ r
            if fj >= 0:
                H[7 * fj:7 * fj + 7, 7 * fj:7 * fj + 7] += B[e].T @ B[e]
                b[7 * fj:7 * fj + 7] += B[e].T @ r
            if fi >= 0 and fj >= 0:
                H[7 * fi:7 * fi + 7, 7 * fj:7 * fj + 7] += A[e].T @ B[e]
                H[7 * fj:7 * fj + 7, 7 * fi:7 * fi + 7] += B[e].T @ A[e]
        self.H, self.b = H, b

    def solve(self, lam):
        try:
            L = np.linalg.cholesky(self.H + lam * np.eye(self.N))
        except np.linalg.LinAlgError:
            return False, np.zeros(self.N)
        x = np.linalg.solve(L.T, np.linalg.solve(L, self.b))
        return bool(np.isfinite(x).all()), x

    def optimize(self, iterations, stats):
        lam, ni, n_bad = 0.0, 2.0, 0
        for it in range(iterations):
            current = self.chi2()
            if it == 0:
                stats["chi2_initial"] = current
                lam, ni, n_bad = 1e-16, 2.0, 0                   # computeLambdaInit returns _userLambdaInit
            ini = current
            self.build()
            rho, qmax = 0.0, 0
            while True:
                backup = self.est.copy()
                ok, x = self.solve(lam)
                if not ok:
                    x = np.zeros(self.N)
                sc = self.ordered_sum(x * (lam * x + self.b))
                if self.N:
                    self.est[self.free] = oplus(self.est[self.free], x.reshape(-1, 7), self.fix_scale)
                temp = self.chi2()
                if not ok:
                    temp = DBL_MAX
                rho = (current - temp) / (sc + 1e-3)
                self.decisions.append(("rho", rho))
                good = rho > 0 and math.isfinite(temp)
                self.transcript.append((it, qmax, bool(good)))
                if good:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                else:
                    lam *= ni
                    ni *= 2
                    self.est = backup
                qmax += 1
                stats["trials"] += 1
                if not (rho < 0 and qmax < 10):
                    break
            stats["iterations"] += 1
            stats["lambda"], stats["chi2_final"] = lam, current
            if qmax == 10 or rho == 0:
                break
            self.decisions.append(("nbad", ((ini - current) * 1e3 - ini) / ini if ini > 0 else math.inf))
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                break


def optimize_essential_graph(pr, n_iterations=20, order="forward", nudge=0):
    global _nudge
    _nudge = nudge
    try:
        g = Graph(pr, order)
        stats = {"iterations": 0, "trials": 0, "lambda": 0.0, "chi2_initial": 0.0, "chi2_final": 0.0}
        if g.E > 0 and g.N > 0:
            g.optimize(n_iterations, stats)
        if stats["iterations"] == 0:
            stats["chi2_initial"] = stats["chi2_final"] = g.chi2() if g.E else 0.0
        Tcw = np.zeros((g.n, 4, 4))                              # :999-1009
        Tcw[:, :3, :3] = quat_to_R(g.est[:, :4])
        Tcw[:, :3, 3] = g.est[:, 4:7] * (1.0 / g.est[:, 7:8])
        Tcw[:, 3, 3] = 1.0
        xw = np.asarray(pr.get("xw", np.zeros((0, 3))), np.float32).astype(np.float64).reshape(-1, 3)
        ref = np.asarray(pr.get("ref", np.zeros(0)), int).reshape(-1)
        has = ref >= 0
        if has.any():                                            # :1032-1040
            xw[has] = smap(inverse(g.est[ref[has]]), smap(g.Scw[ref[has]], xw[has]))
        margin = min([abs(v) for _, v in g.decisions], default=math.inf)
        return {"Scw": g.est.copy(), "Tcw": Tcw, "xw": xw, "stats": stats, "transcript": g.transcript, "decisions": g.decisions,
                "margin": margin}
    finally:
        _nudge = 0
