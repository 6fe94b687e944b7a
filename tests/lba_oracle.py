"""An independent numpy restatement of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778 on g2o) for the tests of
orbp_local_bundle_adjustment / orbm_local_bundle_adjustment.  Not the product's text: poses are rotation matrices and translations
(the product keeps unit quaternions), the Jacobians are the chain rule through the projection (the product restates g2o's written-out
entries), the Schur complement is a dense matrix product over all points at once, the key frames without active edges leave the
reduced system (the product keeps an identity block for them), the reduced system goes to LAPACK (Cholesky, then two solves), and
the errors are recomputed at the top of every iteration as g2o does (the product carries the accepted trial's chi2).

order = "forward" adds the edges' terms into the blocks in edge order and multiplies the Schur product with the points in order,
"reverse" does both backwards; the difference of the two runs is what a summation order can move
(tests/tools/measure_lba_spread.py).

Returns a dict: Tcw float64 [n_local, 4, 4], xw float64 [n_points, 3], erase bool [E], level1 bool [E], stats (as orbp_lba_stats),
margin = the smallest relative distance of any decision from its boundary, transcript = [(round, iteration, trial, accepted)],
stale_chi2 / fresh_chi2 float64 [E]: chi2() of every edge as the final pass reads it, and recomputed at the final estimates."""
import math

import numpy as np

TH_MONO, TH_STEREO = 5.991, 7.815
DELTA_MONO, DELTA_STEREO = float(np.float32(math.sqrt(5.991))), float(np.float32(math.sqrt(7.815)))
DBL_MAX = 1.7976931348623157e308


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def rot_from_float(Rf):
    """the rotation g2o::SE3Quat(R, t) keeps of a float matrix: Eigen's Quaterniond(R), normalised, as a matrix again"""
    R = np.asarray(Rf, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        v = np.array([(R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s])
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        v = np.zeros(3)
        v[i] = 0.5 * s
        s = 0.5 / s
        w = (R[k, j] - R[j, k]) * s
        v[j] = (R[j, i] + R[i, j]) * s
        v[k] = (R[k, i] + R[i, k]) * s
    q = np.concatenate([[w], v])
    q /= math.sqrt(float(q @ q))
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def se3_exp(u):
    """SE3Quat::exp: (R, t) of omega = u[:3], upsilon = u[3:]"""
    om, up = u[:3], u[3:]
    th = math.sqrt(float(om @ om))
    O = skew(om)
    if th < 1e-5:
        # g2o takes R = V = I + O + O O here and then normalises R's quaternion, which leaves the rotation of omega to O(th^3).
        # A matrix has no normalisation step, so R is the series of the rotation itself; V is g2o's.
        V = np.eye(3) + O + O @ O
        R = np.eye(3) + (1 - th * th / 6) * O + (0.5 - th * th / 24) * O @ O
    else:
        a, b, c = math.sin(th) / th, (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
        R = np.eye(3) + a * O + b * O @ O
        V = np.eye(3) + b * O + c * O @ O
    return R, V @ up


class Graph:
    def __init__(self, pr, order):
        self.order = order
        self.n_local = len(pr["local_fixed"])
        T = np.asarray(pr["Tcw"], np.float32).reshape(-1, 4, 4)
        self.NK = len(T)
        self.R = np.stack([rot_from_float(t[:3, :3]) for t in T]) if self.NK else np.zeros((0, 3, 3))
        self.t = T[:, :3, 3].astype(np.float64)
        self.cam = np.asarray(pr["cam"], np.float32).reshape(-1, 5).astype(np.float64)
        self.free = np.zeros(self.NK, bool)
        self.free[:self.n_local] = np.asarray(pr["local_fixed"]).reshape(-1) == 0
        self.X = np.asarray(pr["xw"], np.float32).reshape(-1, 3).astype(np.float64)
        self.P = len(self.X)
        off = np.asarray(pr["edge_off"], np.int64)
        self.E = int(off[-1])
        self.pt = np.repeat(np.arange(self.P), np.diff(off))
        self.kf = np.asarray(pr["edge_kf"], np.int64).reshape(-1)
        self.obs = np.asarray(pr["obs"], np.float32).reshape(-1, 2).astype(np.float64)
        self.ur32 = np.asarray(pr["u_right"], np.float32).reshape(-1)
        self.stereo = ~(self.ur32 < 0)
        self.ur = self.ur32.astype(np.float64)
        self.info = np.asarray(pr["inv_sigma2"], np.float32).reshape(-1).astype(np.float64)
        self.level = np.zeros(self.E, bool)
        self.robust = True
        self.err = np.zeros((self.E, 3))
        self.margin = math.inf
        self.transcript = []

    def note(self, value, boundary_scale):
        """a decision `value` against 0, relative to boundary_scale"""
        m = abs(value) / boundary_scale if boundary_scale > 0 else math.inf
        if m < self.margin:
            self.margin = m

    # ---- per-edge quantities, all edges at once -------------------------------------------------------------------------
    def camera_points(self, idx):
        k, p = self.kf[idx], self.pt[idx]
        return np.einsum("eij,ej->ei", self.R[k], self.X[p]) + self.t[k]

    def errors_of(self, idx):
        pc = self.camera_points(idx)
        c = self.cam[self.kf[idx]]
        st = self.stereo[idx]
        e = np.zeros((len(idx), 3))
        z = pc[:, 2]
        mono = ~st
        e[mono, 0] = self.obs[idx][mono, 0] - (pc[mono, 0] / z[mono] * c[mono, 0] + c[mono, 2])
        e[mono, 1] = self.obs[idx][mono, 1] - (pc[mono, 1] / z[mono] * c[mono, 1] + c[mono, 3])
        invz = (1.0 / z[st]).astype(np.float32).astype(np.float64)         # the stereo cam_project keeps 1/z as a float
        u = pc[st, 0] * invz * c[st, 0] + c[st, 2]
        e[st, 0] = self.obs[idx][st, 0] - u
        e[st, 1] = self.obs[idx][st, 1] - (pc[st, 1] * invz * c[st, 1] + c[st, 3])
        e[st, 2] = self.ur[idx][st] - (u - c[st, 4] * invz)
        return e

    def chi2_of(self, err, idx):
        return (err * err).sum(1) * self.info[idx]

    def active(self):
        return np.flatnonzero(~self.level)

    def compute_active_errors(self):
        idx = self.active()
        self.err[idx] = self.errors_of(idx)

    def ordered_sum(self, terms):
        terms = np.asarray(terms)
        if self.order == "reverse":
            terms = terms[::-1]
        s = 0.0
        for v in terms.tolist():
            s += v
        return s

    def active_robust_chi2(self):
        idx = self.active()
        c2 = self.chi2_of(self.err[idx], idx)
        if self.robust:
            d = np.where(self.stereo[idx], DELTA_STEREO, DELTA_MONO)
            big = c2 > d * d
            c2 = np.where(big, 2 * np.sqrt(np.where(big, c2, 1.0)) * d - d * d, c2)
        return self.ordered_sum(c2)

    def build(self):
        """the active vertices and the normal equations at the current estimates and stored errors"""
        idx = self.active()
        if self.order == "reverse":
            idx = idx[::-1]
        k, p = self.kf[idx], self.pt[idx]
        pc = self.camera_points(idx)
        c = self.cam[k]
        x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
        n = len(idx)
        Jproj = np.zeros((n, 3, 3))                           # d cam_project / d pc
        Jproj[:, 0, 0] = c[:, 0] / z
        Jproj[:, 0, 2] = -c[:, 0] * x / z ** 2
        Jproj[:, 1, 1] = c[:, 1] / z
        Jproj[:, 1, 2] = -c[:, 1] * y / z ** 2
        st = self.stereo[idx]
        Jproj[st, 2, :] = Jproj[st, 0, :]
        Jproj[st, 2, 2] += c[st, 4] / z[st] ** 2
        A = -np.einsum("eij,ejk->eik", Jproj, self.R[k])      # d error / d point
        dpc = np.zeros((n, 3, 6))                             # d pc / d (omega, upsilon) of exp(update) * T
        dpc[:, 0, 1], dpc[:, 0, 2] = z, -y
        dpc[:, 1, 0], dpc[:, 1, 2] = -z, x
        dpc[:, 2, 0], dpc[:, 2, 1] = y, -x
        dpc[:, 0, 3] = dpc[:, 1, 4] = dpc[:, 2, 5] = 1
        B = -np.einsum("eij,ejk->eik", Jproj, dpc)
        err, info = self.err[idx], self.info[idx]
        w = np.ones(n)
        if self.robust:
            c2 = self.chi2_of(err, idx)
            d = np.where(st, DELTA_STEREO, DELTA_MONO)
            big = c2 > d * d
            w = np.where(big, d / np.sqrt(np.where(big, c2, 1.0)), 1.0)
        wi = w * info
        r = -(err * wi[:, None])
        kfree = self.free[k]
        self.akf = np.flatnonzero(np.bincount(k[kfree], minlength=self.NK) > 0) if n else np.zeros(0, np.int64)
        self.apt = np.flatnonzero(np.bincount(p, minlength=self.P) > 0) if n else np.zeros(0, np.int64)
        slot = -np.ones(self.NK, np.int64)
        slot[self.akf] = np.arange(len(self.akf))
        pslot = -np.ones(self.P, np.int64)
        pslot[self.apt] = np.arange(len(self.apt))
        Ka, Pa = len(self.akf), len(self.apt)
        self.Hll = np.zeros((Pa, 3, 3))
        self.bl = np.zeros((Pa, 3))
        np.add.at(self.Hll, pslot[p], np.einsum("eji,e,ejk->eik", A, wi, A))
        np.add.at(self.bl, pslot[p], np.einsum("eji,ej->ei", A, r))
        self.Hpp = np.zeros((Ka, 6, 6))
        self.bp = np.zeros((Ka, 6))
        f = np.flatnonzero(kfree)
        np.add.at(self.Hpp, slot[k[f]], np.einsum("eji,e,ejk->eik", B[f], wi[f], B[f]))
        np.add.at(self.bp, slot[k[f]], np.einsum("eji,ej->ei", B[f], r[f]))
        self.Hpl = np.zeros((6 * Ka, 3 * Pa))
        W = np.einsum("eji,e,ejk->eik", B[f], wi[f], A[f])    # 6 x 3
        rows = (6 * slot[k[f]])[:, None, None] + np.arange(6)[None, :, None]
        cols = (3 * pslot[p[f]])[:, None, None] + np.arange(3)[None, None, :]
        self.Hpl[rows, cols] = W

    def max_diagonal(self):
        d = [0.0]
        if len(self.akf):
            d.append(np.abs(np.einsum("kii->ki", self.Hpp)).max())
        if len(self.apt):
            d.append(np.abs(np.einsum("pii->pi", self.Hll)).max())
        return float(max(d))

    def solve(self, lam):
        """BlockSolver_6_3::solve with lambda on both diagonals -> (ok, xp [Ka, 6], xl [Pa, 3])"""
        Ka, Pa = len(self.akf), len(self.apt)
        Dinv = np.linalg.inv(self.Hll + lam * np.eye(3)) if Pa else np.zeros((0, 3, 3))
        Hpp = np.zeros((6 * Ka, 6 * Ka))
        for s in range(Ka):
            Hpp[6 * s:6 * s + 6, 6 * s:6 * s + 6] = self.Hpp[s] + lam * np.eye(6)
        Hpl = self.Hpl.reshape(6 * Ka, Pa, 3)
        HD = np.einsum("rpi,pij->rpj", Hpl, Dinv)             # Hpl Dinv, point block by point block
        bl = self.bl
        if self.order == "reverse":                           # the product over the points, last point first
            Hpl, HD, bl = Hpl[:, ::-1], HD[:, ::-1], bl[::-1]
        HD = np.ascontiguousarray(HD).reshape(6 * Ka, 3 * Pa)
        S = Hpp - HD @ np.ascontiguousarray(Hpl).reshape(6 * Ka, 3 * Pa).T
        bs = self.bp.reshape(-1) - HD @ np.ascontiguousarray(bl).reshape(-1)
        xp = np.zeros(6 * Ka)
        if Ka:
            if not np.isfinite(S).all():
                return False, None, None
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                return False, None, None
            xp = np.linalg.solve(L.T, np.linalg.solve(L, bs))
        cl = self.bl.reshape(-1) - self.Hpl.T @ xp
        xl = np.einsum("pij,pj->pi", Dinv, cl.reshape(-1, 3))
        return True, xp.reshape(-1, 6), xl

    def scale(self, xp, xl, lam):
        terms = np.concatenate([(xp * (lam * xp + self.bp)).reshape(-1), (xl * (lam * xl + self.bl)).reshape(-1)])
        return self.ordered_sum(terms)

    def apply(self, xp, xl):
        for s, k in enumerate(self.akf):
            dR, dt = se3_exp(xp[s])
            self.t[k] = dR @ self.t[k] + dt
            self.R[k] = dR @ self.R[k]
        self.X[self.apt] += xl

    def optimize(self, rnd, iterations, stats):
        if len(self.active()) == 0:
            return
        lam, ni, n_bad = 0.0, 2.0, 0
        for it in range(iterations):
            self.compute_active_errors()
            current = self.active_robust_chi2()
            ini = current
            self.build()
            if it == 0:
                lam, ni, n_bad = 1e-5 * self.max_diagonal(), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = (self.R.copy(), self.t.copy(), self.X.copy())
                ok, xp, xl = self.solve(lam)
                sc = 0.0
                if ok:
                    sc = self.scale(xp, xl, lam)
                    self.apply(xp, xl)
                self.compute_active_errors()
                temp = self.active_robust_chi2() if ok else DBL_MAX
                rho = (current - temp) / (sc + 1e-3)
                self.note(rho, 1.0)
                good = rho > 0 and math.isfinite(temp)
                self.transcript.append((rnd, it, qmax, bool(good)))
                if good:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                else:
                    lam *= ni
                    ni *= 2
                    self.R, self.t, self.X = backup
                qmax += 1
                stats["trials"][rnd] += 1
                if not (rho < 0 and qmax < 10):
                    break
            stats["iterations"][rnd] += 1
            stats["lambda"], stats["chi2"] = lam, current
            if qmax == 10 or rho == 0:
                break
            self.note((ini - current) * 1e3 - ini, ini)
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                break

    def flagged(self, err):
        idx = np.arange(self.E)
        c2 = self.chi2_of(err, idx)
        th = np.where(self.stereo, TH_STEREO, TH_MONO)
        pc = self.camera_points(idx)
        z = pc[:, 2]
        if self.E:
            self.margin = min(self.margin, float((np.abs(c2 - th) / th).min()), float((np.abs(z) / np.linalg.norm(pc, axis=1)).min()))
        return (c2 > th) | ~(z > 0), c2


def local_bundle_adjustment(pr, order="forward"):
    g = Graph(pr, order)
    stats = {"iterations": [0, 0], "trials": [0, 0], "lambda": 0.0, "chi2": 0.0, "n_level1": 0, "second_round": 1}
    g.optimize(0, 5, stats)
    bad, _ = g.flagged(g.err)
    g.level = bad.copy()
    stats["n_level1"] = int(bad.sum())
    g.robust = False
    g.optimize(1, 10, stats)
    erase, stale = g.flagged(g.err)
    fresh = g.chi2_of(g.errors_of(np.arange(g.E)), np.arange(g.E)) if g.E else np.zeros(0)
    Tcw = np.zeros((g.n_local, 4, 4))
    for k in range(g.n_local):
        Tcw[k, :3, :3], Tcw[k, :3, 3], Tcw[k, 3, 3] = g.R[k], g.t[k], 1.0
    stats["iterations"], stats["trials"] = tuple(stats["iterations"]), tuple(stats["trials"])
    return {"Tcw": Tcw, "xw": g.X.copy(), "erase": erase, "level1": bad, "stats": stats, "margin": g.margin, "transcript": g.transcript,
            "stale_chi2": stale, "fresh_chi2": fresh}
