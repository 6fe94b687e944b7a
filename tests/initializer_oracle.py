"""fp64 restatement of the monocular Initializer (src/Initializer.cc of the reference) in numpy: the draws (:82-97), Normalize
(:749-795), ComputeH21 / ComputeF21 (:226-303) with the products around them (:160-161, :212), CheckHomography / CheckFundamental
(:305-468), DecomposeE (:909-929), the eight motions of ReconstructH (:584-686), Triangulate / CheckRT (:734-907) and the
acceptance rules of ReconstructF / ReconstructH / Initialize.  Everything is double precision and uses numpy.linalg.svd / inv:
it is what the float path of the library is measured against.  Sequential float32 accumulation appears only where the
reference's order is the contract: the sums of Normalize (normalize_f32) and the score (score_f32, which also restates one match of
the two Check* functions in float32 so that it can be fed the library's own float matrices)."""
import math

import numpy as np

TH_H = 5.991                     # CheckHomography :333
TH_F, TH_SCORE = 3.841, 5.991    # CheckFundamental :408-409
MODEL_H, MODEL_F = 0, 1
f32 = np.float32


def random_int(rand, rand_max, lo, hi):
    """DUtils::Random::RandomInt (Random.cpp:47-50)"""
    d = hi - lo + 1
    return int((rand() / (rand_max + 1.0)) * d) + lo


def draw_sets(N, iterations, rand, rand_max):
    """mvSets (:82-97): swap-with-back selection of 8 of N indices, `iterations` times"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(8):
            r = random_int(rand, rand_max, 0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def matches_of(matches12):
    """mvMatches12 (:54-63) -> (first, second)"""
    m = np.asarray(matches12)
    first = np.nonzero(m >= 0)[0]
    return first.astype(np.int32), m[first].astype(np.int32)


def _seq_sum_f32(x):
    return np.add.accumulate(np.asarray(x, f32), dtype=f32)[-1] if len(x) else f32(0)


def normalize_f32(keys):
    """Normalize (:749-795) with its float sums in key order -> (vNormalizedPoints float32 [n, 2], T float32 3x3)"""
    keys = np.asarray(keys, f32).reshape(-1, 2)
    n = f32(len(keys))
    meanX, meanY = _seq_sum_f32(keys[:, 0]) / n, _seq_sum_f32(keys[:, 1]) / n
    px, py = keys[:, 0] - meanX, keys[:, 1] - meanY
    devX, devY = _seq_sum_f32(np.abs(px)) / n, _seq_sum_f32(np.abs(py)) / n
    sX, sY = f32(1.0 / float(devX)), f32(1.0 / float(devY))
    T = np.array([[sX, 0, -meanX * sX], [0, sY, -meanY * sY], [0, 0, 1]], f32)
    return np.stack([px * sX, py * sY], 1).astype(f32), T


def normalize(keys):
    """The same in float64"""
    keys = np.asarray(keys, np.float64).reshape(-1, 2)
    mean = keys.mean(0)
    p = keys - mean
    s = 1.0 / np.abs(p).mean(0)
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]])
    return p * s, T


def compute_h21(p1, p2):
    """ComputeH21 (:226-266): vt.row(8).reshape(0, 3) of the 2N x 9 matrix"""
    A = []
    for (u1, v1), (u2, v2) in zip(p1, p2):
        A.append([0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2])
        A.append([u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2])
    return np.linalg.svd(np.array(A, np.float64), full_matrices=True)[2][8].reshape(3, 3)


def compute_f21(p1, p2):
    """ComputeF21 (:268-303): the rank-2 projection of vt.row(8)"""
    A = [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1] for (u1, v1), (u2, v2) in zip(p1, p2)]
    Fpre = np.linalg.svd(np.array(A, np.float64), full_matrices=True)[2][8].reshape(3, 3)
    u, w, vt = np.linalg.svd(Fpre)
    w[2] = 0
    return u @ np.diag(w) @ vt


def hypothesis_matrix(model, pn, T1, T2, set8):
    """H21i (:160) / F21i (:212) of one set; pn [N, 4] = the normalised u1 v1 u2 v2 of every match"""
    q = np.asarray(pn, np.float64)[np.asarray(set8)]
    T1, T2 = np.asarray(T1, np.float64), np.asarray(T2, np.float64)
    if model == MODEL_H:
        return np.linalg.inv(T2) @ compute_h21(q[:, :2], q[:, 2:]) @ T1
    return T2.T @ compute_f21(q[:, :2], q[:, 2:]) @ T1


def chi_squares(model, M, uv, sigma):
    """(chiSquare1 [N], chiSquare2 [N]) of CheckHomography (:352-374) / CheckFundamental (:428-454) in float64"""
    M = np.asarray(M, np.float64)
    u1, v1, u2, v2 = np.asarray(uv, np.float64).T
    inv = 1.0 / (sigma * sigma)
    if model == MODEL_H:
        Hi = np.linalg.inv(M)
        w = 1.0 / (Hi[2, 0] * u2 + Hi[2, 1] * v2 + Hi[2, 2])
        a, b = (Hi[0, 0] * u2 + Hi[0, 1] * v2 + Hi[0, 2]) * w, (Hi[1, 0] * u2 + Hi[1, 1] * v2 + Hi[1, 2]) * w
        c1 = ((u1 - a) ** 2 + (v1 - b) ** 2) * inv
        w = 1.0 / (M[2, 0] * u1 + M[2, 1] * v1 + M[2, 2])
        a, b = (M[0, 0] * u1 + M[0, 1] * v1 + M[0, 2]) * w, (M[1, 0] * u1 + M[1, 1] * v1 + M[1, 2]) * w
        c2 = ((u2 - a) ** 2 + (v2 - b) ** 2) * inv
        return c1, c2
    a2, b2, c2_ = M[0, 0] * u1 + M[0, 1] * v1 + M[0, 2], M[1, 0] * u1 + M[1, 1] * v1 + M[1, 2], M[2, 0] * u1 + M[2, 1] * v1 + M[2, 2]
    num2 = a2 * u2 + b2 * v2 + c2_
    c1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
    a1, b1, c1_ = M[0, 0] * u2 + M[1, 0] * v2 + M[2, 0], M[0, 1] * u2 + M[1, 1] * v2 + M[2, 1], M[0, 2] * u2 + M[1, 2] * v2 + M[2, 2]
    num1 = a1 * u1 + b1 * v1 + c1_
    c2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
    return c1, c2


def check(model, M, uv, sigma):
    """-> (score, flags) in float64"""
    c1, c2 = chi_squares(model, M, uv, sigma)
    th = TH_H if model == MODEL_H else TH_F
    ts = TH_H if model == MODEL_H else TH_SCORE
    score = float(np.where(c1 <= th, ts - c1, 0).sum() + np.where(c2 <= th, ts - c2, 0).sum())
    return score, (c1 <= th) & (c2 <= th)


def inv33_f32(S):
    """the 3 x 3 inverse the library documents (csrc/orbp_init_body.h): cofactors and determinant in double, rounded to float32"""
    S = np.asarray(S, f32).astype(np.float64)
    d = S[0, 0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) - S[0, 1] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0]) + \
        S[0, 2] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0])
    if d == 0:
        return np.zeros((3, 3), f32)
    d = 1.0 / d
    t = [(S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) * d, (S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]) * d, (S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]) * d,
         (S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]) * d, (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) * d, (S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]) * d,
         (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]) * d, (S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]) * d, (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) * d]
    return np.array(t, np.float64).astype(f32).reshape(3, 3)


def score_f32(model, M, uv, sigma):
    """The reference's score of a float32 matrix M: every match in float32 as written (:337-385 / :413-465), the sum in float32 in
    match order, term 1 then term 2 -> (score float32, flags).  H12 = M.inv() is inv33_f32."""
    with np.errstate(all="ignore"):
        M = np.asarray(M, f32).reshape(3, 3)
        u1, v1, u2, v2 = (np.ascontiguousarray(c) for c in np.asarray(uv, f32).reshape(-1, 4).T)
        inv = f32(1.0 / float(f32(sigma) * f32(sigma)))
        if model == MODEL_H:
            th = ts = f32(TH_H)
            Hi = inv33_f32(M)
            w = (1.0 / (Hi[2, 0] * u2 + Hi[2, 1] * v2 + Hi[2, 2]).astype(np.float64)).astype(f32)
            a, b = (Hi[0, 0] * u2 + Hi[0, 1] * v2 + Hi[0, 2]) * w, (Hi[1, 0] * u2 + Hi[1, 1] * v2 + Hi[1, 2]) * w
            c1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
            w = (1.0 / (M[2, 0] * u1 + M[2, 1] * v1 + M[2, 2]).astype(np.float64)).astype(f32)
            a, b = (M[0, 0] * u1 + M[0, 1] * v1 + M[0, 2]) * w, (M[1, 0] * u1 + M[1, 1] * v1 + M[1, 2]) * w
            c2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
        else:
            th, ts = f32(TH_F), f32(TH_SCORE)
            a2, b2, cc = M[0, 0] * u1 + M[0, 1] * v1 + M[0, 2], M[1, 0] * u1 + M[1, 1] * v1 + M[1, 2], M[2, 0] * u1 + M[2, 1] * v1 + M[2, 2]
            num2 = a2 * u2 + b2 * v2 + cc
            c1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
            a1, b1, cc = M[0, 0] * u2 + M[1, 0] * v2 + M[2, 0], M[0, 1] * u2 + M[1, 1] * v2 + M[2, 1], M[0, 2] * u2 + M[1, 2] * v2 + M[2, 2]
            num1 = a1 * u1 + b1 * v1 + cc
            c2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
        assert c1.dtype == f32 and c2.dtype == f32
        terms = np.empty(2 * len(c1), f32)
        terms[0::2] = np.where(c1 > th, f32(0), ts - c1)
        terms[1::2] = np.where(c2 > th, f32(0), ts - c2)
        return _seq_sum_f32(terms), ~(c1 > th) & ~(c2 > th)


def find(model, pn, T1, T2, uv, sigma, sets):
    """FindHomography / FindFundamental (:148-171 / :199-222) -> (M or None, score, flags, winning iteration or -1)"""
    best, score, flags, win = None, 0.0, np.zeros(len(uv), bool), -1
    for it, st in enumerate(sets):
        M = hypothesis_matrix(model, pn, T1, T2, st)
        sc, fl = check(model, M, uv, sigma)
        if sc > score:
            best, score, flags, win = M, sc, fl, it
    return best, score, flags, win


def K_matrix(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float64)


def decompose_e(E):
    """DecomposeE (:909-929) -> (R1, R2, t)"""
    u, w, vt = np.linalg.svd(E)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    R1 = u @ W @ vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = u @ W.T @ vt
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return R1, R2, t


def motions_f(F21, K):
    """ReconstructF's four candidates (:479-497) -> [(R, t)]"""
    Km = K_matrix(K)
    R1, R2, t = decompose_e(Km.T @ np.asarray(F21, np.float64) @ Km)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def motions_h(H21, K):
    """The eight motions of ReconstructH (:584-686) -> [(R, t)], or [] at the exit of :597"""
    Km = K_matrix(K)
    A = np.linalg.inv(Km) @ np.asarray(H21, np.float64) @ Km
    U, w, Vt = np.linalg.svd(A)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return []
    aux1, aux3 = math.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), math.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    out = []
    aux_st = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    for i, st in enumerate([aux_st, -aux_st, -aux_st, aux_st]):
        Rp = np.array([[ct, 0, -st], [0, 1, 0], [st, 0, ct]])
        t = U @ (np.array([x1[i], 0, -x3[i]]) * (d1 - d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    aux_sp = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    for i, sp in enumerate([aux_sp, -aux_sp, -aux_sp, aux_sp]):
        Rp = np.array([[cp, 0, sp], [0, -1, 0], [sp, 0, -cp]])
        t = U @ (np.array([x1[i], 0, x3[i]]) * (d1 + d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out


def check_rt(R, t, uv, first, n1, flags, K, th2):
    """CheckRT (:798-907) -> (nGood, vP3D [n1, 3], vbGood [n1], parallax, the sorted cosines)"""
    Km = K_matrix(K)
    P1 = np.hstack([Km, np.zeros((3, 1))])
    P2 = Km @ np.hstack([R, np.asarray(t, np.float64).reshape(3, 1)])
    O2 = -R.T @ t
    good, P = np.zeros(n1, bool), np.zeros((n1, 3))
    cosines = []
    for i, (u1, v1, u2, v2) in enumerate(np.asarray(uv, np.float64)):
        if not flags[i]:
            continue
        A = np.array([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]])
        x = np.linalg.svd(A)[2][3]
        with np.errstate(all="ignore"):
            X = x[:3] / x[3]
        if not np.isfinite(X).all():
            continue
        n1v, n2v = X, X - O2
        cosp = n1v @ n2v / (np.linalg.norm(n1v) * np.linalg.norm(n2v))
        if X[2] <= 0 and cosp < 0.99998:
            continue
        X2 = R @ X + t
        if X2[2] <= 0 and cosp < 0.99998:
            continue
        e1 = (K[0] * X[0] / X[2] + K[2] - u1) ** 2 + (K[1] * X[1] / X[2] + K[3] - v1) ** 2
        if e1 > th2:
            continue
        e2 = (K[0] * X2[0] / X2[2] + K[2] - u2) ** 2 + (K[1] * X2[1] / X2[2] + K[3] - v2) ** 2
        if e2 > th2:
            continue
        cosines.append(cosp)
        P[first[i]] = X
        if cosp < 0.99998:
            good[first[i]] = True
    cosines.sort()
    parallax = math.degrees(math.acos(min(1.0, cosines[min(50, len(cosines) - 1)]))) if cosines else 0.0
    return len(cosines), P, good, parallax, cosines


def initialize(keys1, keys2, matches12, K, sigma, sets, min_parallax=1.0, min_triangulated=50):
    """Initialize (:44-121) on given sets -> dict(ok, model, R, t, P, good, SH, SF, RH, counts, parallax, N)"""
    first, second = matches_of(matches12)
    keys1, keys2 = np.asarray(keys1, np.float64).reshape(-1, 2), np.asarray(keys2, np.float64).reshape(-1, 2)
    uv = np.hstack([keys1[first], keys2[second]])
    pn1, T1 = normalize(keys1)
    pn2, T2 = normalize(keys2)
    pn = np.hstack([pn1[first], pn2[second]])
    H, SH, fH, _ = find(MODEL_H, pn, T1, T2, uv, sigma, sets)
    F, SF, fF, _ = find(MODEL_F, pn, T1, T2, uv, sigma, sets)
    out = dict(ok=False, SH=SH, SF=SF, model=None, counts=[], parallax=[], N=0)
    if SH + SF == 0:
        return out
    RH = out["RH"] = SH / (SH + SF)
    th2 = 4.0 * sigma * sigma
    if RH > 0.40:
        out["model"], flags, mots = MODEL_H, fH, motions_h(H, K)
    else:
        out["model"], flags, mots = MODEL_F, fF, motions_f(F, K)
    N = out["N"] = int(flags.sum())
    res = [check_rt(R, t, uv, first, len(keys1), flags, K, th2) for R, t in mots]
    out["counts"], out["parallax"] = [r[0] for r in res], [r[3] for r in res]
    if not mots:
        return out
    best = -1
    if out["model"] == MODEL_F:
        mx = max(out["counts"])
        nsimilar = sum(c > 0.7 * mx for c in out["counts"])
        if not (mx < max(int(0.9 * N), min_triangulated) or nsimilar > 1):
            k = out["counts"].index(mx)
            if out["parallax"][k] > min_parallax:
                best = k
    else:
        bg = sg = 0
        bi, bp = -1, -1.0
        for i, c in enumerate(out["counts"]):
            if c > bg:
                sg, bg, bi, bp = bg, c, i, out["parallax"][i]
            elif c > sg:
                sg = c
        out["second"] = sg
        if sg < 0.75 * bg and bp >= min_parallax and bg > min_triangulated and bg > 0.9 * N:
            best = bi
    if best >= 0:
        out.update(ok=True, R=mots[best][0], t=mots[best][1], P=res[best][1], good=res[best][2], best=best)
    return out
