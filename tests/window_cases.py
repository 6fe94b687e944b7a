"""Planted fixtures for the windowed ORBmatcher searches (tests/test_window_cases_cpu.py pins the oracle to hand-derived answers on
them, tests/test_window_cases_gpu.py pins the library to the oracle).

Part 1, kf_case(grid): one key frame of about 200 key points on 8 levels for the stateless kernel k_search_kf (Fuse, Fuse(Scw),
both directions of SearchBySim3), built once per key-frame grid (plain, distorted, positive origins).
Part 2, sim3proj_case / init_case / last_case / map_case / kfproj_case: one small frame per sequential host scan.

Exact projections.  The oracle's key-frame entries project world points themselves, the C ABI takes (u, v, level).  Both see the
same bits under the identity camera: K = (1, 1, 0, 0), Tcw = I, xw = (u, v, 1) gives zc = 1, invz = 1, u' = 1 * (u * 1) + 0 = u;
wide image bounds let off-grid queries reach the window code; normal = xw / |xw| passes the viewing-angle test, min_inv = 0 and
max_inv = inf the distance gate, and mf_max = |xw| * 1.2**(l - 0.5) makes PredictScale return ceil(l - 0.5) = l.

Descriptors.  Query descriptors are rows of the 256 x 256 Sylvester Hadamard matrix (any two rows differ in exactly 128 bits) or a
row with a few of its first six bits flipped (MapPoints that contend for one slot); background train descriptors are other rows.  A
planted train descriptor is a query with d bits above the sixth flipped, drawn again until it is farther than FAR = 120 from every
query of another family.  So every distance that is not planted lies above 120, for the TH_LOW and the TH_HIGH searches alike."""
import functools

import numpy as np

import oracle_lib as O

F32 = np.float32
NLEV = 8
FAR = 120
KID = (1.0, 1.0, 0.0, 0.0)
WIDE = (-1e4, 1e4, -1e4, 1e4)
LOGSF = float(np.log(F32(1.2)))
SF = np.ones(NLEV, F32)
for _l in range(1, NLEV):
    SF[_l] = F32(SF[_l - 1] * F32(1.2))
KF_GRIDS = ("plain", "distorted", "positive")


def pack(bits):
    return np.packbits(np.ascontiguousarray(bits, np.uint8), axis=1, bitorder="little")


def hamming(a, b):
    """all distances between two sets of packed descriptors"""
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _hadamard():
    a = np.arange(256, dtype=np.uint8)
    return (np.unpackbits((a[:, None] & a[None, :])[..., None], axis=2).sum(2) & 1).astype(np.uint8)


class Book:
    """Descriptor bits of one fixture.  query() -> a new family (a Hadamard row); variant(q, bits) -> a member of q's family with
    some of the six reserved bits flipped; plant(q, d) -> a train row at distance d from q (and d + the reserved bits that differ
    from q's relatives), farther than FAR from every other family; background() -> a row 128 away from every family."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.H = _hadamard()
        self.nq, self.nb = 0, 255
        self.q, self.family = [], []

    def query(self):
        self.nq += 1
        assert self.nq < self.nb
        self.q.append(self.H[self.nq].copy()); self.family.append(len(self.q) - 1)
        return len(self.q) - 1

    def variant(self, q, bits):
        v = self.q[q].copy(); v[list(bits)] ^= 1
        self.q.append(v); self.family.append(self.family[q])
        return len(self.q) - 1

    def background(self):
        self.nb -= 1
        assert self.nq < self.nb
        return self.H[self.nb].copy()

    def plant(self, q, d, reserved=()):
        """call after every query of the fixture exists; `reserved`: reserved bits among the d flipped ones"""
        Q = np.stack(self.q)
        others = Q[np.array(self.family) != self.family[q]]
        for _ in range(20000):
            t = self.q[q].copy()
            t[list(reserved)] ^= 1
            t[6 + self.rng.permutation(250)[:d - len(reserved)]] ^= 1
            if len(others) == 0 or (others ^ t).sum(1).min() > FAR:
                return t
        raise AssertionError("no planted row farther than FAR from the other queries")

    def queries(self):
        return pack(np.stack(self.q))


def kp_array(rows):
    """rows of (x, y, octave[, angle]) -> KP_DTYPE"""
    k = np.zeros(len(rows), O.KP_DTYPE)
    for i, r in enumerate(rows):
        k["x"][i], k["y"][i], k["octave"][i] = F32(r[0]), F32(r[1]), r[2]
        k["angle"][i] = F32(r[3]) if len(r) > 3 else 0.0
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    return k


def mappoints(u, v, lv):
    """(xw, normal, mf_max, min_inv, max_inv) of MapPoints that the identity camera projects to (u, v) on level lv"""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    xw = np.stack([u, v, np.ones_like(u)], 1).astype(F32)
    d = np.linalg.norm(xw.astype(np.float64), axis=1)
    normal = (xw / d[:, None]).astype(F32)
    mf_max = (d * 1.2 ** (np.asarray(lv, np.float64) - 0.5)).astype(F32)
    return xw, normal, mf_max, np.zeros(len(u), F32), np.full(len(u), np.inf, F32)


# =================================================================================================================================
# Part 1: the stateless kernel
# =================================================================================================================================
def kf_grid(name):
    """(assign_min_x, assign_min_y, inv_w, inv_h, query_min_x, query_min_y) of a 1241 x 376 key frame.  plain / distorted are those
    of test_kf_matchers; positive has the int query origin below the float assign origin."""
    import test_kf_matchers as TK
    if name == "plain":
        return TK._kf_grid(False)[0]
    g = TK._kf_grid(True)[0]
    if name == "distorted":
        return g
    return (float(F32(3.7)), float(F32(2.6)), g[2], g[3], 3.0, 2.0)


def walk(grid, x, y, r):
    """window_walk's view of KeyFrame::GetFeaturesInArea(x, y, r) (src/KeyFrame.cc:569-606) on an oracle grid: one record per
    member in candidate order, dict(i = key point, col = cell column, rnd = round of 64 items within the column, lane, before =
    members counted when the round starts).  A column's items of the cell rows cy0 .. cy1 form the rounds, members or not."""
    g = grid.g
    x, y, r = F32(x), F32(y), F32(r)
    qx, qy, iw, ih = F32(g.min_x), F32(g.min_y), F32(g.inv_w), F32(g.inv_h)
    cx0 = max(0, int(np.floor((x - qx - r) * iw)))
    if cx0 >= 64: return []
    cx1 = min(63, int(np.ceil((x - qx + r) * iw)))
    if cx1 < 0: return []
    cy0 = max(0, int(np.floor((y - qy - r) * ih)))
    if cy0 >= 48: return []
    cy1 = min(47, int(np.ceil((y - qy + r) * ih)))
    if cy1 < 0: return []
    cs = np.ctypeslib.as_array(g.cell_start)
    out, n = [], 0
    for ix in range(cx0, cx1 + 1):
        s, e = int(cs[ix * 48 + cy0]), int(cs[ix * 48 + cy1 + 1])
        for j0 in range(s, e, 64):
            before = n
            for j in range(j0, min(j0 + 64, e)):
                i = int(grid.items[j])
                if abs(grid.kps["x"][i] - x) < r and abs(grid.kps["y"][i] - y) < r:
                    out.append(dict(i=i, col=ix, rnd=(j0 - s) // 64, lane=j - j0, before=before))
                    n += 1
    return out


def _round_edge(amin, inv, k):
    """the two neighbouring floats x_lo < x_hi with (x_lo - amin) * inv < k + 0.5 <= (x_hi - amin) * inv in float arithmetic"""
    amin, inv, half = F32(amin), F32(inv), F32(k + 0.5)
    t = lambda x: F32(F32(x - amin) * inv)
    x = F32((k + 0.5) / float(inv) + float(amin))
    while t(x) >= half: x = np.nextafter(x, F32(-np.inf))
    while t(np.nextafter(x, F32(np.inf))) < half: x = np.nextafter(x, F32(np.inf))
    return x, np.nextafter(x, F32(np.inf)), t


TH_KF = 8.0                     # th of every Part 1 search: r = 8 * 1.2**lv, exactly 8 on level 0
CLUSTER_LV = 2
BF = 8.0                        # Fuse: ur = u - bf * invz = u - 8
P_ = float(F32(1e-6))           # a permissive inv_level_sigma2 entry: no candidate of these windows is gated
INV_SIGMA2 = np.array([P_, P_, P_, np.nextafter(F32(5.99), F32(np.inf)), F32(5.99), P_, np.nextafter(F32(7.8), F32(0)), F32(7.8)], F32)


@functools.lru_cache(maxsize=None)
def kf_case(grid_name):
    rng = np.random.default_rng({"plain": 11, "distorted": 12, "positive": 13}[grid_name])
    grid = kf_grid(grid_name)
    amx, amy, iw, ih, qmx, qmy = grid
    book = Book(7)
    specs, tag_of = [], {}              # key points of the big frame: [x, y, octave, u_right], tag -> spec number
    order_pairs = []                    # (tag a, tag b): index(a) < index(b)

    def kp(tag, x, y, octave, u_right=-1.0):
        tag_of[tag] = len(specs); specs.append([F32(x), F32(y), octave, F32(u_right)])

    queries = {}                        # name -> dict(u, v, lv, q = book query, use)

    def query(name, u, v, lv, use=1):
        queries[name] = dict(u=F32(u), v=F32(v), lv=lv, q=book.query(), use=use)

    # ---- the cluster: one window of 130 members in two cell columns, with non-members in the same cells ----
    xb = 5.5 / iw + amx                                          # columns 5 | 6 of the assignment
    cu, cv = float(np.round(xb)), 100.0
    lat = lambda lo, hi: np.arange(np.ceil(lo * 8) / 8, hi, 0.125)
    ys = lat(cv - 11, cv + 11)
    for k, x in enumerate(rng.choice(lat(cu - 11, xb - 0.5), 70)): kp("cl.A%d" % k, x, rng.choice(ys), 2)
    for k, x in enumerate(rng.choice(lat(xb + 0.5, cu + 11), 60)): kp("cl.B%d" % k, x, rng.choice(ys), 2)
    for k, x in enumerate(rng.choice(lat(cu - 13, cu - 11.75), 12)): kp("cl.a%d" % k, x, rng.choice(ys), 2)
    for k, x in enumerate(rng.choice(lat(cu + 11.75, cu + 13), 6)): kp("cl.b%d" % k, x, rng.choice(ys), 2)
    for name in ("a1", "a2", "a3", "a4", "a5", "b1", "b2", "c1", "d50", "d51", "d100", "d101"):
        query(name, cu, cv, CLUSTER_LV)
    query("off", cu, cv, CLUSTER_LV, use=0)                      # use = 0: a copy of a1 that must stay -1

    # ---- small groups, one window each, 80 px apart ----
    slot = iter([(80.0 + 80 * k, gy) for gy in (200.0, 280.0) for k in range(14)])
    plants = []                                                  # (query, tag, distance)

    def group(name, lv, members, at=None, use=1):
        """members: (role, dx, dy, octave, distance or None, u_right or None)"""
        u, v = at if at is not None else next(slot)
        query(name, u, v, lv, use)
        for role, dx, dy, octave, d, ur in members:
            kp("%s.%s" % (name, role), F32(u) + F32(dx), F32(v) + F32(dy), octave, -1.0 if ur is None else ur)
            if d is not None: plants.append((name, "%s.%s" % (name, role), d))
        return u, v

    # (c) level edges
    group("c0", 0, [("on0", 1, 0, 0, 20, None), ("on1", -1, 0, 1, 10, None)])
    group("c7", 7, [("on7", 0.5, 0, 7, 20, None), ("on6", -0.5, 0, 6, 15, None), ("on5", 0, 0.5, 5, 10, None)])
    # (e) window edges on level 0: r = 8
    inside = lambda c: float(np.nextafter(F32(c + 8), F32(0))) - c      # the last float below c + 8, minus c: exact in float
    group("ex", 0, [("at", 8, 0, 0, 10, None), ("in", inside(560.0), 0, 0, 20, None)], at=(560.0, 340.0))
    group("ey", 0, [("at", 0, 8, 0, 10, None), ("in", 0, inside(248.0), 0, 20, None)], at=(720.0, 248.0))
    group("clamp", 0, [("in", -1.5, -1.5, 0, 20, None)], at=(qmx + 5.0, qmy + 5.0))
    for name, (u, v) in dict(offl=(qmx - 60, 150.0), offr=(qmx + 64 / iw + 60, 150.0), offt=(600.0, qmy - 60),
                             offb=(600.0, qmy + 48 / ih + 60)).items():
        query(name, float(np.round(u)), float(np.round(v)), 0)
    x_lo, x_hi, _ = _round_edge(amx, iw, 20)
    for name, xa, gy in (("rlo", x_lo, 330.0), ("rhi", x_hi, 40.0)):
        u = float(np.round(xa)) + 1.0
        group(name, 0, [("edge", float(xa) - u, 0, 0, 20, None), ("right", float(F32(xa + F32(3))) - u, 0, 0, 20, None)], at=(u, gy))
        order_pairs.append((name + ".right", name + ".edge"))
    # (f) degenerate windows
    query("empty", 900.0, 340.0, 0)
    group("one", 2, [("only", 2, -1, 2, 20, None)])
    group("none", 2, [("lo", 1, 0, 0, 10, None), ("hi", -1, 1, 3, 10, None)])
    # (g) Fuse's gate: e2 == 1 and er == 0 exactly, the table value is the product
    near = lambda octave, ur: ("near", -1, 0, octave, 10, ur)
    far = lambda octave: ("far", 0.5, 0, octave, 30, None)
    for name, lv, octave, stereo in (("g599", 4, 4, None), ("g599up", 3, 3, None), ("g78dn", 6, 6, 0.0), ("g78", 7, 7, 0.0), ("ger", 6, 6, -1.0)):
        u, v = next(slot)
        group(name, lv, [near(octave, None if stereo is None else u - BF + stereo), far(octave - 1)], at=(u, v))
    group("gzero", 6, [near(6, 0.0), far(5)], at=(BF, 200.0 + 80 * 2))                               # ur = 8 - 8 = 0 == u_right
    # (h) the first of a tie is dropped by the gate
    group("h", 3, [("first", -1, 0, 3, 20, None), ("second", 0.5, 0, 3, 20, None)])
    order_pairs.append(("h.first", "h.second"))
    # (i) SearchBySim3's agreement
    group("cross", 0, [("only", 1, 1, 0, 20, None)])
    group("nouse", 0, [("only", 1, 1, 0, 20, None)])
    group("off2", 0, [("only", 1, 1, 0, 20, None)], use=0)

    # ---- background, index order ----
    while len(specs) < 204:
        kp("bg%d" % len(specs), rng.uniform(40, 1200), rng.choice([20.0, 60.0, 360.0]), int(rng.integers(0, 8)))
    n = len(specs)
    index = rng.permutation(n)                                   # spec number -> key-point index
    for a, b in order_pairs:
        ia, ib = tag_of[a], tag_of[b]
        if index[ia] > index[ib]: index[ia], index[ib] = index[ib], index[ia]
    idx = {t: int(index[s]) for t, s in tag_of.items()}
    rows = [None] * n
    for s, sp in enumerate(specs): rows[index[s]] = sp
    kps = kp_array([(r[0], r[1], r[2]) for r in rows])
    ur_kf = np.array([r[3] for r in rows], F32)

    # ---- planted positions of the cluster queries ----
    r_cl = F32(TH_KF) * SF[CLUSTER_LV]
    recs = walk(O.KeyFrameGrid(kps, grid), cu, cv, r_cl)
    colA, colB = recs[0]["col"], recs[-1]["col"]
    slotpos = lambda p: recs[p]["before"] + recs[p]["lane"]      # the lane's slot in its round: not the position, and ordered differently
    taken = set()

    def pick(pred, after=-1):
        for p in range(after + 1, len(recs)):
            if p not in taken and pred(p, recs[p]):
                taken.add(p); return p
        raise AssertionError("no such position in the cluster")

    pos = {}
    p1 = pick(lambda p, c: c["col"] == colA and c["rnd"] == 0 and c["lane"] >= 3)
    pos["a1"] = (p1, pick(lambda p, c: c["col"] == colA and c["rnd"] == 0 and c["lane"] > recs[p1]["lane"] + 5))
    p1 = pick(lambda p, c: c["col"] == colA and c["rnd"] == 0 and c["lane"] >= 20)
    pos["a2"] = (p1, pick(lambda p, c: c["col"] == colA and c["rnd"] == 1 and c["lane"] != recs[p1]["lane"]))
    p1 = pick(lambda p, c: c["col"] == colA and c["rnd"] == 1)
    pos["a3"] = (p1, pick(lambda p, c: c["col"] == colB and c["rnd"] == 0 and c["lane"] >= 10))
    lanesB = {c["lane"] for c in recs if c["col"] == colB and c["rnd"] == 0}
    p1 = pick(lambda p, c: c["col"] == colA and c["rnd"] == 0 and c["lane"] >= 30 and c["lane"] in lanesB)
    pos["a4"] = (p1, pick(lambda p, c: c["col"] == colB and c["rnd"] == 0 and c["lane"] == recs[p1]["lane"]))
    first_r1 = min(p for p, c in enumerate(recs) if c["col"] == colA and c["rnd"] == 1)
    p2 = pick(lambda p, c: c["col"] == colA and c["rnd"] == 1 and p > first_r1)
    pos["a5"] = (pick(lambda p, c: c["col"] == colA and c["rnd"] == 0 and slotpos(p) > slotpos(p2)), p2)
    p1 = pick(lambda p, c: c["col"] == colA and c["lane"] >= 40)
    pos["b1"] = (p1, pick(lambda p, c: True, after=p1))
    p1 = pick(lambda p, c: c["col"] == colA and c["lane"] >= 45)
    pos["b2"] = (p1, pick(lambda p, c: c["col"] == colB))
    for name in ("c1", "d50", "d51", "d100", "d101"):
        pos[name] = (pick(lambda p, c: c["lane"] >= 50 or c["col"] == colB),)
    for p, c in enumerate(recs):                                 # octaves: the unplanted members hold positions on every level
        kps["octave"][c["i"]] = 2 if p in taken else [0, 1, 2, 2, 3][p % 5]
    retag = lambda p, t: idx.__setitem__(t, recs[p]["i"])
    for name, roles, octs, dists in (("a1", ("first", "second"), (2, 2), (20, 20)), ("a2", ("first", "second"), (2, 2), (20, 20)),
                                     ("a3", ("first", "second"), (2, 2), (20, 20)), ("a4", ("first", "second"), (2, 2), (20, 20)),
                                     ("a5", ("first", "second"), (2, 2), (20, 20)), ("b1", ("first", "second"), (3, 2), (20, 20)),
                                     ("b2", ("first", "second"), (0, 1), (20, 20)), ("c1", ("only",), (1,), (20,)),
                                     ("d50", ("only",), (2,), (50,)), ("d51", ("only",), (2,), (51,)), ("d100", ("only",), (2,), (100,)),
                                     ("d101", ("only",), (2,), (101,))):
        for p, role, octave, d in zip(pos[name], roles, octs, dists):
            retag(p, "%s.%s" % (name, role))
            kps["octave"][recs[p]["i"]] = octave
            plants.append((name, "%s.%s" % (name, role), d))
    plants += [("off", "a1.first", 20), ("off", "a1.second", 20)]      # the unused copy of a1 would find a1's candidates

    # ---- descriptors ----
    off_q = queries["off"]["q"]
    book.q[off_q] = book.q[queries["a1"]["q"]].copy(); book.family[off_q] = book.family[queries["a1"]["q"]]
    tbits = np.stack([book.background() for _ in range(n)])
    for name, tag, d in plants:
        if name != "off":
            tbits[idx[tag]] = book.plant(queries[name]["q"], d)
    names = list(queries)
    # interleave the unused entries with the used ones
    names.remove("off"); names.remove("off2")
    names.insert(2, "off"); names.insert(9, "off2")
    u = np.array([queries[q]["u"] for q in names], F32); v = np.array([queries[q]["v"] for q in names], F32)
    lv = np.array([queries[q]["lv"] for q in names], np.int32)
    use = np.array([queries[q]["use"] for q in names], np.uint8)
    qdesc = book.queries()[[queries[q]["q"] for q in names]]
    xw, normal, mf_max, min_inv, max_inv = mappoints(u, v, lv)
    fx = dict(grid_name=grid_name, grid=grid, kps=kps, ur_kf=ur_kf, desc=pack(tbits), idx=idx, names=names, u=u, v=v, lv=lv, use=use,
              qdesc=qdesc, xw=xw, normal=normal, mf_max=mf_max, min_inv=min_inv, max_inv=max_inv, plants=plants,
              cluster=dict(u=cu, v=cv, r=float(r_cl), recs=recs, pos=pos, cols=(colA, colB), slotpos=slotpos),
              round_edge=(x_lo, x_hi), th=TH_KF, bf=BF, inv_sigma2=INV_SIGMA2, sf=SF)

    # ---- the second key frame of SearchBySim3: one key point per query, 60 px apart, on the plain grid; the MapPoint of every
    # planted key point of the big frame projects onto the key point of its query and carries that key point's descriptor ----
    nq = len(names)
    small = kp_array([(30.0 + 60 * (i % 20), 30.0 + 60 * (i // 20), 0) for i in range(nq)])
    sbits = 1 - np.stack([_hadamard()[40 + i] for i in range(nq)])
    owner = np.full(n, -1)
    for name, tag, d in plants:
        if name != "off": owner[idx[tag]] = names.index(name)
    owner[idx["cross.only"]] = names.index("empty")              # i1 -> i2, but i2 -> another key point of the small frame
    use_b = (owner >= 0).astype(np.uint8)
    use_b[idx["nouse.only"]] = 0                                 # i1 -> i2, but i2 has no usable MapPoint
    for t in sorted(t for t in idx if t.startswith("bg")):       # usable MapPoints that find nothing, until nq2 is odd and != nq1
        if use_b.sum() % 2 == 1 and use_b.sum() != use.sum(): break
        use_b[idx[t]] = 1
    ub = np.where(owner >= 0, small["x"][np.maximum(owner, 0)], F32(1100.0)).astype(F32)
    vb = np.where(owner >= 0, small["y"][np.maximum(owner, 0)], F32(350.0)).astype(F32)
    bdesc = np.where((owner >= 0)[:, None], pack(sbits)[np.maximum(owner, 0)], np.uint8(0)).astype(np.uint8)
    bxw, _, bmf, bmin, bmax = mappoints(ub, vb, np.zeros(n))
    fx["small"] = dict(kps=small, desc=pack(sbits), grid=kf_grid("plain"), owner=owner, use=use_b, u=ub, v=vb, lv=np.zeros(n, np.int32),
                       mp_desc=bdesc, xw=bxw, mf_max=bmf, min_inv=bmin, max_inv=bmax)
    return fx


def kf_subset(fx, k):
    """use flags with only the first k usable queries left"""
    use = fx["use"].copy()
    use[np.nonzero(use)[0][k:]] = 0
    return use


def oracle_fuse(fx, use=None):
    og = O.KeyFrameGrid(fx["kps"], fx["grid"])
    return O.fuse(fx["use"] if use is None else use, fx["xw"], fx["normal"], fx["min_inv"], fx["max_inv"], fx["mf_max"], fx["qdesc"],
                  np.eye(4, dtype=F32), np.zeros(3, F32), KID, fx["bf"], WIDE, fx["sf"], fx["inv_sigma2"], LOGSF, og, fx["ur_kf"],
                  fx["desc"], fx["th"])


def oracle_fuse_sim3(fx, use=None):
    og = O.KeyFrameGrid(fx["kps"], fx["grid"])
    return O.fuse_sim3(fx["use"] if use is None else use, fx["xw"], fx["normal"], fx["min_inv"], fx["max_inv"], fx["mf_max"], fx["qdesc"],
                       np.eye(4, dtype=F32), KID, WIDE, fx["sf"], LOGSF, og, fx["desc"], fx["th"])


def sim3_sides(fx, big_first, n_small=None):
    """the two key frames of a SearchBySim3 call as dicts: the arrays of both the oracle's and the library's entry"""
    s = fx["small"]
    m = len(s["kps"]) if n_small is None else n_small
    small = dict(usable=fx["use"][:m], xw=fx["xw"][:m], min_inv=fx["min_inv"][:m], max_inv=fx["max_inv"][:m], mf_max=fx["mf_max"][:m],
                 mp_desc=fx["qdesc"][:m], u=fx["u"][:m], v=fx["v"][:m], lv=fx["lv"][:m], kps=s["kps"][:m], desc=s["desc"][:m], grid_t=s["grid"])
    big = dict(usable=s["use"], xw=s["xw"], min_inv=s["min_inv"], max_inv=s["max_inv"], mf_max=s["mf_max"], mp_desc=s["mp_desc"], u=s["u"],
               v=s["v"], lv=s["lv"], kps=fx["kps"], desc=fx["desc"], grid_t=fx["grid"])
    for sd in (small, big):
        sd.update(Tw=np.eye(4, dtype=F32), bounds=WIDE, sf=fx["sf"], log_sf=LOGSF)
    return (big, small) if big_first else (small, big)


def oracle_sim3(fx, big_first, n_small=None):
    s1, s2 = sim3_sides(fx, big_first, n_small)
    for sd in (s1, s2): sd["grid"] = O.KeyFrameGrid(sd["kps"], sd["grid_t"])
    return O.search_by_sim3(s1, s2, KID, 1.0, np.eye(3, dtype=F32), np.zeros(3, F32), fx["th"])


# =================================================================================================================================
# Part 2: the sequential scans, one small frame each
# =================================================================================================================================
FRAME_BOUNDS = (0.0, 640.0, 0.0, 480.0)         # Frame grid: 10 x 10 px cells
TH = 8.0                                        # r = 8 * 1.2**octave


class Planted:
    """Key points of one frame in insertion order (= index order) and the distances planted on them."""

    def __init__(self, seed):
        self.book = Book(seed)
        self.rows, self.tag, self.plants, self.q = [], {}, [], {}

    def query(self, name, of=None, bits=()):
        self.q[name] = self.book.query() if of is None else self.book.variant(self.q[of], bits)

    def kp(self, tag, x, y, octave=0, angle=0.0, near=None, reserved=()):
        """near = (query, distance): the descriptor is planted at that distance from the query"""
        self.tag[tag] = len(self.rows); self.rows.append((x, y, octave, angle))
        if near: self.plants.append((near[0], tag, near[1], reserved))

    def finish(self):
        kps = kp_array(self.rows)
        bits = np.stack([self.book.background() for _ in self.rows])
        for q, t, d, reserved in self.plants: bits[self.tag[t]] = self.book.plant(self.q[q], d, reserved)
        names = list(self.q)
        fam = np.array([self.book.family[self.q[n]] for n in names])
        owner = np.full(len(kps), -1)                            # family a key point is planted for
        for q, t, d, _ in self.plants: owner[self.tag[t]] = self.book.family[self.q[q]]
        return dict(kps=kps, desc=pack(bits), names=names, qdesc=self.book.queries()[[self.q[n] for n in names]], tag=dict(self.tag),
                    plants=[(q, t, d) for q, t, d, _ in self.plants], related=fam[:, None] == owner[None, :])


def _lone(P, name, x, y, d=10, octave=0, angle=0.0):
    P.query(name)
    P.kp(name + ".only", x + 1.0, y + 0.5, octave, angle, near=(name, d))


@functools.lru_cache(maxsize=None)
def sim3proj_case():
    """SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:370-398), th = 8, every MapPoint on level 0."""
    P = Planted(21)
    at = {}
    for name, of, xy in (("A", None, (100, 100)), ("B", "A", (100, 100)), ("C", None, (200, 100)), ("D", "C", (200, 100)), ("E", None, (300, 100)),
                         ("F", None, (400, 100)), ("X", None, (500, 100))):
        P.query(name, of, (0, 1)); at[name] = xy
    P.kp("s1", 101, 100, near=("A", 10)); P.kp("s2", 99, 100, near=("B", 50))
    P.kp("t1", 201, 100, near=("C", 10)); P.kp("t2", 199, 100, near=("D", 51))
    P.kp("p1", 301, 100, near=("E", 5)); P.kp("p2", 299, 100, near=("E", 20))
    P.kp("r0", 400.5, 100, 2, near=("F", 5)); P.kp("r1", 401, 100, near=("F", 15)); P.kp("r2", 401.5, 100, near=("F", 15))
    P.kp("x1", 501, 100, near=("X", 5))
    for k in range(12): P.kp("bg%d" % k, 50.0 + 45 * k, 300.0, k % 4)
    fx = P.finish()
    u = np.array([at[n][0] for n in fx["names"]], F32); v = np.array([at[n][1] for n in fx["names"]], F32)
    lv = np.zeros(len(u), np.int32)
    xw, normal, mf_max, min_inv, max_inv = mappoints(u, v, lv)
    matched = np.zeros(len(fx["kps"]), np.uint8); matched[fx["tag"]["p1"]] = 1
    use = np.array([n != "X" for n in fx["names"]], np.uint8)
    fx.update(u=u, v=v, lv=lv, xw=xw, normal=normal, mf_max=mf_max, min_inv=min_inv, max_inv=max_inv, matched=matched, use=use, th=8,
              grid=(0.0, 0.0, float(F32(64) / F32(640)), float(F32(48) / F32(480)), 0.0, 0.0))
    return fx


def oracle_sim3proj(fx):
    matched = fx["matched"].copy()
    km, n = O.search_by_projection_sim3(fx["use"], fx["xw"], fx["normal"], fx["min_inv"], fx["max_inv"], fx["mf_max"], fx["qdesc"],
                                        np.eye(4, dtype=F32), KID, WIDE, SF, LOGSF, O.KeyFrameGrid(fx["kps"], fx["grid"]), fx["desc"], matched, fx["th"])
    return km, n, matched


@functools.lru_cache(maxsize=None)
def init_case():
    """SearchForInitialization (src/ORBmatcher.cc:425-516): nnratio = 0.5 (exact in float), windowSize = 8.  Frame 1's key points are
    the queries, in this order; vbPrevMatched holds the window centres."""
    P = Planted(22)
    f1 = []                                                      # (name, octave, angle, prev x, prev y)

    def q(name, x, y, octave=0, angle=0.0, of=None, bits=()):
        P.query(name, of, bits); f1.append((name, octave, angle, float(x), float(y)))

    q("A", 100, 100, angle=90.0)                                 # matches s at 20, then loses it to B
    q("C", 200, 100)                                             # matches s1 at 20 and keeps it
    q("R10", 300, 100); q("R9", 400, 100); q("R11", 500, 100)    # best < second * 0.5 at 10, 9 and 11 against 20
    q("E", 100, 200, octave=1)                                   # never queried
    q("B", 100, 100, of="A", bits=(0, 1, 2, 3, 4))               # 15 from s: steals it
    q("D", 210, 100, of="C", bits=(0, 1))                        # 20 from s1 as well: no steal, and s1 is no second-best for D
    for k in range(2): q("b1_%d" % k, 100 + 100 * k, 300, angle=30.0)
    for k in range(2): q("b2_%d" % k, 300 + 100 * k, 300, angle=60.0)
    q("G", 500, 300, angle=150.0)                                # alone in bin 5: culled with mbCheckOrientation
    P.kp("s", 101, 100.5, near=("B", 15))
    P.kp("s1", 205, 100.5, near=("C", 20), reserved=(0,)); P.kp("s2", 214, 100.5, near=("D", 21))
    px = {n: x for n, _, _, x, _ in f1}
    for name, d in (("R10", 10), ("R9", 9), ("R11", 11)):
        x = px[name]
        P.kp(name + ".best", x + 1, 100.5, near=(name, d)); P.kp(name + ".second", x - 1, 100.5, near=(name, 20))
    P.kp("e", 101, 200.5, 1, near=("E", 0))
    for name, _, _, x, y in f1[8:]:
        P.kp(name + ".only", x + 1, y + 0.5, near=(name, 10))
    for k in range(10): P.kp("bg%d" % k, 60.0 + 50 * k, 420.0, k % 3)
    fx = P.finish()
    order = [fx["names"].index(n) for n, *_ in f1]
    assert order == list(range(len(f1)))
    kps1 = kp_array([(x, y, octave, angle) for _, octave, angle, x, y in f1])
    fx.update(kps1=kps1, prev=np.ascontiguousarray(np.stack([kps1["x"], kps1["y"]], 1), F32), window=8, nnratio=0.5)
    return fx


def oracle_init(fx, check_ori):
    prev = fx["prev"].copy()
    m12, n = O.search_for_initialization(fx["kps1"], fx["qdesc"], O.FrameGrid(fx["kps"], *FRAME_BOUNDS), fx["desc"], prev, fx["window"],
                                         fx["nnratio"], check_ori)
    return m12, n, prev


LAST_MODES = {"neither": 0.0, "forward": -1.0, "backward": 1.0}      # tz of Tcw; Tlw = I, mb = 0.5: tlc.z = -tz


@functools.lru_cache(maxsize=None)
def last_case():
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1396-1466): th = 8, mbf = 16 (ur = u - 16), the last
    frame's features are the queries, in this order."""
    P = Planted(23)
    last = []                                                    # (name, octave, angle, u, v, mp_obs, has_point)

    def q(name, u, v, octave=0, angle=0.0, obs=1, has=1, of=None):
        P.query(name, of, (0,)); last.append((name, octave, angle, float(u), float(v), obs, has))

    q("blk", 100, 100); q("zero", 200, 100, obs=3)
    q("P", 300, 100, obs=0); q("Q", 300, 100, obs=0, of="P")                           # one slot, two assignments, both stay
    q("P2", 400, 100, angle=150.0, obs=0); q("Q2", 400, 100, angle=150.0, obs=0, of="P2")   # one slot, two assignments, both culled
    q("Uk", 500, 100); q("Ud", 100, 200); q("Uz", 200, 200)
    q("O", 300, 200, octave=2)
    q("T100", 400, 200); q("T101", 500, 200)
    for k in range(3): q("b1_%d" % k, 100 + 100 * k, 300, angle=30.0)
    for k in range(3): q("b2_%d" % k, 400 + 100 * (k % 2), 300 + 100 * (k // 2), angle=60.0)
    q("nopoint", 100, 400, has=0)
    ur = {}
    P.kp("blk.x1", 101, 100, near=("blk", 5)); P.kp("blk.x2", 99, 100, near=("blk", 20))
    P.kp("zero.z1", 201, 100, near=("zero", 10))
    P.kp("s", 301, 100, near=("P", 10)); P.kp("s2", 401, 100, near=("P2", 10))
    P.kp("Uk.g", 501, 100, near=("Uk", 10)); ur["Uk.g"] = 500.0 - 16 - 8                     # er == radius: kept
    P.kp("Uk.o", 499, 100, near=("Uk", 20))
    P.kp("Ud.g", 101, 200, near=("Ud", 10)); ur["Ud.g"] = float(np.nextafter(F32(100.0 - 16 - 8), F32(0)))     # er just above: dropped
    P.kp("Ud.o", 99, 200, near=("Ud", 20))
    P.kp("Uz.g", 201, 200, near=("Uz", 10)); ur["Uz.g"] = 0.0                                # u_right == 0 is not gated (`> 0`)
    for octave, d, dx in ((0, 10, -2), (1, 15, -1), (2, 30, 0), (3, 25, 1), (4, 20, 2)):
        P.kp("O.o%d" % octave, 300 + dx, 200.5, octave, near=("O", d))
    P.kp("T100.only", 401, 200, near=("T100", 100)); P.kp("T101.only", 501, 200, near=("T101", 101))
    for name, _, _, u, v, _, _ in last[12:]:
        P.kp(name + ".only", u + 1, v + 0.5, near=(name, 10 if name != "nopoint" else 0))
    for k in range(8): P.kp("bg%d" % k, 60.0 + 60 * k, 450.0, k % 3)
    fx = P.finish()
    assert fx["names"] == [r[0] for r in last]
    n2 = len(fx["kps"])
    u_right = np.full(n2, -1, F32)
    for t, val in ur.items(): u_right[fx["tag"][t]] = val
    cur_obs = np.full(n2, -1, np.int32); cur_obs[fx["tag"]["blk.x1"]] = 2; cur_obs[fx["tag"]["zero.z1"]] = 0
    kps_last = kp_array([(u, v, octave, angle) for _, octave, angle, u, v, _, _ in last])
    fx.update(kps_last=kps_last, uv=np.array([(r[3], r[4]) for r in last], F32), mp_obs=np.array([r[5] for r in last], np.int32),
              has=np.array([r[6] for r in last], np.uint8), u_right=u_right, cur_obs=cur_obs, th=TH, mb=0.5, mbf=16.0)
    return fx


def last_pose(fx, mode):
    """(xw, Tcw, Tlw): zc = xw.z + tz = 1 in every mode, so u, v and invzc are the planted ones"""
    tz = LAST_MODES[mode]
    xw = np.concatenate([fx["uv"], np.full((len(fx["uv"]), 1), 1.0 - tz, F32)], 1).astype(F32)
    Tcw = np.eye(4, dtype=F32); Tcw[2, 3] = tz
    return xw, Tcw, np.eye(4, dtype=F32)


def oracle_last(fx, mode, check_ori):
    xw, Tcw, Tlw = last_pose(fx, mode)
    cur_obs = fx["cur_obs"].copy()
    cm, n = O.search_by_projection_last(fx["has"], xw, fx["qdesc"], fx["mp_obs"], fx["kps_last"], Tcw, Tlw, KID, fx["mb"], fx["mbf"], WIDE, SF,
                                        O.FrameGrid(fx["kps"], *FRAME_BOUNDS), fx["desc"], cur_obs, fx["th"], False, check_ori, fx["u_right"])
    return cm, n, cur_obs


@functools.lru_cache(maxsize=None)
def map_case():
    """SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:73-122): th = 1 (no factor), nnratio = 0.5; r = 4 * 1.2**level, or
    2.5 * 1.2**level when viewCos > 0.998."""
    P = Planted(24)
    mp = []                                                      # (name, x, y, level, view_cos, proj_xr, in_view)
    c998 = F32(0.998)

    def q(name, x, y, lv=0, vc=0.99, xr=0.0, in_view=1):
        P.query(name); mp.append((name, float(x), float(y), lv, F32(vc), float(xr), in_view))

    q("Req", 100, 100, lv=1); q("Rdiff", 200, 100, lv=1)
    q("Vc", 300, 100, vc=c998); q("Vlo", 400, 100, vc=np.nextafter(c998, F32(0))); q("Vhi", 500, 100, vc=np.nextafter(c998, F32(1)))
    q("T100", 100, 200); q("T101", 200, 200)
    q("XRk", 300, 200, xr=284.0); q("XRd", 400, 200, xr=384.0)
    q("Blk", 500, 200)
    q("unseen", 100, 300, in_view=0)
    ur = {}
    P.kp("Req.best", 101, 100, 1, near=("Req", 20)); P.kp("Req.second", 99, 100, 1, near=("Req", 30))
    P.kp("Rdiff.best", 201, 100, 1, near=("Rdiff", 20)); P.kp("Rdiff.second", 199, 100, 0, near=("Rdiff", 30))
    for name in ("Vc", "Vlo", "Vhi"):                            # 3 px away: inside r = 4, outside r = 2.5
        P.kp(name + ".only", dict((m[0], m[1]) for m in mp)[name] + 3, 100, near=(name, 10))
    P.kp("T100.only", 101, 200, near=("T100", 100)); P.kp("T101.only", 201, 200, near=("T101", 101))
    P.kp("XRk.g", 301, 200, near=("XRk", 10)); ur["XRk.g"] = 280.0                           # er == r == 4: kept
    P.kp("XRk.o", 299, 200, near=("XRk", 20))
    P.kp("XRd.g", 401, 200, near=("XRd", 10)); ur["XRd.g"] = float(np.nextafter(F32(380.0), F32(0)))       # er just above 4: dropped
    P.kp("XRd.o", 399, 200, near=("XRd", 20))
    P.kp("Blk.taken", 501, 200, near=("Blk", 5)); P.kp("Blk.free", 499, 200, near=("Blk", 20))
    P.kp("unseen.only", 101, 300, near=("unseen", 0))
    for k in range(8): P.kp("bg%d" % k, 60.0 + 60 * k, 450.0, k % 3)
    fx = P.finish()
    n2 = len(fx["kps"])
    u_right = np.full(n2, -1, F32)
    for t, val in ur.items(): u_right[fx["tag"][t]] = val
    cur_obs = np.full(n2, -1, np.int32); cur_obs[fx["tag"]["Blk.taken"]] = 1
    fx.update(px=np.array([m[1] for m in mp], F32), py=np.array([m[2] for m in mp], F32), lv=np.array([m[3] for m in mp], np.int32),
              vc=np.array([m[4] for m in mp], F32), pxr=np.array([m[5] for m in mp], F32), in_view=np.array([m[6] for m in mp], np.uint8),
              mp_obs=np.arange(1, len(mp) + 1, dtype=np.int32), u_right=u_right, cur_obs=cur_obs, th=1.0, nnratio=0.5)
    return fx


def oracle_map(fx):
    cur_obs = fx["cur_obs"].copy()
    cm, n = O.search_by_projection_map(fx["in_view"], fx["px"], fx["py"], fx["lv"], fx["vc"], fx["qdesc"], fx["mp_obs"], SF,
                                       O.FrameGrid(fx["kps"], *FRAME_BOUNDS), fx["desc"], cur_obs, fx["th"], fx["nnratio"], fx["pxr"], fx["u_right"])
    return cm, n, cur_obs


@functools.lru_cache(maxsize=None)
def kfproj_case():
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1538-1596): th = 8, ORBdist = 64."""
    P = Planted(25)
    mp = []                                                      # (name, u, v, level, key-frame angle, usable)

    def q(name, u, v, lv=0, angle=0.0, use=1):
        P.query(name); mp.append((name, float(u), float(v), lv, angle, use))

    q("Hblk", 100, 100); q("T64", 200, 100); q("T65", 300, 100); q("Lv", 400, 100, lv=3); q("Lv2", 500, 100, lv=3)
    for k in range(2): q("b1_%d" % k, 100 + 100 * k, 300, angle=30.0)
    for k in range(2): q("b2_%d" % k, 300 + 100 * k, 300, angle=60.0)
    q("Cull", 500, 300, angle=150.0)
    q("unused", 100, 400, use=0)
    P.kp("Hblk.taken", 101, 100, near=("Hblk", 5)); P.kp("Hblk.free", 99, 100, near=("Hblk", 20))
    P.kp("T64.only", 201, 100, near=("T64", 64)); P.kp("T65.only", 301, 100, near=("T65", 65))
    for octave, d, dx in ((1, 5, -2), (5, 6, -1), (4, 15, 1), (2, 20, 2)): P.kp("Lv.o%d" % octave, 400 + dx, 100.5, octave, near=("Lv", d))
    for octave, d, dx in ((1, 5, -1), (2, 20, 1)): P.kp("Lv2.o%d" % octave, 500 + dx, 100.5, octave, near=("Lv2", d))
    for name, u, v, _, _, _ in mp[5:]:
        P.kp(name + ".only", u + 1, v + 0.5, near=(name, 10 if name != "unused" else 0))
    for k in range(8): P.kp("bg%d" % k, 60.0 + 60 * k, 450.0, k % 3)
    fx = P.finish()
    u = np.array([m[1] for m in mp], F32); v = np.array([m[2] for m in mp], F32); lv = np.array([m[3] for m in mp], np.int32)
    xw, _, mf_max, min_inv, max_inv = mappoints(u, v, lv)
    has = np.zeros(len(fx["kps"]), np.uint8); has[fx["tag"]["Hblk.taken"]] = 1
    fx.update(u=u, v=v, lv=lv, xw=xw, mf_max=mf_max, min_inv=min_inv, max_inv=max_inv, kf_angle=np.array([m[4] for m in mp], F32),
              use=np.array([m[5] for m in mp], np.uint8), has=has, th=TH, orb_dist=64)
    return fx


def oracle_kfproj(fx, check_ori):
    has = fx["has"].copy()
    cm, n = O.search_by_projection_kf(fx["use"], fx["xw"], fx["min_inv"], fx["max_inv"], fx["mf_max"], fx["qdesc"], fx["kf_angle"],
                                      np.eye(4, dtype=F32), KID, WIDE, SF, LOGSF, O.FrameGrid(fx["kps"], *FRAME_BOUNDS), fx["desc"], has, fx["th"],
                                      fx["orb_dist"], check_ori)
    return cm, n, has
