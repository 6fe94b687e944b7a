"""Client of oracle/_ref/ref_orbx: the reference's own src/ORBextractor.cc, compiled unmodified on the OpenCV shim
(oracle/ref/).  The executable reads a batch of cases from a request file and writes a response file (format in
oracle/ref/ref_orbx.cc).  Used by tests/test_reference_pin_cpu.py and tests/test_reference_pin_gpu.py."""
import os
import struct
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle_lib import KP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(REF_OUT, "ref_orbx")
EXE_UBSAN = os.path.join(REF_OUT, "ref_orbx_ubsan")

TABLES, PYRAMID, LEVELS, OCTREE, EXTRACT = range(5)
MAX_PROCS = 16


def reference_dir():
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", os.path.join(ROOT, "oracle", "ref"),
                                   "print-ref-dir"], text=True)
    return out.strip()


def ensure(allow_build=True):
    """Path to ref_orbx, building it when it is missing and the reference exists; None when neither exists."""
    if os.path.exists(EXE) and os.path.exists(EXE_UBSAN):
        return EXE
    if allow_build and os.path.exists(os.path.join(reference_dir(), "src", "ORBextractor.cc")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")])
        return EXE
    return None


class Case:
    """One request.  params = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, blur_mode)."""

    def __init__(self, mode, params, img=None, cands=None, bounds=None, N=None):
        self.mode, self.params = mode, tuple(params)
        nf, sf, nl, ini, mn, blur = self.params
        b = struct.pack("<iifiiii", mode, nf, sf, nl, ini, mn, blur)
        if mode in (PYRAMID, LEVELS, EXTRACT):
            img = np.ascontiguousarray(img, dtype=np.uint8)
            b += struct.pack("<ii", img.shape[1], img.shape[0]) + img.tobytes()
        elif mode == OCTREE:
            c = np.ascontiguousarray(cands, dtype=np.dtype([("x", "<i4"), ("y", "<i4"), ("response", "<i4")]))
            minX, maxX, minY, maxY = bounds
            b += struct.pack("<iiiiii", len(c), minX, maxX, minY, maxY, N) + c.tobytes()
        self.blob = b


class _Reader:
    def __init__(self, data):
        self.d, self.o = data, 0

    def take(self, n):
        assert self.o + n <= len(self.d), "truncated ref_orbx response"
        v = self.d[self.o:self.o + n]
        self.o += n
        return v

    def i32(self):
        return struct.unpack("<i", self.take(4))[0]

    def arr(self, dtype, n):
        dt = np.dtype(dtype)
        return np.frombuffer(self.take(dt.itemsize * n), dtype=dt).copy()

    def kps(self):
        return self.arr(KP_DTYPE, self.i32())


def _parse(case, r):
    mode = r.i32()
    assert mode == case.mode, "response out of step"
    nl = case.params[2]
    if mode == TABLES:
        t = {k: r.arr("<f4", nl) for k in ("scale", "inv_scale", "sigma2", "inv_sigma2")}
        t["quota"] = r.arr("<i4", nl)
        t["umax"] = r.arr("<i4", r.i32())
        t["pattern"] = r.arr("<i4", 2 * r.i32()).reshape(-1, 2)
        return t
    if mode == PYRAMID:
        out = []
        for _ in range(nl):
            rows, cols = r.i32(), r.i32()
            out.append(r.arr(np.uint8, rows * cols).reshape(rows, cols))
        return out
    if mode == LEVELS:
        return [r.kps() for _ in range(nl)]
    if mode == OCTREE:
        return r.kps()
    k = r.kps()
    return k, r.arr(np.uint8, 32 * len(k)).reshape(-1, 32)


def run(cases, exe=None):
    """Runs the cases in one ref_orbx process; returns one result per case.  A non-zero exit raises
    CalledProcessError (the UBSan build exits non-zero at the first undefined operation)."""
    exe = exe or EXE
    if not cases:
        return []
    with tempfile.TemporaryDirectory(prefix="ref_orbx_") as d:
        req, resp = os.path.join(d, "req.bin"), os.path.join(d, "resp.bin")
        with open(req, "wb") as f:
            f.write(struct.pack("<ii", 0x5142524F, len(cases)))
            for c in cases:
                f.write(c.blob)
        p = subprocess.run([exe, req, resp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise subprocess.CalledProcessError(p.returncode, [exe], p.stdout, p.stderr)
        with open(resp, "rb") as f:
            r = _Reader(f.read())
    assert r.i32() == 0x5252424F
    out = [_parse(c, r) for c in cases]
    assert r.o == len(r.d), "trailing bytes in the ref_orbx response"
    return out


def run_parallel(cases, exe=None, procs=None):
    """Splits the cases over up to MAX_PROCS ref_orbx processes (round-robin, so large cases spread out)."""
    procs = procs or max(1, min(MAX_PROCS, os.cpu_count() or 1, len(cases)))
    parts = [list(range(i, len(cases), procs)) for i in range(procs)]
    with ThreadPoolExecutor(procs) as pool:
        res = list(pool.map(lambda ix: run([cases[i] for i in ix], exe), parts))
    out = [None] * len(cases)
    for ix, rr in zip(parts, res):
        for i, v in zip(ix, rr):
            out[i] = v
    return out


def level_dims(W, H, sf, nl):
    """Level sizes as ComputePyramid computes them (src/ORBextractor.cc:1113-1114), in float32."""
    inv, dims = [], []
    s = np.float32(1.0)
    for l in range(nl):
        if l:
            s = np.float32(s * np.float32(sf))
        inv = np.float32(np.float32(1.0) / s)
        dims.append((int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))))
    return dims


def undefined_levels(W, H, sf, nl):
    """Levels on which the reference's ComputeKeyPointsOctTree / DistributeOctTree are undefined: no 30-px cell
    (:786-789 divide by nCols or nRows of 0 and convert the infinity to int) or a root count of 0 (:545, the first
    candidate indexes an empty vector)."""
    bad = []
    for l, (w, h) in enumerate(level_dims(W, H, sf, nl)):
        width, height = np.float32(w - 32), np.float32(h - 32)
        ncols, nrows = int(width / np.float32(30)), int(height / np.float32(30))
        if ncols < 1 or nrows < 1:
            bad.append(l)
            continue
        if np.float32(width / height) < np.float32(0.5):   # roundf(q) == 0
            bad.append(l)
    return bad
