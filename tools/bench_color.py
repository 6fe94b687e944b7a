#!/usr/bin/env python3
"""What the colour input formats (orbx_set_input_format, my-slam_amd/csrc/orbx_color.hip) cost, and whether the grey path noticed.

Medians of --reps calls after --warmup, host clock around calls that end in a synchronisation.  Frames: a synth.py stream of
--batch frames of 640 x 480 as one channel, a rolled and an inverted copy as the other two, constant alpha.

  grey_path      `python bench.py --gpus 1` (extras off) and the single-frame host call orbx_extract in grey, on this tree and, with
                 --parent-root DIR (a built checkout of the parent commit), on the parent: the parent three times (its own
                 run-to-run spread), this tree three times, alternating.
  device_batch   orbx_extract_batch_device + stream synchronise on --batch frames resident in HBM: grey, BGR, BGRA.
  host_batch     orbx_extract_batch from pageable host memory: grey, BGR, BGRA (the upload grows 3x / 4x).
  host_loop      tools/color_host_loop.cc: a g++ -O2 single-thread loop of the same formula over the same frames, checked against
                 the library's level 0.  It is not OpenCV's SIMD cvtColor, which this tool cannot time.
  kernel         with --kernel-stats CSV (the stats file of a `rocprofv3 --kernel-trace --stats` run of this tool with
                 --only-device FMT, a run of its own): the conversion kernel's mean duration against (bytes read + written) /
                 --hbm-tbps (the achievable HBM bandwidth; default 6.3 TB/s, the float4-copy figure measured on an MI355X).

usage: tools/bench_color.py [--batch 64] [--reps 30] [--warmup 5] [--parent-root DIR] [--kernel-stats bgr=CSV,bgra=CSV]
                            [--only-device bgr|bgra] [--grey-single] [--out profiles/color_bench.json]
"""
import argparse
import csv
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NF = 640, 480, 1000
FMT = {"grey": 0, "bgr": 1, "bgra": 3}
CN = {"grey": 1, "bgr": 3, "bgra": 4}


def _pkg(root=ROOT):
    spec = importlib.util.spec_from_file_location("my_slam_amd", os.path.join(root, "my-slam_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(root, "my-slam_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["my_slam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn, reps, warmup):
    t = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t))


def frames_of(pkg, batch, name):
    import my_slam_amd.synth as synth
    g = synth.stream(11, W, H, batch)
    if name == "grey":
        return g
    planes = [g, np.roll(g, 37, axis=2), 255 - g] + ([np.full_like(g, 255)] if name == "bgra" else [])
    return np.ascontiguousarray(np.stack(planes, -1))


def grey_single(pkg, reps, warmup):
    """the single-frame host call, grey (this works on the parent commit's package too)"""
    import my_slam_amd.synth as synth
    img = synth.stream(11, W, H, 1)[0]
    ex = pkg.ORBextractor(NF, max_width=W, max_height=H)
    kps = np.zeros(ex.cap, pkg.KP_DTYPE); desc = np.zeros((ex.cap, 32), np.uint8); n = C.c_int()
    return timed(lambda: pkg._chk(ex.L.orbx_extract(ex.h, img.ctypes.data, W, H, W, kps.ctypes.data, desc.ctypes.data, ex.cap, C.byref(n))), reps * 10, warmup * 10)


def bench_py(root, steps=200, warmup=20):
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                          "--no-pipelined", "--no-host-api", "--no-extra-configs"], capture_output=True, text=True, check=True, cwd=root).stdout
    return json.loads(out.strip().splitlines()[-1])["ms_per_step"]


def grey_single_of(root, reps, warmup):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--grey-single", "--root", root, "--reps", str(reps), "--warmup", str(warmup)],
                         capture_output=True, text=True, check=True).stdout
    return float(out.strip().splitlines()[-1])


def device_batch(pkg, name, batch, reps, warmup):
    import torch
    fr = frames_of(pkg, batch, name)
    ex = pkg.ORBextractor(NF, max_width=W, max_height=H, max_batch=batch)
    ex.set_input_format(FMT[name])
    d = torch.from_numpy(fr).cuda()
    cap = ex.cap
    k = torch.zeros((batch, cap, 7), device="cuda"); de = torch.zeros((batch, cap, 32), dtype=torch.uint8, device="cuda")
    c = torch.zeros(batch, dtype=torch.int32, device="cuda"); s = torch.zeros(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call():
        ex.extract_batch_device(d.data_ptr(), batch, W, H, W * CN[name], W * H * CN[name], k.data_ptr(), de.data_ptr(), c.data_ptr(), s.data_ptr(), st.cuda_stream)
        st.synchronize()
    ms = timed(call, reps, warmup)
    lvl0 = np.zeros((H, W), np.uint8)
    pkg._chk(ex.L.orbx_download_level(ex.h, batch - 1, 0, lvl0.ctypes.data, W, 0))
    return ms, int(c.sum()), fr, lvl0


def host_batch(pkg, name, batch, reps, warmup):
    fr = frames_of(pkg, batch, name)
    ex = pkg.ORBextractor(NF, max_width=W, max_height=H, max_batch=batch)
    ex.set_input_format(FMT[name])
    return timed(lambda: ex.extract_batch_raw(fr), reps, warmup)


def host_loop(fr, name, lvl0, reps, warmup):
    so = os.path.join(tempfile.mkdtemp(prefix="color_loop_"), "color_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "color_host_loop.cc"), "-o", so])
    L = C.CDLL(so)
    L.color_host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    L.color_host_loop.restype = None
    dst = np.zeros(fr.shape[:3], np.uint8)
    ms = timed(lambda: L.color_host_loop(fr.ctypes.data, dst.ctypes.data, dst.size, CN[name], 0), reps, warmup)
    if not np.array_equal(dst[-1], lvl0):
        raise SystemExit("host loop differs from the library's level 0 (%s)" % name)
    return ms


def kernel_stats(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_color_to_grey" in row["Name"]:
                return int(row["Calls"]), float(row["TotalDurationNs"]) / int(row["Calls"]) / 1e3
    raise SystemExit("%s: no k_color_to_grey row" % path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--only-device", default=None)
    ap.add_argument("--grey-single", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.grey_single:
        print(grey_single(_pkg(a.root), a.reps, a.warmup))
        return
    pkg = _pkg()
    if a.only_device:
        ms, nk, _, _ = device_batch(pkg, a.only_device, a.batch, a.reps, a.warmup)
        print(json.dumps({"format": a.only_device, "device_batch_ms": ms, "keypoints": nk}))
        return
    out = dict(tool="tools/bench_color.py", shape="%d x %dx%d, nfeatures %d" % (a.batch, W, H, NF), reps=a.reps, warmup=a.warmup)

    gp = dict(this_bench_ms_per_step=[], this_single_frame_ms=[])
    if a.parent_root:
        gp.update(parent_bench_ms_per_step=[], parent_single_frame_ms=[])
    for rnd in range(3):
        print("grey path, round %d" % rnd, file=sys.stderr, flush=True)
        if a.parent_root:
            gp["parent_bench_ms_per_step"].append(bench_py(a.parent_root))
            gp["parent_single_frame_ms"].append(grey_single_of(a.parent_root, a.reps, a.warmup))
        gp["this_bench_ms_per_step"].append(bench_py(ROOT))
        gp["this_single_frame_ms"].append(grey_single_of(ROOT, a.reps, a.warmup))
    if a.parent_root:
        for key in ("bench_ms_per_step", "single_frame_ms"):
            p, t = gp["parent_" + key], gp["this_" + key]
            gp[key + "_parent_spread"] = max(p) - min(p)
            gp[key + "_median_difference"] = float(np.median(t) - np.median(p))
    out["grey_path"] = gp

    dev, hst, loop = {}, {}, {}
    for name in ("grey", "bgr", "bgra"):
        print("batches, %s" % name, file=sys.stderr, flush=True)
        ms, nk, fr, lvl0 = device_batch(pkg, name, a.batch, a.reps, a.warmup)
        dev[name] = dict(ms=ms, keypoints=nk)
        hst[name] = dict(ms=host_batch(pkg, name, a.batch, a.reps, a.warmup), upload_bytes=int(fr.nbytes))
        if name != "grey":
            ms = host_loop(fr, name, lvl0, max(5, a.reps // 3), 2)
            loop[name] = dict(ms=ms, ms_per_frame=ms / a.batch)
    for name in ("bgr", "bgra"):
        dev[name]["over_grey_ms"] = dev[name]["ms"] - dev["grey"]["ms"]
        hst[name]["over_grey_ms"] = hst[name]["ms"] - hst["grey"]["ms"]
        hst[name]["times_grey"] = hst[name]["ms"] / hst["grey"]["ms"]
    out["device_batch"] = dev; out["host_batch"] = hst; out["host_loop"] = loop
    out["host_loop_note"] = "g++ -O2 single-thread loop of the same formula (tools/color_host_loop.cc); NOT OpenCV's SIMD cvtColor, which was not timed"

    if a.kernel_stats:
        ker = {}
        for item in a.kernel_stats.split(","):
            name, path = item.split("=")
            calls, us = kernel_stats(path)
            nbytes = a.batch * W * H * (CN[name] + 1)
            floor_us = nbytes / (a.hbm_tbps * 1e12) * 1e6
            ker[name] = dict(calls=calls, kernel_us=us, bytes=nbytes, floor_us_at_hbm=floor_us, hbm_tbps=a.hbm_tbps, fraction_of_hbm=floor_us / us,
                             achieved_tbps=nbytes / (us * 1e-6) / 1e12, source=os.path.basename(path))
        out["kernel"] = ker
        out["kernel_note"] = ("bound: bytes over bandwidth (3 or 4 bytes read + 1 written per pixel); the 64-frame colour input (59 / 79 MB) fits the "
                              "256 MiB Infinity Cache, so repeated calls on the same resident frames can read faster than HBM")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
