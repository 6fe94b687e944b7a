"""bench.py's launch contract, without a GPU: --gpus N > 1 starts N ranks itself and fails loudly when they fail;
a launcher that started a different number of ranks than --gpus says is refused."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(kw)
    return e


def test_world_size_must_match_gpus():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=_env(WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 2 and "WORLD_SIZE=4" in p.stderr and p.stdout.strip() == ""


def test_gpus_flag_starts_the_ranks_and_relays_failure():
    """No GPU here, so both ranks stop with "bench.py needs a GPU": the parent must exit non-zero and print no result line
    (with GPUs the same path relays rank 0's JSON line; tests/test_bench_gpu.py)."""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("the failure relay is exercised on GPU-less hosts")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode != 0
    assert p.stdout.strip() == ""
    assert "2-rank run failed" in p.stderr and "needs a GPU" in p.stderr


def test_steps_must_be_positive():
    """--steps is the number of timed steps and ms_per_step divides by it: zero or fewer is refused before anything runs."""
    for bad in (["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]):
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + bad, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert p.returncode == 2 and bad[0] in p.stderr and p.stdout.strip() == ""


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _filled_blocks(shard, cap, ranges):
    """Flat result blocks as the timed path leaves them, with known contents: frame f has 3 + f keypoints whose fields encode
    (f, i), descriptors (f + i + b) & 255, matches i - 1."""
    import numpy as np
    import torch
    layout = shard.FlatLayout(max(hi - lo for lo, hi in ranges), cap)
    blocks = []
    for lo, hi in ranges:
        buf = layout.alloc()
        kv, dv, mv, cv, nv = layout.views(buf)
        for j in range(1, hi - lo + 1):
            f = lo + j - 1
            n = 3 + f
            rec = np.zeros(n, [("xyzar", "<f4", 5), ("octave", "<i4"), ("class_id", "<i4")])
            rec["xyzar"] = np.arange(5, dtype=np.float32) + 10 * f + 0.5
            rec["octave"] = np.arange(n) % 8
            rec["class_id"] = -1
            kv[j, :n] = torch.from_numpy(rec.view(np.float32).reshape(n, 7).copy())
            dv[j, :n] = torch.from_numpy(((f + np.arange(n)[:, None] + np.arange(32)[None, :]) & 255).astype(np.uint8))
            mv[j, :n] = torch.arange(n, dtype=torch.int32) - 1
            cv[j] = n
            nv[j] = n - 1
        blocks.append(buf)
    return layout, blocks


def test_dump_outputs_writes_the_stream_in_order(tmp_path):
    """bench.py --dump-outputs without a GPU: the flat blocks of two ranks come out as one stream, frame by frame, every array
    float32 / float64, integer fields by value."""
    import numpy as np
    import my_slam_amd.shard as shard
    bench = _bench_module()
    ranges = [shard.shard_range(7, 2, r) for r in range(2)]
    layout, blocks = _filled_blocks(shard, 16, ranges)
    info = bench.dump_outputs(str(tmp_path / "out"), layout, blocks, ranges)
    assert info["frames"] == info["of_frames"] == 7
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(got) == {"keypoints", "descriptors", "matches", "frame_index", "keypoint_counts", "match_counts"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) == info["bytes"] <= bench.DUMP_LIMIT_BYTES
    assert got["frame_index"].tolist() == list(range(7))
    assert got["keypoint_counts"].tolist() == [3 + f for f in range(7)] and got["match_counts"].tolist() == [2 + f for f in range(7)]
    off = 0
    for f in range(7):
        n = 3 + f
        k = got["keypoints"][off:off + n]
        assert np.array_equal(k[:, :5], np.broadcast_to(np.arange(5, dtype=np.float32) + 10 * f + 0.5, (n, 5)))
        assert k[:, 5].tolist() == [float(i % 8) for i in range(n)] and (k[:, 6] == -1).all()
        assert np.array_equal(got["descriptors"][off:off + n], (f + np.arange(n)[:, None] + np.arange(32)[None, :]) & 255)
        assert got["matches"][off:off + n].tolist() == [float(i - 1) for i in range(n)]
        off += n
    assert off == len(got["keypoints"]) == len(got["descriptors"]) == len(got["matches"])


def test_dump_outputs_samples_a_fixed_set_of_frames_when_too_large(tmp_path):
    """Over the size limit a seeded sample of whole frames is written; it depends on the stream length and capacity only."""
    import numpy as np
    import my_slam_amd.shard as shard
    bench = _bench_module()
    ranges = [(0, 40)]
    layout, blocks = _filled_blocks(shard, 64, ranges)
    limit = 10 * (64 * 40 * 4 + 24)
    a = bench.dump_outputs(str(tmp_path / "a"), layout, blocks, ranges, limit=limit)
    assert a["frames"] == 10 and a["of_frames"] == 40 and a["bytes"] <= limit
    layout2, blocks2 = _filled_blocks(shard, 64, ranges)
    kv = layout2.views(blocks2[0])[3]
    kv[1:] = 1                                             # other results, same shape of stream
    bench.dump_outputs(str(tmp_path / "b"), layout2, blocks2, ranges, limit=limit)
    fa, fb = np.load(tmp_path / "a" / "frame_index.npy"), np.load(tmp_path / "b" / "frame_index.npy")
    assert np.array_equal(fa, fb) and len(np.unique(fa)) == 10 and (np.diff(fa) > 0).all()
    assert np.load(tmp_path / "a" / "keypoint_counts.npy").tolist() == [3 + f for f in fa.astype(int)]
