"""Restatement of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307 of WChen09/My-SLAM) in numpy, shaped like
the reference (the full matrix, a sort per row, index int(0.5 * (N - 1)), the first strict minimum), not like the kernels that
are tested against it.  Line numbers are those of src/MapPoint.cc."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1647-1663): the number of differing bits of two 32-byte rows."""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def distinctive_descriptor(D):
    """One MapPoint.  D: the rows vDescriptors holds after :261-267 (map order, bad key frames left out), N x 32 uint8.
    Returns (BestIdx, BestMedian); (-1, -1) where the reference returns early with mDescriptor untouched (:256, :269)."""
    D = np.asarray(D, np.uint8).reshape(-1, 32)
    N = len(D)                                                  # :273
    if N == 0:                                                  # :256-257, :269-270
        return -1, -1
    Distances = np.zeros((N, N), np.float32)                    # :275 float Distances[N][N]
    for i in range(N):                                          # :276
        Distances[i, i] = 0                                     # :278
        if i + 1 < N:                                           # :279-284, all j > i at once
            dij = _POP[np.bitwise_xor(D[i + 1:], D[i])].sum(axis=1)
            Distances[i, i + 1:] = dij                          # :282
            Distances[i + 1:, i] = dij                          # :283
    BestMedian = np.iinfo(np.int32).max                         # :288 INT_MAX
    BestIdx = 0                                                 # :289
    for i in range(N):                                          # :290
        vDists = Distances[i].astype(np.int32)                  # :292 vector<int> from the float row (exact: <= 256)
        vDists = np.sort(vDists)                                # :293
        median = int(vDists[int(0.5 * (N - 1))])                # :294
        if median < BestMedian:                                 # :296
            BestMedian = median                                 # :298
            BestIdx = i                                         # :299
    return BestIdx, BestMedian


def distinctive_descriptors(off, desc):
    """A batch as the library takes it: point p owns rows off[p]:off[p+1] of desc.  Returns (best, best_median), int32."""
    off = np.asarray(off, np.int64)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    n = len(off) - 1
    best, med = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for p in range(n):
        best[p], med[p] = distinctive_descriptor(desc[off[p]:off[p + 1]])
    return best, med


# ---- batches the tests, the stress tool and the benchmark share

def run_lengths_keyframe(rng, n_points, tail=(17, 400), tail_share=0.03):
    """Observations per MapPoint of a key frame: mostly 2..15, a tail up to a few hundred."""
    n = rng.integers(2, 16, n_points)
    t = rng.random(n_points) < tail_share
    lo, hi = tail
    n[t] = np.exp(rng.uniform(np.log(lo), np.log(hi), int(t.sum()))).astype(np.int64)
    return n.astype(np.int64)


def batch_from_lengths(rng, lengths, flips=6):
    """CSR batch: a run's rows are one random base descriptor with up to `flips` random bit flips per observation (small
    distances, many ties).  flips=None: uniformly random rows (distances crowd round 128)."""
    lengths = np.asarray(lengths, np.int64)
    off = np.zeros(len(lengths) + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    if flips is None:
        return off, rng.integers(0, 256, (total, 32), dtype=np.uint8)
    base = rng.integers(0, 256, (len(lengths), 32), dtype=np.uint8)
    desc = np.repeat(base, lengths, axis=0)
    for _ in range(flips):
        hit = rng.random(total) < 0.7
        byte = rng.integers(0, 32, total)
        bit = (1 << rng.integers(0, 8, total)).astype(np.uint8)
        rows = np.nonzero(hit)[0]
        desc[rows, byte[rows]] ^= bit[rows]
    return off, desc
