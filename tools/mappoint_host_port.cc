// mappoint_host_port.cc -- a single-thread host PORT of the algorithm of MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:242-307 of WChen09/My-SLAM) for tools/bench_mappoint.py: the baseline an integrator keeps when the
// descriptor choice stays on the CPU.  Written for this repository (it is not the reference's code and links none of it); it
// keeps the reference's shape -- an N x N float matrix, the upper triangle computed and mirrored, std::sort of every row, the
// first strict minimum -- with the matrix on the heap instead of the stack, and the bit count the compiler makes of
// __builtin_popcountll.  tools/bench_mappoint.py compiles it with g++ -O2 into a shared object and checks its answers.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

static inline int distance256(const uint8_t *a, const uint8_t *b)
{
    uint64_t x[4], y[4];
    memcpy(x, a, 32); memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
           __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" void mappoint_host_port(int n_points, const int32_t *off, const uint8_t *desc, int32_t *best, int32_t *best_median)
{
    std::vector<float> Distances;
    std::vector<int> vDists;
    for (int p = 0; p < n_points; p++) {
        const size_t N = (size_t)(off[p + 1] - off[p]);
        const uint8_t *D = desc + (size_t)off[p] * 32;
        if (N == 0) { best[p] = -1; best_median[p] = -1; continue; }
        Distances.resize(N * N);
        for (size_t i = 0; i < N; i++) {
            Distances[i * N + i] = 0;
            for (size_t j = i + 1; j < N; j++) {
                const int distij = distance256(D + 32 * i, D + 32 * j);
                Distances[i * N + j] = (float)distij;
                Distances[j * N + i] = (float)distij;
            }
        }
        int BestMedian = INT_MAX, BestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            vDists.assign(Distances.begin() + i * N, Distances.begin() + (i + 1) * N);
            std::sort(vDists.begin(), vDists.end());
            const int median = vDists[(size_t)(0.5 * (N - 1))];
            if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
        }
        best[p] = BestIdx; best_median[p] = BestMedian;
    }
}
