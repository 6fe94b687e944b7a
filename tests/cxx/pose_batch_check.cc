// pose_batch_check.cc -- the C++ adapter Optimizer::PoseOptimizationBatch (my-slam_amd/host/PnPsolver.h) against
// Optimizer::PoseOptimization on the same problems: the host path once per problem, the batch in one GPU launch, then every pose
// entry (|d| <= 2e-6: the output is fp32), every mvbOutlier flag and every return value compared.
// Driven by tests/test_pose_batch_cxx.py:  pose_batch_check compile-only  |  pose_batch_check <case file>
// Case file: int32 B, then per problem int32 n, int32 has_uRight, float fx fy cx cy bf, float Tcw[16], obs[2n], invSigma2[n],
// Xw[3n], uRight[n] when has_uRight.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "PnPsolver.h"

using ORB_SLAM2::Optimizer;

template <class T> static bool rd(FILE *f, T *dst, size_t count) { return count == 0 || fread(dst, sizeof(T), count, f) == count; }

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "compile-only")) {
        // the call shape without a device: a NULL matcher is refused, and the problems stay as they were
        std::vector<Optimizer::PoseProblem> none(1);
        none[0].nGood = -5;
        std::string err;
        const int rc = Optimizer::PoseOptimizationBatch(nullptr, none, &err);
        printf("NULL matcher: status %d (%s)\n", rc, err.c_str());
        return (rc != ORBX_OK && none[0].nGood == -5 && !err.empty()) ? 0 : 1;
    }
    if (argc != 2) { fprintf(stderr, "usage: %s compile-only | <case file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t B = 0;
    if (!rd(f, &B, 1) || B < 0) return 2;
    std::vector<Optimizer::PoseProblem> problems(B);
    for (auto &P : problems) {
        int32_t head[2];
        float cam[5];
        if (!rd(f, head, 2) || !rd(f, cam, 5) || !rd(f, P.Tcw.data(), 16)) return 2;
        const size_t n = (size_t)head[0];
        P.fx = cam[0]; P.fy = cam[1]; P.cx = cam[2]; P.cy = cam[3]; P.bf = cam[4];
        P.obs.resize(2 * n); P.invSigma2.resize(n); P.Xw.resize(3 * n);
        if (head[1]) P.uRight.resize(n);
        if (!rd(f, P.obs.data(), 2 * n) || !rd(f, P.invSigma2.data(), n) || !rd(f, P.Xw.data(), 3 * n) || !rd(f, P.uRight.data(), P.uRight.size())) return 2;
    }
    fclose(f);

    // the host path, problem by problem
    std::vector<ORB_SLAM2::Pose> hostT(B);
    std::vector<std::vector<bool>> hostOut(B);
    std::vector<int> hostGood(B);
    for (int p = 0; p < B; p++) {
        const auto &P = problems[p];
        hostT[p] = P.Tcw;
        hostGood[p] = Optimizer::PoseOptimization(P.obs, P.uRight, P.invSigma2, P.Xw, P.fx, P.fy, P.cx, P.cy, P.bf, hostT[p], hostOut[p]);
    }

    orbm_matcher *m = nullptr;
    if (orbm_create(&m, 0, 1024, 1024, 1 << 16) != ORBX_OK) { fprintf(stderr, "orbm_create: %s\n", orbm_last_error()); return 3; }
    std::string err;
    const int rc = Optimizer::PoseOptimizationBatch(m, problems, &err);
    orbm_destroy(m);
    if (rc != ORBX_OK) { fprintf(stderr, "PoseOptimizationBatch: status %d: %s\n", rc, err.c_str()); return 3; }

    int differences = 0;
    for (int p = 0; p < B; p++) {
        const auto &P = problems[p];
        double d = 0;
        for (int k = 0; k < 16; k++) d = std::fmax(d, std::fabs((double)P.Tcw[k] - (double)hostT[p][k]));
        int flips = P.outlier.size() != hostOut[p].size();
        for (size_t i = 0; i < P.outlier.size() && i < hostOut[p].size(); i++) flips += P.outlier[i] != hostOut[p][i];
        const bool bad = !(d <= 2e-6) || flips || P.nGood != hostGood[p];
        if (bad) printf("problem %d (n=%zu): |dTcw| %.3g, %d flags differ, nGood %d / %d\n", p, P.invSigma2.size(), d, flips, P.nGood, hostGood[p]);
        differences += bad;
    }
    printf("%d problems, %d differences\n", B, differences);
    return differences ? 1 : 0;
}
