// orbp_pose.cc -- Optimizer::PoseOptimization (src/Optimizer.cc:239-451 of WChen09/My-SLAM, on g2o) over flat arrays:
// orbp_pose_optimization (include/orbp.h).  The arithmetic of an edge, the 6x6 solve, the Levenberg loop and the four rounds are
// csrc/orbp_pose_body.h, the text the kernel of orbm_pose.hip runs as well; this file owns the order of the sums (edge order, as
// g2o's active edges are sorted by id) and keeps an edge's error between two passes at one estimate.
#include <cstring>
#include <vector>
#include "../../include/orbp.h"
#include "../../include/orbx.h"
#include "orbp_internal.h"
#include "orbp_pose_body.h"

namespace {
// The edges keep the point in the camera frame and the error of the last pass, as g2o's do, so that the system pass right after an
// accepted trial (same estimate) does not map every point again; what is kept is what pose_edge_error would give anew.
struct PoseHost {
    PoseCam cam;
    PoseEdges E;
    int n;
    Se3 at;                     // the estimate the kept errors of the active edges are at
    bool kept = false;
    std::vector<PoseEdge> edge;

    template <bool SYSTEM>
    void pass(const Se3 &T, bool robust, double *acc)
    {
        const bool reuse = kept && memcmp(&T, &at, sizeof T) == 0;
        for (int i = 0; i < n; i++)
            if (!E.outlier[i]) {
                if (!reuse) pose_edge_error(edge[i], T, cam);
                pose_edge_sums<SYSTEM>(edge[i], cam, robust, acc);
            }
        at = T; kept = true;
    }
    void system(const Se3 &T, bool robust, double *sys)
    {
        for (int v = 0; v < POSE_NSYS; v++) sys[v] = 0;
        pass<true>(T, robust, sys);
    }
    double chi2(const Se3 &T, bool robust)
    {
        double sum[1] = {0};
        pass<false>(T, robust, sum);
        return sum[0];
    }
    int flag(const Se3 &est, const Se3 &err_est)
    {
        const bool reuse = kept && memcmp(&err_est, &at, sizeof at) == 0;
        int n_bad = 0;
        for (int i = 0; i < n; i++) {
            if (E.outlier[i]) pose_edge_error(edge[i], est, cam);
            else if (!reuse) pose_edge_error(edge[i], err_est, cam);
            n_bad += E.outlier[i] = pose_edge_is_outlier(edge[i]);
        }
        kept = false;           // the active set changes
        return n_bad;
    }
};
}   // namespace

extern "C" int orbp_pose_optimization(int n, const float *obs, const float *u_right, const float *inv_sigma2, const float *xw,
                                      float fx, float fy, float cx, float cy, float bf, float *Tcw, uint8_t *outlier)
{
    if (n < 0 || !Tcw || !outlier || (n > 0 && (!obs || !inv_sigma2 || !xw))) {
        orbp_set_error("bad arguments");
        return ORBX_E_INVALID;
    }
    for (int i = 0; i < n; i++) outlier[i] = 0;
    if (n < 3) return 0;                        // :363-364: the pose stays as it came
    PoseHost P;
    P.cam = {fx, fy, cx, cy, bf};
    P.E = {obs, u_right, inv_sigma2, xw, outlier};
    P.n = n;
    P.edge.resize(n);
    for (int i = 0; i < n; i++) pose_edge_load(P.edge[i], P.E, i);
    Se3 est;
    const int n_bad = pose_rounds(P, n, se3_from_Tcw(Tcw), est);
    se3_to_Tcw(est, Tcw);
    return n - n_bad;
}
