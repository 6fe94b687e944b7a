/*
 * ref_pnp.cc -- driver that runs the reference's own src/PnPsolver.cc (compiled unmodified and in place, behind the stand-in
 * Frame / MapPoint of solver_standin.h, on the C API of the OpenCV shim's cv_linalg.hpp) for
 * tests/test_reference_pin_solvers_*.py.
 *
 *   ref_pnp REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable.  The file format and the scripted rand() are in ref_solver_io.h.
 * PnPsolver's state is private; this translation unit alone reads include/PnPsolver.h with `private` defined as `public`
 * (after the standard headers), the reference's .cc is compiled as it is.
 *
 * Request:
 *   p2d     float32 [N, 2]   mvKeysUn[i].pt of the matched keypoints
 *   sig2    float32 [N]      mvLevelSigma2[octave] of each (keypoint i has octave i, the table has N entries)
 *   p3d     float32 [N, 3]   GetWorldPos() of the matched points
 *   K       float32 [4]      fx, fy, cx, cy
 *   prob    float64 [1]
 *   fpar    float32 [2]      epsilon, th2
 *   ipar    int32   [7]      seed of the scripted source, minInliers, maxIterations, minSet, mode, step, max_calls
 *
 * Response: after SetRansacParameters(prob, minInliers, maxIterations, minSet, epsilon, th2)
 *   maxits, mininl, minset  int32     mRansacMaxIts, mRansacMinInliers, mRansacMinSet
 *   eps                     float32   mRansacEpsilon
 *   maxerr                  float32 [N]   mvMaxError
 * then one group per iterate(step, ...) call, until bNoMore in mode 2 and for max_calls calls in mode 1:
 *   got, nomore, rn  int32           a pose came back; bNoMore; nInliers
 *   rinl             uint8 [N]       vbInliers (zeros when the reference left it empty)
 *   T                float32 [4, 4]  the returned pose (zeros without one)
 *   iters, best      int32           mnIterations, mnBestInliers
 * Mode 1 (one hypothesis per call) adds to each group
 *   sample           int32 [minSet]  the indices drawn
 *   R, t             float64         mRi, mti of the hypothesis
 *   ninl, inl        int32, uint8[N] mnInliersi, mvbInliersi
 *   direct           int32           see below
 *
 * Mode 1.  The loop of iterate is `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` (src/PnPsolver.cc:182):
 * with mRansacMaxIts set to 1, every iterate(1) call runs exactly one iteration.  The driver sets that, and mRansacMinInliers to
 * N, after recording the state, so that Refine (:226), which overwrites mRi, mti and mvbInliersi, runs only for a hypothesis with
 * all N inliers.  When it did run (mnRefinedInliers changed), the driver evaluates the sample again through the reference's own
 * reset_correspondences / add_correspondence / compute_pose / CheckInliers, in the order of :186-207, and marks the group
 * direct = 1.  The sample is the replay of the RandomInt calls of :191-201 on a copy of the source's state, proved against pws,
 * the reference's own copy of the sample's points (exit status 3 on a mismatch).
 *
 * Mode 2 is the transcript of iterate(step) with nothing changed, Refine included.
 *
 * Refused (status 2): N == 0, N < minSet, or N below the minimum inlier count that SetRansacParameters arrives at, where :150
 * converts a NaN to int.  The CONSTRUCTOR makes the same conversion with its defaults (minInliers 8) whenever N < 8; what it
 * computes is overwritten by the driver's own call, so those requests are answered, and the UBSan copy reports that one line.
 */
#include "ref_solver_io.h"

#define private public
#include "PnPsolver.h"           // the reference's; MapPoint.h and Frame.h in it are skipped by solver_standin.h
#undef private
#include "Thirdparty/DBoW2/DUtils/Random.h"

using namespace ORB_SLAM2;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy;

int main(int argc, char **argv)
{
    refio::g_name = "ref_pnp";
    if (argc != 3) refio::refuse("usage: ref_pnp REQUEST RESPONSE");
    refio::Request req(argv[1]);
    const refio::Record &r2 = req.get("p2d", refio::F32, -1, 2);
    const int n = r2.rows;
    const float *p2d = r2.as<float>(refio::F32), *p3d = req.get("p3d", refio::F32, n, 3).as<float>(refio::F32);
    const float *sig2 = req.get("sig2", refio::F32, 1, n).as<float>(refio::F32), *k = req.get("K", refio::F32, 1, 4).as<float>(refio::F32);
    const double prob = req.get("prob", refio::F64, 1, 1).as<double>(refio::F64)[0];
    const float *fp = req.get("fpar", refio::F32, 1, 2).as<float>(refio::F32);
    const int32_t *ip = req.get("ipar", refio::I32, 1, 7).as<int32_t>(refio::I32);
    const float epsilon = fp[0], th2 = fp[1];
    const int seed = ip[0], min_inliers = ip[1], max_its = ip[2], min_set = ip[3], mode = ip[4], step = ip[5], max_calls = ip[6];
    if (mode != 1 && mode != 2) refio::refuse("mode is 1 (hypotheses) or 2 (transcript)");
    if (min_inliers < 1 || max_its < 1 || min_set < 4 || step < 1 || max_calls < 1 || (mode == 1 && step != 1)) refio::refuse("bad parameters");
    int n_min = n * epsilon;                             /* :134-138 */
    if (n_min < min_inliers) n_min = min_inliers;
    if (n_min < min_set) n_min = min_set;
    if (n == 0 || n < min_set || n < n_min) refio::refuse("N is below what SetRansacParameters and the draw are defined for (src/PnPsolver.cc:141-150, :193)");

    Frame F;
    Frame::fx = k[0];
    Frame::fy = k[1];
    Frame::cx = k[2];
    Frame::cy = k[3];
    F.mvKeysUn.resize(n);
    F.mvLevelSigma2.assign(sig2, sig2 + n);
    std::vector<MapPoint> store;
    store.reserve(n);
    for (int i = 0; i < n; i++) {
        F.mvKeysUn[i].pt = cv::Point2f(p2d[2 * i], p2d[2 * i + 1]);
        F.mvKeysUn[i].octave = i;
        cv::Mat pos(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) pos.at<float>(c) = p3d[3 * i + c];
        store.push_back(MapPoint(pos));
        F.mvpMapPoints.push_back(&store.back());
    }

    refio::lcg_seed(seed);
    PnPsolver s(F, F.mvpMapPoints);
    if (s.mvP2D.size() != (size_t)n) refio::refuse("the solver dropped a correspondence");
    s.SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2);

    refio::Response out(argv[2]);
    out.i32("maxits", s.mRansacMaxIts);
    out.i32("mininl", s.mRansacMinInliers);
    out.i32("minset", s.mRansacMinSet);
    out.f32("eps", s.mRansacEpsilon);
    out.put("maxerr", refio::F32, 1, n, s.mvMaxError.data());
    if (mode == 1) {
        s.mRansacMaxIts = 1;
        s.mRansacMinInliers = n;
    }

    for (int call = 0; call < max_calls; call++) {
        std::vector<int32_t> sample(min_set, 0);
        if (mode == 1) {                                 /* the replay of :188-201, on a copy of the source */
            const uint32_t state = refio::g_lcg;
            const int calls = refio::g_rand_calls;
            std::vector<size_t> avail = s.mvAllIndices;
            for (int i = 0; i < min_set; i++) {
                int randi = DUtils::Random::RandomInt(0, (int)avail.size() - 1);
                sample[i] = (int32_t)avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
            refio::g_lcg = state;
            refio::g_rand_calls = calls;
            s.mnRefinedInliers = -1;
        }
        const int before = s.mnIterations;
        bool no_more = false;
        std::vector<bool> inl;
        int n_inl = 0;
        cv::Mat T = s.iterate(step, no_more, inl, n_inl);
        out.i32("got", T.empty() ? 0 : 1);
        out.i32("nomore", no_more ? 1 : 0);
        out.i32("rn", n_inl);
        if (!inl.empty() && (int)inl.size() != n) refio::refuse("vbInliers has an unexpected size");
        out.flags("rinl", inl.empty() ? std::vector<bool>(n, false) : inl);
        std::vector<float> tv(16, 0.0f);
        if (!T.empty())
            for (int i = 0; i < 16; i++) tv[i] = T.at<float>(i);
        out.put("T", refio::F32, 4, 4, tv.data());
        out.i32("iters", s.mnIterations);
        out.i32("best", s.mnBestInliers);
        if (mode == 1) {
            if (s.mnIterations != before + 1) refio::refuse("an iterate(1) call did not run one iteration");
            int direct = 0;
            if (s.mnRefinedInliers != -1) {              /* Refine overwrote the hypothesis: evaluate the sample again, :186-207 */
                direct = 1;
                s.set_maximum_number_of_correspondences(min_set);
                s.reset_correspondences();
                for (int i = 0; i < min_set; i++) {
                    int idx = sample[i];
                    s.add_correspondence(s.mvP3Dw[idx].x, s.mvP3Dw[idx].y, s.mvP3Dw[idx].z, s.mvP2D[idx].x, s.mvP2D[idx].y);
                }
                s.compute_pose(s.mRi, s.mti);
                s.CheckInliers();
            }
            for (int i = 0; i < min_set; i++)            /* pws is the reference's own copy of the sample */
                for (int c = 0; c < 3; c++)
                    if (s.pws[3 * i + c] != (double)p3d[3 * sample[i] + c]) {
                        std::fprintf(stderr, "ref_pnp: the replayed sample is not the one the reference drew\n");
                        return 3;
                    }
            out.put("sample", refio::I32, 1, min_set, sample.data());
            out.put("R", refio::F64, 3, 3, &s.mRi[0][0]);
            out.put("t", refio::F64, 1, 3, s.mti);
            out.i32("ninl", s.mnInliersi);
            out.flags("inl", s.mvbInliersi);
            out.i32("direct", direct);
        } else if (no_more) {
            break;
        }
    }
    out.close();
    return 0;
}
