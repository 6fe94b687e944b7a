/*
 * ref_sim3.cc -- driver that runs the reference's own src/Sim3Solver.cc (compiled unmodified and in place, behind the stand-in
 * KeyFrame / MapPoint of solver_standin.h, on the OpenCV shim's cv_linalg.hpp) for tests/test_reference_pin_solvers_*.py.
 *
 *   ref_sim3 REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable: it keeps the reference's code out of the test process.  The file format and
 * the scripted rand() are in ref_solver_io.h.
 *
 * Request:
 *   x1, x2       float32 [N, 3]   the matched points in camera 1 / camera 2 (mvX3Dc1 / mvX3Dc2)
 *   sig1, sig2   float32 [N]      mvLevelSigma2[octave] of the two keypoints of each match
 *   K1, K2       float32 [4]      fx, fy, cx, cy
 *   prob         float64 [1]
 *   ipar         int32   [6]      bFixScale, seed of the scripted source, minInliers, maxIterations, step, max_calls
 * The driver builds two key frames with identity pose and one MapPoint pair per match whose world positions are x1 / x2, so
 * Rcw * Xw + tcw (src/Sim3Solver.cc:95-98) is 1 * x + 0 * y + 0 * z + 0, the given float.  Keypoint i has octave i and
 * mvLevelSigma2 has N entries, so every match gets its own sigma2.
 *
 * Response: after SetRansacParameters(prob, minInliers, maxIterations)
 *   maxits, mininl  int32           mRansacMaxIts, mRansacMinInliers
 *   err1, err2      float64 [N]     mvnMaxError1 / mvnMaxError2 (the integer-truncated thresholds, src/Sim3Solver.cc:87-88)
 * then one group per iterate(step, ...) call until bNoMore (at most max_calls):
 *   got, nomore, rn int32           a pose came back; bNoMore; nInliers
 *   rinl            uint8 [N]       vbInliers
 *   T               float32 [4, 4]  the returned pose (zeros without one)
 *   iters, best     int32           mnIterations, mnBestInliers after the call
 *   es, eR, et      float32         GetEstimatedScale / Rotation / Translation (zeros before the first iteration)
 * and, with step == 1, the state of the hypothesis the call evaluated (ran = 0 and zeros when the call evaluated none):
 *   ran             int32
 *   tri             int32 [3]       the triple drawn
 *   ninl, inl       int32, uint8[N] mnInliersi, mvbInliersi
 *   s, R, t         float32         ms12i, mR12i, mt12i
 *
 * The triple.  iterate() keeps its draw in locals.  The driver replays the three DUtils::Random::RandomInt calls of
 * src/Sim3Solver.cc:166-177 on a copy of the source's state before the call, and proves the replay: ComputeSim3 on the replayed
 * triple must give mR12i, mt12i and ms12i byte for byte (exit status 3 otherwise).
 *
 * Refused (status 2): N < minInliers or N == 0, where SetRansacParameters divides by N and converts a NaN to int (:125-133).
 * The CONSTRUCTOR makes the same conversion with its default minInliers = 6 whenever N < 6; what it computes is overwritten by
 * the driver's own SetRansacParameters call, so those requests are answered, and the UBSan copy reports that one line.
 */
#include "ref_solver_io.h"

#include "Sim3Solver.h"          // the reference's; KeyFrame.h in it is skipped by solver_standin.h
#include "Thirdparty/DBoW2/DUtils/Random.h"

using namespace ORB_SLAM2;

class Probe : public Sim3Solver {
public:
    Probe(KeyFrame *a, KeyFrame *b, const std::vector<MapPoint *> &m, bool fix) : Sim3Solver(a, b, m, fix) {}
    using Sim3Solver::ComputeSim3;
    using Sim3Solver::mvX3Dc1;
    using Sim3Solver::mvX3Dc2;
    using Sim3Solver::mvAllIndices;
    using Sim3Solver::mvnMaxError1;
    using Sim3Solver::mvnMaxError2;
    using Sim3Solver::mR12i;
    using Sim3Solver::mt12i;
    using Sim3Solver::ms12i;
    using Sim3Solver::mvbInliersi;
    using Sim3Solver::mnInliersi;
    using Sim3Solver::mnIterations;
    using Sim3Solver::mnBestInliers;
    using Sim3Solver::mRansacMaxIts;
    using Sim3Solver::mRansacMinInliers;
    using Sim3Solver::N;
};

static cv::Mat mat_k(const float *k)
{
    cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
    K.at<float>(0, 0) = k[0];
    K.at<float>(1, 1) = k[1];
    K.at<float>(0, 2) = k[2];
    K.at<float>(1, 2) = k[3];
    return K;
}

static void put_mat(refio::Response &out, const char *tag, const cv::Mat &m, int rows, int cols)
{
    std::vector<float> v((size_t)rows * cols, 0.0f);
    if (!m.empty()) {
        if (m.type() != CV_32F || (int)m.total() != rows * cols) refio::refuse("a matrix of an unexpected shape");
        for (int i = 0; i < rows * cols; i++) v[i] = m.at<float>(i);
    }
    out.put(tag, refio::F32, rows, cols, v.data());
}

int main(int argc, char **argv)
{
    refio::g_name = "ref_sim3";
    if (argc != 3) refio::refuse("usage: ref_sim3 REQUEST RESPONSE");
    refio::Request req(argv[1]);
    const refio::Record &rx1 = req.get("x1", refio::F32, -1, 3);
    const int n = rx1.rows;
    const float *x1 = rx1.as<float>(refio::F32), *x2 = req.get("x2", refio::F32, n, 3).as<float>(refio::F32);
    const float *sig1 = req.get("sig1", refio::F32, 1, n).as<float>(refio::F32), *sig2 = req.get("sig2", refio::F32, 1, n).as<float>(refio::F32);
    const float *k1 = req.get("K1", refio::F32, 1, 4).as<float>(refio::F32), *k2 = req.get("K2", refio::F32, 1, 4).as<float>(refio::F32);
    const double prob = req.get("prob", refio::F64, 1, 1).as<double>(refio::F64)[0];
    const int32_t *ip = req.get("ipar", refio::I32, 1, 6).as<int32_t>(refio::I32);
    const bool fix = ip[0] != 0;
    const int seed = ip[1], min_inliers = ip[2], max_its = ip[3], step = ip[4], max_calls = ip[5];
    if (n == 0 || n < min_inliers) refio::refuse("N < minInliers: SetRansacParameters is undefined there (src/Sim3Solver.cc:125-133)");
    if (min_inliers < 1 || max_its < 1 || step < 1 || max_calls < 1) refio::refuse("minInliers, maxIterations, step and max_calls must be positive");

    std::vector<cv::KeyPoint> keys(n);
    for (int i = 0; i < n; i++) keys[i].octave = i;
    cv::Mat I = cv::Mat::eye(3, 3, CV_32F), zero(3, 1, CV_32F, cv::Scalar(0));
    KeyFrame kf1(keys, std::vector<float>(sig1, sig1 + n), mat_k(k1), I, zero), kf2(keys, std::vector<float>(sig2, sig2 + n), mat_k(k2), I, zero);
    std::vector<MapPoint *> matched(n);
    std::vector<MapPoint> store;
    store.reserve(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        cv::Mat a(3, 1, CV_32F), b(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) {
            a.at<float>(k) = x1[3 * i + k];
            b.at<float>(k) = x2[3 * i + k];
        }
        store.push_back(MapPoint(a));
        store.back().index[&kf1] = i;
        kf1.mvpMapPoints.push_back(&store.back());
        store.push_back(MapPoint(b));
        store.back().index[&kf2] = i;
        matched[i] = &store.back();
    }

    refio::lcg_seed(seed);
    Probe s(&kf1, &kf2, matched, fix);
    if (s.N != n) refio::refuse("the solver dropped a correspondence");
    for (int i = 0; i < n; i++)                          /* the camera-frame points are the request's floats */
        for (int k = 0; k < 3; k++)
            if (std::memcmp(&s.mvX3Dc1[i].at<float>(k), &x1[3 * i + k], 4) || std::memcmp(&s.mvX3Dc2[i].at<float>(k), &x2[3 * i + k], 4)) return 3;
    s.SetRansacParameters(prob, min_inliers, max_its);

    refio::Response out(argv[2]);
    out.i32("maxits", s.mRansacMaxIts);
    out.i32("mininl", s.mRansacMinInliers);
    std::vector<double> e1(s.mvnMaxError1.begin(), s.mvnMaxError1.end()), e2(s.mvnMaxError2.begin(), s.mvnMaxError2.end());
    out.put("err1", refio::F64, 1, n, e1.data());
    out.put("err2", refio::F64, 1, n, e2.data());

    for (int call = 0; call < max_calls; call++) {
        int32_t tri[3] = {0, 0, 0};
        cv::Mat wantR, wantt;
        float wants = 0;
        if (step == 1) {                                 /* the replay of :163-177, on a copy of the source */
            const uint32_t state = refio::g_lcg;
            const int calls = refio::g_rand_calls;
            std::vector<size_t> avail = s.mvAllIndices;
            cv::Mat P1(3, 3, CV_32F), P2(3, 3, CV_32F);
            for (int i = 0; i < 3; i++) {
                int randi = DUtils::Random::RandomInt(0, (int)avail.size() - 1);
                tri[i] = (int32_t)avail[randi];
                s.mvX3Dc1[tri[i]].copyTo(P1.col(i));
                s.mvX3Dc2[tri[i]].copyTo(P2.col(i));
                avail[randi] = avail.back();
                avail.pop_back();
            }
            s.ComputeSim3(P1, P2);
            wantR = s.mR12i.clone();
            wantt = s.mt12i.clone();
            wants = s.ms12i;
            refio::g_lcg = state;
            refio::g_rand_calls = calls;
        }
        const int before = s.mnIterations;
        bool no_more = false;
        std::vector<bool> inl;
        int n_inl = 0;
        cv::Mat T = s.iterate(step, no_more, inl, n_inl);
        out.i32("got", T.empty() ? 0 : 1);
        out.i32("nomore", no_more ? 1 : 0);
        out.i32("rn", n_inl);
        if ((int)inl.size() != n) refio::refuse("vbInliers has an unexpected size");
        out.flags("rinl", inl);
        put_mat(out, "T", T, 4, 4);
        out.i32("iters", s.mnIterations);
        out.i32("best", s.mnBestInliers);
        out.f32("es", s.mnIterations > 0 ? s.GetEstimatedScale() : 0.0f);
        put_mat(out, "eR", s.GetEstimatedRotation(), 3, 3);
        put_mat(out, "et", s.GetEstimatedTranslation(), 3, 1);
        if (step == 1) {
            const bool ran = s.mnIterations == before + 1;
            if (ran) {
                bool same = std::memcmp(&wants, &s.ms12i, 4) == 0;
                for (int i = 0; i < 9; i++) same = same && std::memcmp(&wantR.at<float>(i), &s.mR12i.at<float>(i), 4) == 0;
                for (int i = 0; i < 3; i++) same = same && std::memcmp(&wantt.at<float>(i), &s.mt12i.at<float>(i), 4) == 0;
                if (!same) {
                    std::fprintf(stderr, "ref_sim3: the replayed triple does not reproduce the hypothesis\n");
                    return 3;
                }
            } else {
                tri[0] = tri[1] = tri[2] = 0;
            }
            out.i32("ran", ran ? 1 : 0);
            out.put("tri", refio::I32, 1, 3, tri);
            out.i32("ninl", ran ? s.mnInliersi : 0);
            out.flags("inl", ran ? s.mvbInliersi : std::vector<bool>(n, false));
            out.f32("s", ran ? s.ms12i : 0.0f);
            put_mat(out, "R", ran ? s.mR12i : cv::Mat(), 3, 3);
            put_mat(out, "t", ran ? s.mt12i : cv::Mat(), 3, 1);
        }
        if (no_more) break;
    }
    out.close();
    return 0;
}
