/*
 * ref_init.cc -- driver that runs the reference's own src/Initializer.cc (compiled unmodified and in place, behind the stand-in
 * Frame of solver_standin.h, on the OpenCV shim's cv_linalg.hpp) for tests/test_reference_pin_solvers_*.py.
 *
 *   ref_init REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable.  The file format and the scripted rand() are in ref_solver_io.h.
 * Initializer's state and steps are private; this translation unit alone reads include/Initializer.h with `private` defined as
 * `public` (after the standard headers), the reference's .cc is compiled as it is.
 *
 * Request:
 *   keys1, keys2   float32 [n1, 2], [n2, 2]   mvKeysUn[i].pt of the reference and the current frame
 *   m12            int32   [n1]               vMatches12
 *   K              float32 [4]                fx, fy, cx, cy
 *   sigma          float32 [1]
 *   ipar           int32   [3]                seed of the scripted source, iterations, n_per_set (sets recorded one by one)
 *
 * Response, in this order (N = mvMatches12.size(), W = (N + 7) / 8, flags of the per-set records packed little-endian in bytes):
 *   the whole Initialize (src/Initializer.cc:44-121):
 *     ok int32; R21 float32 [3, 3]; t21 float32 [3]; vP3D float32 [n1, 3]; vbTri uint8 [n1]   (zeros where the reference left them empty)
 *     sets int32 [iterations, 8] (mvSets); m1st, m2nd int32 [N] (mvMatches12); nrand, nsrand int32 (calls of rand / srand it made)
 *   Normalize (:749-795) of both frames:            pn1 [n1, 2], T1 [3, 3], pn2 [n2, 2], T2 [3, 3]  float32
 *   the first n_per_set sets, by the statements of :159-163 and :210-214 on the reference's own ComputeH21 / ComputeF21 /
 *   CheckHomography / CheckFundamental:             Hs, Fs float32 [k, 9]; Hsc, Fsc float32 [k]; Hinl, Finl uint8 [k, W]
 *   FindHomography / FindFundamental (:124-223):    fH, fF float32 [3, 3]; fHsc, fFsc float32; fHinl, fFinl uint8 [N or 0];
 *                                                   fHwin, fFwin int32: the first set whose H21i / F21i is the winner byte for byte
 *   ReconstructH (:572-732) on FindHomography's result and ReconstructF (:470-570) on FindFundamental's, each with
 *   minParallax 1.0 and minTriangulated 50 as Initialize calls them:
 *     Hret, Fret int32; Hmot, Fmot float32 [k, 12]: the motions (R row-major, t) in the order they are handed to CheckRT
 *     (k = 8 / 4, or 0 at an early exit); HR21, Ht21, FR21, Ft21: what came back
 *   CheckRT (:798-907) called once per recorded motion with the same arguments:
 *     Hgood, Fgood int32 [k]; Hvb, Fvb uint8 [k, n1]; Hp3d, Fp3d float32 [k, 3 n1]; Hpar, Fpar float32 [k]
 *
 * The motions.  ReconstructH / ReconstructF keep their candidates in locals and hand them to the private CheckRT, whose first
 * use of them is R.copyTo(P2.rowRange(0,3).colRange(0,3)); t.copyTo(P2.rowRange(0,3).col(3)) (:822-823) after
 * K.copyTo(P1...) (:816).  The shim lets a driver watch the sources of copyTo-into-a-range (cv_linalg.hpp); the driver records
 * them during the one call and takes every (3x3, 3x3, 3x1) group as (K, R, t).
 *
 * Refused (status 2): fewer than 8 matches (the draw of :87-96 reads an empty vector), iterations < 1 (RH is 0 / 0 and
 * ReconstructF gets an empty F), a match index outside the current frame.
 */
#include "ref_solver_io.h"

#define private public
#include "Initializer.h"         // the reference's; Frame.h in it is skipped by solver_standin.h
#undef private

using namespace ORB_SLAM2;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy;

static std::vector<cv::Mat> g_seen;
static void watch(const cv::Mat &src) { g_seen.push_back(src.clone()); }

static void put_mat(refio::Response &out, const char *tag, const cv::Mat &m, int rows, int cols)
{
    std::vector<float> v((size_t)rows * cols, 0.0f);
    if (!m.empty()) {
        if (m.type() != CV_32F || (int)m.total() != rows * cols) refio::refuse("a matrix of an unexpected shape");
        for (int y = 0; y < m.rows; y++)
            for (int x = 0; x < m.cols; x++) v[(size_t)y * m.cols + x] = m.at<float>(y, x);
    }
    out.put(tag, refio::F32, rows, cols, v.data());
}

static void put_points(refio::Response &out, const char *tag, const std::vector<cv::Point2f> &p)
{
    std::vector<float> v(2 * p.size() + 1);
    for (size_t i = 0; i < p.size(); i++) {
        v[2 * i] = p[i].x;
        v[2 * i + 1] = p[i].y;
    }
    out.put(tag, refio::F32, (int)p.size(), 2, v.data());
}

static void pack(const std::vector<bool> &f, unsigned char *dst)
{
    for (size_t i = 0; i < f.size(); i++)
        if (f[i]) dst[i / 8] |= (unsigned char)(1u << (i % 8));
}

static bool same_bytes(const cv::Mat &a, const cv::Mat &b)
{
    for (int i = 0; i < 9; i++)
        if (std::memcmp(&a.at<float>(i / 3, i % 3), &b.at<float>(i / 3, i % 3), 4)) return false;
    return true;
}

/* the motions seen during a Reconstruct call: every (3x3, 3x3, 3x1) group is (K, R, t) of one CheckRT */
static std::vector<std::pair<cv::Mat, cv::Mat> > motions_seen()
{
    std::vector<std::pair<cv::Mat, cv::Mat> > m;
    if (g_seen.size() % 3) refio::refuse("unexpected copies during a Reconstruct call");
    for (size_t i = 0; i < g_seen.size(); i += 3) {
        const cv::Mat &K = g_seen[i], &R = g_seen[i + 1], &t = g_seen[i + 2];
        if (K.rows != 3 || K.cols != 3 || R.rows != 3 || R.cols != 3 || t.rows != 3 || t.cols != 1) refio::refuse("unexpected copies during a Reconstruct call");
        m.push_back(std::make_pair(R, t));
    }
    return m;
}

static void reconstruct_and_check(refio::Response &out, Initializer &init, bool is_h, std::vector<bool> &inl, cv::Mat &M, int n1)
{
    const char *tags_h[] = {"Hret", "Hmot", "HR21", "Ht21", "Hgood", "Hvb", "Hp3d", "Hpar"};
    const char *tags_f[] = {"Fret", "Fmot", "FR21", "Ft21", "Fgood", "Fvb", "Fp3d", "Fpar"};
    const char **tg = is_h ? tags_h : tags_f;
    std::vector<std::pair<cv::Mat, cv::Mat> > mot;
    cv::Mat R21, t21;
    bool ret = false;
    if (!M.empty() && inl.size() == init.mvMatches12.size()) {
        std::vector<cv::Point3f> p;
        std::vector<bool> tri;
        g_seen.clear();
        cv::shim_copy_to_range_hook() = watch;
        ret = is_h ? init.ReconstructH(inl, M, init.mK, R21, t21, p, tri, 1.0, 50) : init.ReconstructF(inl, M, init.mK, R21, t21, p, tri, 1.0, 50);
        cv::shim_copy_to_range_hook() = 0;
        mot = motions_seen();
    }
    const int k = (int)mot.size();
    out.i32(tg[0], ret ? 1 : 0);
    std::vector<float> rt((size_t)k * 12 + 1), p3d((size_t)k * n1 * 3 + 1, 0.0f), par(k + 1);
    std::vector<int32_t> good(k + 1);
    std::vector<unsigned char> vb((size_t)k * n1 + 1, 0);
    for (int j = 0; j < k; j++) {
        for (int i = 0; i < 9; i++) rt[(size_t)j * 12 + i] = mot[j].first.at<float>(i / 3, i % 3);
        for (int i = 0; i < 3; i++) rt[(size_t)j * 12 + 9 + i] = mot[j].second.at<float>(i);
        std::vector<cv::Point3f> p;
        std::vector<bool> g;
        float parallax = 0;
        good[j] = init.CheckRT(mot[j].first, mot[j].second, init.mvKeys1, init.mvKeys2, init.mvMatches12, inl, init.mK, p, 4.0 * init.mSigma2, g, parallax);
        par[j] = parallax;
        if ((int)p.size() != n1 || (int)g.size() != n1) refio::refuse("CheckRT's outputs have an unexpected size");
        for (int i = 0; i < n1; i++) {
            p3d[((size_t)j * n1 + i) * 3] = p[i].x;
            p3d[((size_t)j * n1 + i) * 3 + 1] = p[i].y;
            p3d[((size_t)j * n1 + i) * 3 + 2] = p[i].z;
            vb[(size_t)j * n1 + i] = g[i] ? 1 : 0;
        }
    }
    out.put(tg[1], refio::F32, k, 12, rt.data());
    put_mat(out, tg[2], R21, 3, 3);
    put_mat(out, tg[3], t21, 3, 1);
    out.put(tg[4], refio::I32, 1, k, good.data());
    out.put(tg[5], refio::U8, k, n1, vb.data());
    out.put(tg[6], refio::F32, k, 3 * n1, p3d.data());
    out.put(tg[7], refio::F32, 1, k, par.data());
}

int main(int argc, char **argv)
{
    refio::g_name = "ref_init";
    if (argc != 3) refio::refuse("usage: ref_init REQUEST RESPONSE");
    refio::Request req(argv[1]);
    const refio::Record &rk1 = req.get("keys1", refio::F32, -1, 2), &rk2 = req.get("keys2", refio::F32, -1, 2);
    const int n1 = rk1.rows, n2 = rk2.rows;
    const float *keys1 = rk1.as<float>(refio::F32), *keys2 = rk2.as<float>(refio::F32);
    const int32_t *m12 = req.get("m12", refio::I32, 1, n1).as<int32_t>(refio::I32);
    const float *k = req.get("K", refio::F32, 1, 4).as<float>(refio::F32);
    const float sigma = req.get("sigma", refio::F32, 1, 1).as<float>(refio::F32)[0];
    const int32_t *ip = req.get("ipar", refio::I32, 1, 3).as<int32_t>(refio::I32);
    const int seed = ip[0], iterations = ip[1];
    int matched = 0;
    for (int i = 0; i < n1; i++) {
        if (m12[i] >= n2) refio::refuse("a match index outside the current frame");
        if (m12[i] >= 0) matched++;
    }
    if (matched < 8) refio::refuse("fewer than 8 matches: the draw of src/Initializer.cc:87-96 is undefined there");
    if (iterations < 1) refio::refuse("iterations < 1: RH is 0 / 0 and ReconstructF gets an empty F");
    const int n_per = std::min(std::max((int)ip[2], 0), iterations);

    Frame f1, f2;
    f1.mK = cv::Mat::eye(3, 3, CV_32F);
    f1.mK.at<float>(0, 0) = k[0];
    f1.mK.at<float>(1, 1) = k[1];
    f1.mK.at<float>(0, 2) = k[2];
    f1.mK.at<float>(1, 2) = k[3];
    f2.mK = f1.mK.clone();
    f1.mvKeysUn.resize(n1);
    f2.mvKeysUn.resize(n2);
    for (int i = 0; i < n1; i++) f1.mvKeysUn[i].pt = cv::Point2f(keys1[2 * i], keys1[2 * i + 1]);
    for (int i = 0; i < n2; i++) f2.mvKeysUn[i].pt = cv::Point2f(keys2[2 * i], keys2[2 * i + 1]);

    refio::lcg_seed(seed);
    Initializer init(f1, sigma, iterations);
    refio::Response out(argv[2]);
    {
        cv::Mat R21, t21;
        std::vector<cv::Point3f> p;
        std::vector<bool> tri;
        bool ok = init.Initialize(f2, std::vector<int>(m12, m12 + n1), R21, t21, p, tri);
        out.i32("ok", ok ? 1 : 0);
        put_mat(out, "R21", R21, 3, 3);
        put_mat(out, "t21", t21, 3, 1);
        std::vector<float> pv((size_t)n1 * 3 + 1, 0.0f);
        if (!p.empty() && (int)p.size() != n1) refio::refuse("vP3D has an unexpected size");
        for (size_t i = 0; i < p.size(); i++) {
            pv[3 * i] = p[i].x;
            pv[3 * i + 1] = p[i].y;
            pv[3 * i + 2] = p[i].z;
        }
        out.put("vP3D", refio::F32, n1, 3, pv.data());
        if (!tri.empty() && (int)tri.size() != n1) refio::refuse("vbTriangulated has an unexpected size");
        out.flags("vbTri", tri.empty() ? std::vector<bool>(n1, false) : tri);
    }
    const int N = (int)init.mvMatches12.size(), W = (N + 7) / 8;
    if ((int)init.mvSets.size() != iterations) refio::refuse("mvSets has an unexpected size");
    {
        std::vector<int32_t> sets((size_t)iterations * 8), a(N + 1), b(N + 1);
        for (int it = 0; it < iterations; it++)
            for (int j = 0; j < 8; j++) sets[(size_t)it * 8 + j] = (int32_t)init.mvSets[it][j];
        for (int i = 0; i < N; i++) {
            a[i] = init.mvMatches12[i].first;
            b[i] = init.mvMatches12[i].second;
        }
        out.put("sets", refio::I32, iterations, 8, sets.data());
        out.put("m1st", refio::I32, 1, N, a.data());
        out.put("m2nd", refio::I32, 1, N, b.data());
        out.i32("nrand", refio::g_rand_calls);
        out.i32("nsrand", refio::g_srand_calls);
    }

    std::vector<cv::Point2f> pn1, pn2;
    cv::Mat T1, T2;
    init.Normalize(init.mvKeys1, pn1, T1);
    init.Normalize(init.mvKeys2, pn2, T2);
    put_points(out, "pn1", pn1);
    put_mat(out, "T1", T1, 3, 3);
    put_points(out, "pn2", pn2);
    put_mat(out, "T2", T2, 3, 3);

    /* every set's H21i / F21i, by the statements of :151-163 and :202-214; the first n_per are recorded */
    std::vector<cv::Mat> allH(iterations), allF(iterations);
    std::vector<float> Hs((size_t)n_per * 9 + 1), Fs((size_t)n_per * 9 + 1), Hsc(n_per + 1), Fsc(n_per + 1);
    std::vector<unsigned char> Hinl((size_t)n_per * W + 1, 0), Finl((size_t)n_per * W + 1, 0);
    {
        cv::Mat T2inv = T2.inv(), T2t = T2.t();
        std::vector<cv::Point2f> a(8), b(8);
        for (int it = 0; it < iterations; it++) {
            for (int j = 0; j < 8; j++) {
                int idx = (int)init.mvSets[it][j];
                a[j] = pn1[init.mvMatches12[idx].first];
                b[j] = pn2[init.mvMatches12[idx].second];
            }
            cv::Mat Hn = init.ComputeH21(a, b);
            cv::Mat H21i = T2inv * Hn * T1;
            cv::Mat H12i = H21i.inv();
            cv::Mat Fn = init.ComputeF21(a, b);
            cv::Mat F21i = T2t * Fn * T1;
            allH[it] = H21i.clone();
            allF[it] = F21i.clone();
            if (it >= n_per) continue;
            std::vector<bool> fh(N, false), ff(N, false);
            Hsc[it] = init.CheckHomography(H21i, H12i, fh, init.mSigma);
            Fsc[it] = init.CheckFundamental(F21i, ff, init.mSigma);
            for (int i = 0; i < 9; i++) {
                Hs[(size_t)it * 9 + i] = H21i.at<float>(i / 3, i % 3);
                Fs[(size_t)it * 9 + i] = F21i.at<float>(i / 3, i % 3);
            }
            pack(fh, &Hinl[(size_t)it * W]);
            pack(ff, &Finl[(size_t)it * W]);
        }
    }
    out.put("Hs", refio::F32, n_per, 9, Hs.data());
    out.put("Hsc", refio::F32, 1, n_per, Hsc.data());
    out.put("Hinl", refio::U8, n_per, W, Hinl.data());
    out.put("Fs", refio::F32, n_per, 9, Fs.data());
    out.put("Fsc", refio::F32, 1, n_per, Fsc.data());
    out.put("Finl", refio::U8, n_per, W, Finl.data());

    std::vector<bool> vbH, vbF;                          /* empty on entry, as in Initialize (:100) */
    float SH = 0, SF = 0;
    cv::Mat H, F;
    init.FindHomography(vbH, SH, H);
    init.FindFundamental(vbF, SF, F);
    int winH = -1, winF = -1;
    for (int it = iterations - 1; it >= 0; it--) {
        if (!H.empty() && same_bytes(H, allH[it])) winH = it;
        if (!F.empty() && same_bytes(F, allF[it])) winF = it;
    }
    put_mat(out, "fH", H, 3, 3);
    out.f32("fHsc", SH);
    out.flags("fHinl", vbH);
    out.i32("fHwin", winH);
    put_mat(out, "fF", F, 3, 3);
    out.f32("fFsc", SF);
    out.flags("fFinl", vbF);
    out.i32("fFwin", winF);

    reconstruct_and_check(out, init, true, vbH, H, n1);
    reconstruct_and_check(out, init, false, vbF, F, n1);
    out.close();
    return 0;
}
