// initializer_callsites.cc -- the Initializer lines of Tracking::MonocularInitialization (src/Tracking.cc:589 and :623 of the
// reference) against my-slam_amd/host/Initializer.h, verbatim, on a frame class with the two members the adapter reads (mK,
// mvKeysUn; tests/cxx/slam_shims/Frame.h plus mK) and orbx_cv_compat.h.
// usage: initializer_callsites compile-only | initializer_callsites host (no GPU: every hypothesis on the host) |
//        initializer_callsites (needs a GPU: the same calls through the GPU and on the host, compared call by call)
//
// Scenes: a planted motion seen by two frames; points in a volume (the fundamental route) and on a plane (the homography route),
// 0.2 px of noise, a fifth of the matches wrong; a pure rotation, which must be refused; 7 matches, which must be refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "Frame.h"
#include "Initializer.h"

using namespace std;
using namespace ORB_SLAM2;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct Lcg { unsigned s; };
static int lcg_next(void *ctx) { Lcg *g = (Lcg *)ctx; g->s = (1103515245u * g->s + 12345u) & 0x7fffffffu; return (int)g->s; }
static double uni(Lcg &g, double a, double b) { return a + (b - a) * (lcg_next(&g) / 2147483648.0); }

// the frame of the reference has mK next to mvKeysUn (include/Frame.h:108, :134); the shared shim has no use for it elsewhere
struct TrackFrame : public Frame { cv::Mat mK; };

static const float FX = 517.3f, FY = 516.5f, CX = 318.6f, CY = 255.3f;

struct Scene {
    TrackFrame f1, f2;
    vector<int> matches;
    double R[9], t[3];
    vector<double> X;                   // the point of every key of frame 1 (camera 1)
    vector<bool> wrong;
};

static void make_scene(Scene &sc, int n, bool plane, bool rotation_only, int n_wrong, unsigned seed)
{
    Lcg g{seed};
    const double th = 0.09, c = cos(th), s = sin(th);
    const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {rotation_only ? 0.0 : -1.0, rotation_only ? 0.0 : 0.05, rotation_only ? 0.0 : 0.03};
    memcpy(sc.R, R, sizeof R); memcpy(sc.t, t, sizeof t);
    cv::Mat K(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) K.at<float>(i / 3, i % 3) = 0.f;
    K.at<float>(0, 0) = FX; K.at<float>(1, 1) = FY; K.at<float>(0, 2) = CX; K.at<float>(1, 2) = CY; K.at<float>(2, 2) = 1.f;
    sc.f1.mK = K.clone(); sc.f2.mK = K.clone();
    const int extra = n / 4 + 2;
    sc.f1.mvKeysUn.resize(n + extra); sc.f2.mvKeysUn.resize(n + extra);
    sc.matches.assign(n + extra, -1);
    sc.X.assign(3 * (size_t)(n + extra), 0.0);
    sc.wrong.assign(n + extra, false);
    for (int i = 0; i < n + extra; i++) {
        const double x = uni(g, -3, 3), y = uni(g, -2, 2), z = plane ? 6 + 1.0 * x - 0.5 * y : uni(g, 4, 10);
        const double p[3] = {x, y, z};
        double q[3];
        for (int k = 0; k < 3; k++) q[k] = R[3 * k] * p[0] + R[3 * k + 1] * p[1] + R[3 * k + 2] * p[2] + t[k];
        memcpy(&sc.X[3 * (size_t)i], p, sizeof p);
        sc.f1.mvKeysUn[i].pt = cv::Point2f((float)(FX * p[0] / p[2] + CX + uni(g, -0.2, 0.2)), (float)(FY * p[1] / p[2] + CY + uni(g, -0.2, 0.2)));
        // key i of frame 1 is key (n + extra - 1 - i) of frame 2
        const int j = n + extra - 1 - i;
        float u = (float)(FX * q[0] / q[2] + CX + uni(g, -0.2, 0.2)), v = (float)(FY * q[1] / q[2] + CY + uni(g, -0.2, 0.2));
        if (i < n_wrong) { u += 90.f; v -= 70.f; sc.wrong[i] = true; }
        sc.f2.mvKeysUn[j].pt = cv::Point2f(u, v);
        if (i < n) sc.matches[i] = j;
    }
    sc.f1.N = sc.f2.N = n + extra;
}

struct Outcome { bool ok = false; cv::Mat R, t; vector<cv::Point3f> P; vector<bool> tri; bool usedGpu = false; string err; };

// Tracking's members around the two lines
struct TrackingLike {
    Initializer *mpInitializer = nullptr;
    TrackFrame mInitialFrame, mCurrentFrame;
    vector<int> mvIniMatches;
    vector<cv::Point3f> mvIniP3D;

    Outcome run(Scene &sc, bool gpu, unsigned seed)
    {
        Outcome out;
        Lcg g{seed};
        mCurrentFrame = sc.f1;
        {
            // src/Tracking.cc:586-589
            if(mpInitializer)
                delete mpInitializer;

            mpInitializer =  new Initializer(mCurrentFrame,1.0,200);
        }
        mInitialFrame = mCurrentFrame;
        mpInitializer->SetRand(lcg_next, &g, 0x7fffffff);
        mpInitializer->SetUseGpu(gpu);
        mCurrentFrame = sc.f2;
        mvIniMatches = sc.matches;
        mvIniP3D.clear();

        cv::Mat Rcw; // Current Camera Rotation
        cv::Mat tcw; // Current Camera Translation
        vector<bool> vbTriangulated; // Triangulated Correspondences (mvIniMatches)

        // src/Tracking.cc:623
        if(mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated))
        {
            out.ok = true;
        }
        out.R = Rcw; out.t = tcw; out.P = mvIniP3D; out.tri = vbTriangulated;
        out.usedGpu = mpInitializer->LastUsedGpu(); out.err = mpInitializer->LastError();
        return out;
    }
    ~TrackingLike() { delete mpInitializer; }
};

static void check_planted(const Scene &sc, const Outcome &o, int n)
{
    CHECK(o.ok);
    if (!o.ok) return;
    CHECK(o.R.rows == 3 && o.R.cols == 3 && o.t.rows == 3 && o.t.cols == 1 && o.P.size() == sc.matches.size() && o.tri.size() == sc.matches.size());
    const double tn = sqrt(sc.t[0] * sc.t[0] + sc.t[1] * sc.t[1] + sc.t[2] * sc.t[2]);
    double worstR = 0, worstT = 0;
    for (int i = 0; i < 9; i++) worstR = fmax(worstR, fabs(o.R.at<float>(i / 3, i % 3) - sc.R[i]));
    for (int i = 0; i < 3; i++) worstT = fmax(worstT, fabs(o.t.at<float>(i) - sc.t[i] / tn));
    CHECK(worstR < 0.05 && worstT < 0.2);
    int nTri = 0;
    for (size_t i = 0; i < o.tri.size(); i++) {
        if (!o.tri[i]) continue;
        nTri++;
        CHECK((int)i < n && !sc.wrong[i]);                                     // only keys with a correct match
        CHECK(fabs(o.P[i].z * tn - sc.X[3 * i + 2]) < 0.5 * sc.X[3 * i + 2]);    // the depth, up to the scale |t| = 1 fixes
    }
    CHECK(nTri > 50);
    printf("  R %.2e t %.2e, %d triangulated\n", worstR, worstT, nTri);
}

static bool same(const Outcome &a, const Outcome &b)
{
    if (a.ok != b.ok || a.R.empty() != b.R.empty() || a.t.empty() != b.t.empty() || a.P.size() != b.P.size() || a.tri != b.tri) return false;
    if (!a.R.empty() && memcmp(a.R.ptr<float>(), b.R.ptr<float>(), 36)) return false;
    if (!a.t.empty() && (a.t.at<float>(0) != b.t.at<float>(0) || a.t.at<float>(1) != b.t.at<float>(1) || a.t.at<float>(2) != b.t.at<float>(2))) return false;
    return a.P.empty() || !memcmp(a.P.data(), b.P.data(), a.P.size() * sizeof(cv::Point3f));
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    const bool host_only = argc > 1 && !strcmp(argv[1], "host");
    struct Spec { const char *name; int n; bool plane, rot; int wrong; bool expect; } specs[] = {
        {"general", 150, false, false, 30, true}, {"plane", 150, true, false, 30, true}, {"rotation", 150, false, true, 30, false},
        {"general65", 65, false, false, 0, true}, {"seven", 7, false, false, 0, false}};
    for (const Spec &sp : specs) {
        Scene sc;
        make_scene(sc, sp.n, sp.plane, sp.rot, sp.wrong, 11);
        TrackingLike trH;
        printf("%s\n", sp.name);
        const Outcome h = trH.run(sc, false, 3);
        CHECK(h.ok == sp.expect && !h.usedGpu);
        if (sp.expect) check_planted(sc, h, sp.n);
        if (sp.n < 8) CHECK(!h.err.empty());                                  // RandomInt(0, -1) in the reference: refused here
        const Outcome h2 = trH.run(sc, false, 3);                             // the object is rebuilt as Tracking does: the same bytes again
        CHECK(same(h, h2));
        if (host_only) continue;
        TrackingLike trG;
        const Outcome g = trG.run(sc, true, 3);
        CHECK(sp.n < 8 || (g.usedGpu && g.err.empty()));
        if (!g.err.empty()) printf("  GPU path: %s\n", g.err.c_str());
        CHECK(same(g, h));
        printf("  GPU and host runs agree\n");
    }
    if (g_fail) { printf("initializer_callsites: %d checks failed\n", g_fail); return 1; }
    printf("initializer_callsites ok\n");
    return 0;
}
