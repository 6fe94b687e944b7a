// ORBextractor::ExtractColor the way Tracking::GrabImageMonocular would call it once its cvtColor block (src/Tracking.cc:172-199) is
// gone: the camera's CV_8UC3 / CV_8UC4 frame and mbRGB go to the extractor, which converts on the GPU.  Each result is compared with
// operator() on the grey image the test's numpy oracle made of the same frame.  With argv[1] == "compile-only" nothing runs.
// usage: color_callsites c3.u8 c4.u8 grey_bgr.u8 grey_rgb.u8 W H      (c3 / c4: W x H x 3 / 4 bytes; the greys: W x H)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ORBextractor.h"

static bool load(const char *path, cv::Mat &m)
{
    FILE *f = fopen(path, "rb");
    const size_t n = (size_t)m.rows * m.step;
    const bool ok = f && fread(m.data, 1, n, f) == n;
    if (f) fclose(f);
    return ok;
}
static bool same(const std::vector<cv::KeyPoint> &ka, const cv::Mat &da, const std::vector<cv::KeyPoint> &kb, const cv::Mat &db)
{
    if (ka.size() != kb.size() || ka.empty() || da.rows != db.rows) return false;
    if (memcmp(ka.data(), kb.data(), ka.size() * sizeof(cv::KeyPoint))) return false;
    for (int i = 0; i < da.rows; i++) if (memcmp(da.ptr<unsigned char>(i), db.ptr<unsigned char>(i), 32)) return false;
    return true;
}
static bool level0_is(const ORB_SLAM2::ORBextractor &ex, const cv::Mat &grey)
{
    const cv::Mat &l0 = ex.mvImagePyramid[0];
    if (l0.rows != grey.rows || l0.cols != grey.cols || l0.type() != CV_8UC1) return false;
    for (int y = 0; y < grey.rows; y++) if (memcmp(l0.ptr<unsigned char>(y), grey.ptr<unsigned char>(y), (size_t)grey.cols)) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "compile-only")) return 0;
    if (argc < 7) { fprintf(stderr, "usage: %s c3.u8 c4.u8 grey_bgr.u8 grey_rgb.u8 W H\n", argv[0]); return 2; }
    const int W = atoi(argv[5]), H = atoi(argv[6]);
    cv::Mat c3(H, W, CV_8UC3), c4(H, W, CV_8UC4), gBGR(H, W, CV_8UC1), gRGB(H, W, CV_8UC1);
    if (!load(argv[1], c3) || !load(argv[2], c4) || !load(argv[3], gBGR) || !load(argv[4], gRGB)) { fprintf(stderr, "read failed\n"); return 2; }
    ORB_SLAM2::ORBextractor extractor(1000, 1.2f, 8, 20, 7), plain(1000, 1.2f, 8, 20, 7);
    if (!extractor.Valid() || !plain.Valid()) { fprintf(stderr, "create failed: %s\n", extractor.LastError().c_str()); return 3; }
    int bad = 0;
    auto report = [&](const char *name, bool ok) { printf("%s %d\n", name, ok ? 1 : 0); bad += !ok; };
    for (int rgb = 0; rgb < 2; rgb++) {
        const cv::Mat &grey = rgb ? gRGB : gBGR;
        std::vector<cv::KeyPoint> kRef, k;
        cv::Mat dRef, d;
        plain(grey, cv::Mat(), kRef, dRef);
        extractor.ExtractColor(c3, rgb != 0, k, d);
        report(rgb ? "ExtractColor(CV_8UC3,RGB)" : "ExtractColor(CV_8UC3,BGR)", same(k, d, kRef, dRef) && level0_is(extractor, grey));
        extractor.ExtractColor(c4, rgb != 0, k, d);
        report(rgb ? "ExtractColor(CV_8UC4,RGB)" : "ExtractColor(CV_8UC4,BGR)", same(k, d, kRef, dRef) && level0_is(extractor, grey));
        extractor.ExtractColor(grey, rgb != 0, k, d);
        report(rgb ? "ExtractColor(CV_8UC1,RGB)" : "ExtractColor(CV_8UC1,BGR)", same(k, d, kRef, dRef) && level0_is(extractor, grey));
        extractor(grey, cv::Mat(), k, d);                      // operator() on the handle that has just been colour
        report(rgb ? "operator()(after-RGB)" : "operator()(after-BGR)", same(k, d, kRef, dRef));
    }
    {   // operator() keeps refusing what is not CV_8UC1 (the reference asserts, src/ORBextractor.cc:1052), and so does ExtractColor for float
        std::vector<cv::KeyPoint> k(3);
        cv::Mat d(4, 32, CV_8U), f(H, W, CV_32FC1);
        extractor(c3, cv::Mat(), k, d);
        const bool rej3 = k.empty() && d.empty();
        k.resize(3); d.create(4, 32, CV_8U);
        extractor.ExtractColor(f, false, k, d);
        report("operator()(CV_8UC3)-empty", rej3);
        report("ExtractColor(CV_32FC1)-empty", k.empty() && d.empty());
    }
    return bad ? 1 : 0;
}
