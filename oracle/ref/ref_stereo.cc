/*
 * ref_stereo.cc -- driver that runs the reference's own Frame::ComputeStereoMatches (src/Frame.cc:466-640) on a batch
 * of cases, for tests/test_reference_pin_stereo_cpu.py.
 *
 *   ref_stereo REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  Compiling Frame.cc whole would pull in g2o, Eigen and DBoW2, so the build
 * (oracle/ref/Makefile) slices the function's text out of $(REF_DIR)/src/Frame.cc into oracle/_ref/frame_stereo.inc,
 * and this file includes it inside a minimal ORB_SLAM2::Frame that has only the members the function uses, next to an
 * ORBextractor that holds nothing but mvImagePyramid and an ORBmatcher with TH_HIGH, TH_LOW and DescriptorDistance.  The
 * Mat operations come from the OpenCV shim in cv_shim/.
 *
 * Request (little-endian): int32 magic 'STRQ', int32 ncases, then per case
 *   int32 nlevels; float32 mb, mbf; nlevels x float32 mvScaleFactors; nlevels x float32 mvInvScaleFactors;
 *   the left pyramid, then the right one: per level int32 cols, rows, then rows * cols bytes (row-major);
 *   int32 N, N 28-byte KeyPoints, N x 32 descriptor bytes; int32 Nr, Nr KeyPoints, Nr x 32 descriptor bytes
 * Response: int32 magic 'STRR', then per case N float32 mvuRight and N float32 mvDepth.
 *
 * Every case must lie inside the reference's defined domain (tests/stereo_cases.py).  In particular at least one left
 * keypoint must pass the disparity test: :627 reads vDistIdx[vDistIdx.size()/2] without a check, which UBSan does not
 * flag.  Only N == 0 can be refused here, before the call; the test generators keep to the rest.
 */
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "opencv2/core/core.hpp"

using namespace std;

static_assert(sizeof(cv::KeyPoint) == 28, "cv::KeyPoint layout");

namespace ORB_SLAM2 {

class ORBextractor {
public:
    std::vector<cv::Mat> mvImagePyramid;
};

class ORBmatcher {
public:
    static const int TH_LOW;
    static const int TH_HIGH;
    // the number of differing bits of two 256-bit rows
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b)
    {
        int dist = 0;
        for (int i = 0; i < 32; i++) dist += __builtin_popcount((unsigned)(a.ptr(0)[i] ^ b.ptr(0)[i]));
        return dist;
    }
};
const int ORBmatcher::TH_LOW = 50;
const int ORBmatcher::TH_HIGH = 100;

class Frame {
public:
    void ComputeStereoMatches();

    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    float mbf, mb;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors, mDescriptorsRight;
    std::vector<float> mvScaleFactors, mvInvScaleFactors;
};

#include "frame_stereo.inc"

}  // namespace ORB_SLAM2

static void die(const char *what)
{
    std::fprintf(stderr, "ref_stereo: %s\n", what);
    std::exit(2);
}

struct Reader {
    FILE *f;
    void bytes(void *p, size_t n)
    {
        if (n && std::fread(p, 1, n, f) != n) die("truncated request");
    }
    template <typename T> T get()
    {
        T v;
        bytes(&v, sizeof v);
        return v;
    }
};

static cv::Mat read_level(Reader &r)
{
    const int cols = r.get<int32_t>(), rows = r.get<int32_t>();
    if (cols <= 0 || rows <= 0) die("bad level size");
    cv::Mat m(rows, cols, CV_8UC1);
    for (int y = 0; y < rows; y++) r.bytes(m.ptr(y), (size_t)cols);
    return m;
}

static void read_side(Reader &r, std::vector<cv::KeyPoint> &kps, cv::Mat &desc)
{
    const int n = r.get<int32_t>();
    if (n < 0) die("bad keypoint count");
    kps.resize(n);
    r.bytes(kps.data(), sizeof(cv::KeyPoint) * (size_t)n);
    desc = cv::Mat(n, 32, CV_8UC1);
    for (int i = 0; i < n; i++) r.bytes(desc.ptr(i), 32);
}

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: ref_stereo REQUEST RESPONSE");
    FILE *in = std::fopen(argv[1], "rb");
    FILE *out = std::fopen(argv[2], "wb");
    if (!in || !out) die("cannot open the request or the response");
    Reader r = {in};
    if (r.get<int32_t>() != 0x51525453) die("bad request magic");
    const int ncases = r.get<int32_t>();
    const int32_t magic = 0x52525453;
    std::fwrite(&magic, 4, 1, out);
    for (int c = 0; c < ncases; c++) {
        const int nl = r.get<int32_t>();
        if (nl <= 0 || nl > 32) die("bad nlevels");
        ORB_SLAM2::ORBextractor left, right;
        ORB_SLAM2::Frame F;
        F.mb = r.get<float>();
        F.mbf = r.get<float>();
        F.mvScaleFactors.resize(nl);
        F.mvInvScaleFactors.resize(nl);
        r.bytes(F.mvScaleFactors.data(), 4 * (size_t)nl);
        r.bytes(F.mvInvScaleFactors.data(), 4 * (size_t)nl);
        for (int l = 0; l < nl; l++) left.mvImagePyramid.push_back(read_level(r));
        for (int l = 0; l < nl; l++) right.mvImagePyramid.push_back(read_level(r));
        F.mpORBextractorLeft = &left;
        F.mpORBextractorRight = &right;
        read_side(r, F.mvKeys, F.mDescriptors);
        read_side(r, F.mvKeysRight, F.mDescriptorsRight);
        F.N = (int)F.mvKeys.size();
        if (F.N == 0) die("N == 0: the median of an empty vDistIdx is undefined in the reference");
        F.ComputeStereoMatches();
        std::fwrite(F.mvuRight.data(), 4, (size_t)F.N, out);
        std::fwrite(F.mvDepth.data(), 4, (size_t)F.N, out);
    }
    if (std::fclose(out) != 0) die("cannot write the response");
    std::fclose(in);
    return 0;
}
