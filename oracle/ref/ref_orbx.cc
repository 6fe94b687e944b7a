/*
 * ref_orbx.cc -- driver that runs the reference's own src/ORBextractor.cc (compiled unmodified, on the
 * OpenCV shim in cv_shim/) on a batch of cases, for tests/test_reference_pin_*.py.
 *
 *   ref_orbx REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable on purpose: it replaces the global operator new /
 * delete, and it keeps the reference's code out of the test process.
 *
 * Build variants (oracle/ref/Makefile):
 *   default           bump allocator; cos/sin of computeOrbDescriptor bound to the correctly rounded values
 *   -DREF_NO_BUMP     glibc malloc behind operator new (measurement only)
 *   -DREF_LIBM_SINCOS glibc cosf/sinf (measurement only)
 *
 * Request (little-endian): int32 magic 'ORBQ', int32 ncases, then per case
 *   int32 mode, nfeatures; float32 scaleFactor; int32 nlevels, iniThFAST, minThFAST, blur_mode
 *   mode PYRAMID / LEVELS / EXTRACT: int32 W, H; W*H bytes (row-major, contiguous)
 *   mode OCTREE: int32 n, minX, maxX, minY, maxY, N; n x int32 (x, y, response), coordinates relative to
 *                (minX, minY); each becomes KeyPoint(x, y, 7, -1, response, 0, class_id = its index)
 * Response: int32 magic 'ORBR', then per case int32 mode and
 *   TABLES:  nlevels x float32 scale, inv scale, sigma2, inv sigma2; nlevels x int32 features per level;
 *            int32 16 + umax[16]; int32 512 + the pattern as 512 (x, y) int32 pairs
 *   PYRAMID: per level int32 rows, cols of the bordered level, then its bytes
 *   LEVELS:  per level int32 n + n 28-byte KeyPoints (ComputeKeyPointsOctTree, before descriptors)
 *   OCTREE:  int32 n + n 28-byte KeyPoints (DistributeOctTree's result, in list order)
 *   EXTRACT: int32 n + n 28-byte KeyPoints + n x 32 descriptor bytes (operator())
 */
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include <sys/mman.h>

#include "ORBextractor.h"

static_assert(sizeof(cv::KeyPoint) == 28, "cv::KeyPoint layout");
static_assert(sizeof(cv::Point) == 8, "cv::Point layout");

/* ---- sin / cos of computeOrbDescriptor (src/ORBextractor.cc:115), declared by ref_sincos.h ---- */
namespace ORB_SLAM2 {
#ifdef REF_LIBM_SINCOS
float cos(float x) { return ::cosf(x); }
float sin(float x) { return ::sinf(x); }
#else
float cos(float x) { float c, s; oro_sincos_rad_array(&x, &c, &s, 1); return c; }
float sin(float x) { float c, s; oro_sincos_rad_array(&x, &c, &s, 1); return s; }
#endif
}

/* ---- bump allocator: addresses only grow inside a case, so the (size, pointer) sort of DistributeOctTree
 * (src/ORBextractor.cc:686) orders equal sizes by creation.  Each case starts from the same mark. ---- */
#ifndef REF_NO_BUMP
static char *g_base, *g_cur, *g_end;

static void arena_init()
{
    for (int sh = 40; sh >= 32 && !g_base; sh--) {
        void *p = mmap(0, (size_t)1 << sh, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p != MAP_FAILED) { g_base = g_cur = (char *)p; g_end = g_base + ((size_t)1 << sh); }
    }
    if (!g_base) { std::fprintf(stderr, "ref_orbx: cannot reserve the arena\n"); std::abort(); }
}

static void *bump(size_t n)
{
    if (!g_base) arena_init();
    n = (n + 15) & ~(size_t)15;
    if (n == 0) n = 16;
    if ((size_t)(g_end - g_cur) < n) { std::fprintf(stderr, "ref_orbx: arena exhausted\n"); std::abort(); }
    void *p = g_cur;
    g_cur += n;
    return p;
}

void *operator new(size_t n) { return bump(n); }
void *operator new[](size_t n) { return bump(n); }
void *operator new(size_t n, const std::nothrow_t &) noexcept { return bump(n); }
void *operator new[](size_t n, const std::nothrow_t &) noexcept { return bump(n); }
void operator delete(void *) noexcept {}
void operator delete[](void *) noexcept {}
void operator delete(void *, size_t) noexcept {}
void operator delete[](void *, size_t) noexcept {}

static char *case_mark() { if (!g_base) arena_init(); return g_cur; }
/* nothing allocated inside a case outlives it: give the pages back and start the next case at the same address */
static void case_reset(char *mark)
{
    const size_t pg = 4096;
    char *lo = (char *)(((uintptr_t)mark + pg - 1) & ~(uintptr_t)(pg - 1));
    if (g_cur > lo) madvise(lo, (size_t)(g_cur - lo), MADV_DONTNEED);
    g_cur = mark;
}
#else
static char *case_mark() { return 0; }
static void case_reset(char *) {}
#endif

/* ---- the probe: reaches the extractor's protected members ---- */
class Probe : public ORB_SLAM2::ORBextractor {
public:
    Probe(int nf, float sf, int nl, int ini, int mn) : ORBextractor(nf, sf, nl, ini, mn) {}
    using ORBextractor::ComputePyramid;
    using ORBextractor::ComputeKeyPointsOctTree;
    using ORBextractor::DistributeOctTree;
    using ORBextractor::mnFeaturesPerLevel;
    using ORBextractor::umax;
    using ORBextractor::pattern;
    using ORBextractor::mvScaleFactor;
    using ORBextractor::mvInvScaleFactor;
    using ORBextractor::mvLevelSigma2;
    using ORBextractor::mvInvLevelSigma2;
};

enum { M_TABLES = 0, M_PYRAMID = 1, M_LEVELS = 2, M_OCTREE = 3, M_EXTRACT = 4 };

static const unsigned char *g_in, *g_in_end;
static FILE *g_out;

static void fail(const char *m) { std::fprintf(stderr, "ref_orbx: %s\n", m); std::exit(2); }
static void rd(void *p, size_t n)
{
    if ((size_t)(g_in_end - g_in) < n) fail("truncated request");
    std::memcpy(p, g_in, n);
    g_in += n;
}
static int32_t rd_i() { int32_t v; rd(&v, 4); return v; }
static float rd_f() { float v; rd(&v, 4); return v; }
static void wr(const void *p, size_t n) { if (n && std::fwrite(p, 1, n, g_out) != n) fail("write failed"); }
static void wr_i(int32_t v) { wr(&v, 4); }
static void wr_kps(const std::vector<cv::KeyPoint> &k)
{
    wr_i((int32_t)k.size());
    if (!k.empty()) wr(k.data(), k.size() * sizeof(cv::KeyPoint));
}
template <typename T> static void wr_vec(const std::vector<T> &v, int n) { for (int i = 0; i < n; i++) wr(&v[i], 4); }

static void run_case()
{
    const int mode = rd_i(), nf = rd_i();
    const float sf = rd_f();
    const int nl = rd_i(), ini = rd_i(), mn = rd_i(), blur = rd_i();
    cv::shim_set_blur_mode(blur);
    wr_i(mode);
    Probe ex(nf, sf, nl, ini, mn);
    if (mode == M_TABLES) {
        wr_vec(ex.mvScaleFactor, nl); wr_vec(ex.mvInvScaleFactor, nl);
        wr_vec(ex.mvLevelSigma2, nl); wr_vec(ex.mvInvLevelSigma2, nl);
        wr_vec(ex.mnFeaturesPerLevel, nl);
        wr_i((int32_t)ex.umax.size()); wr_vec(ex.umax, (int)ex.umax.size());
        wr_i((int32_t)ex.pattern.size()); wr(ex.pattern.data(), ex.pattern.size() * sizeof(cv::Point));
        return;
    }
    if (mode == M_OCTREE) {
        const int n = rd_i(), minX = rd_i(), maxX = rd_i(), minY = rd_i(), maxY = rd_i(), N = rd_i();
        std::vector<cv::KeyPoint> v;
        v.reserve(n);
        for (int i = 0; i < n; i++) {
            int x = rd_i(), y = rd_i(), r = rd_i();
            v.push_back(cv::KeyPoint((float)x, (float)y, 7.f, -1, (float)r, 0, i));
        }
        wr_kps(ex.DistributeOctTree(v, minX, maxX, minY, maxY, N, 0));
        return;
    }
    const int W = rd_i(), H = rd_i();
    if (W <= 0 || H <= 0) fail("bad image size");
    unsigned char *img = (unsigned char *)std::malloc((size_t)W * H);
    rd(img, (size_t)W * H);
    cv::Mat m(H, W, CV_8UC1, img, (size_t)W);
    if (mode == M_PYRAMID || mode == M_LEVELS) {
        ex.ComputePyramid(m);
        if (mode == M_PYRAMID) {
            for (int l = 0; l < nl; l++) {
                cv::Mat b = ex.mvImagePyramid[l];
                b.adjustROI(19, 19, 19, 19);
                wr_i(b.rows); wr_i(b.cols);
                for (int y = 0; y < b.rows; y++) wr(b.ptr(y), (size_t)b.cols);
            }
        } else {
            std::vector<std::vector<cv::KeyPoint> > all;
            ex.ComputeKeyPointsOctTree(all);
            for (int l = 0; l < nl; l++) wr_kps(all[l]);
        }
    } else if (mode == M_EXTRACT) {
        std::vector<cv::KeyPoint> kps;
        cv::Mat desc;
        ex(m, cv::Mat(), kps, desc);
        wr_kps(kps);
        for (size_t i = 0; i < kps.size(); i++) wr(desc.ptr((int)i), 32);
    } else {
        fail("unknown mode");
    }
    std::free(img);
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ref_orbx REQUEST RESPONSE\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) fail("cannot open the request");
    std::fseek(f, 0, SEEK_END);
    long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    unsigned char *buf = (unsigned char *)std::malloc(sz > 0 ? (size_t)sz : 1);
    if (sz < 0 || std::fread(buf, 1, (size_t)sz, f) != (size_t)sz) fail("cannot read the request");
    std::fclose(f);
    g_in = buf; g_in_end = buf + sz;
    if (rd_i() != 0x5142524f) fail("bad request magic");
    const int ncases = rd_i();
    g_out = std::fopen(argv[2], "wb");
    if (!g_out) fail("cannot open the response");
    wr_i(0x5252424f);
    for (int c = 0; c < ncases; c++) {
        char *mark = case_mark();
        run_case();
        case_reset(mark);
    }
    if (std::fclose(g_out) != 0) fail("cannot close the response");
    std::free(buf);
    return 0;
}
