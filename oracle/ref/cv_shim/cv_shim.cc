/* cv_shim.cc -- the shim's image operations, each one a call of the matching oracle primitive. */
#include "cv_shim.hpp"

namespace cv {

static int g_blur_mode = ORO_BLUR_SCALAR;

void shim_set_blur_mode(int mode) { g_blur_mode = mode; }

static void die(const char *what)
{
    std::fprintf(stderr, "cv_shim: unsupported call: %s\n", what);
    std::abort();
}

/* cv::FAST(image, keypoints, threshold, nonmax) with the 9/16 detector: KeyPoint(x, y, 7, -1, score) per corner,
 * in the detector's row-major order; the output vector is cleared first. */
void FAST(InputArray image, std::vector<KeyPoint> &keypoints, int threshold, bool nonmaxSuppression)
{
    Mat m = image.getMat();
    keypoints.clear();
    if (m.empty()) return;
    int cap = m.rows * m.cols + 1;
    oro_cand *c = (oro_cand *)std::malloc(sizeof(oro_cand) * (size_t)cap);
    int n = oro_fast9_16(m.data, (int)m.step, m.cols, m.rows, threshold, nonmaxSuppression ? 1 : 0, c, cap);
    if (n < 0) die("FAST capacity");
    for (int i = 0; i < n; i++)
        keypoints.push_back(KeyPoint((float)c[i].x, (float)c[i].y, 7.f, -1, (float)c[i].response));
    std::free(c);
}

void resize(InputArray src, OutputArray dst, Size dsize, double fx, double fy, int interpolation)
{
    if (interpolation != INTER_LINEAR || fx != 0 || fy != 0 || dsize.width <= 0 || dsize.height <= 0) die("resize");
    Mat s = src.getMat();
    dst.create(dsize, CV_8UC1);
    Mat d = dst.getMat();
    oro_resize_linear(s.data, s.cols, s.rows, (int)s.step, d.data, d.cols, d.rows, (int)d.step);
}

/* BORDER_REFLECT_101, with or without BORDER_ISOLATED; the source is always treated as an isolated image.
 * The result is built aside first: the reference's destination holds the source as its interior. */
void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType,
                    const Scalar &)
{
    if ((borderType & ~BORDER_ISOLATED) != BORDER_REFLECT_101 || top != bottom || top != left || top != right || top < 0)
        die("copyMakeBorder");
    Mat s = src.getMat();
    const int b = top, ow = s.cols + 2 * b, oh = s.rows + 2 * b;
    std::vector<uchar> tmp((size_t)ow * oh);
    oro_copy_make_border101(s.data, s.cols, s.rows, (int)s.step, tmp.data(), ow, b);
    dst.create(oh, ow, CV_8UC1);
    Mat d = dst.getMat();
    for (int y = 0; y < oh; y++) std::memcpy(d.ptr(y), tmp.data() + (size_t)y * ow, (size_t)ow);
}

/* GaussianBlur(src, dst, Size(7, 7), 2, 2, BORDER_REFLECT_101) on 8-bit data, column rounding per shim_set_blur_mode */
void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY, int borderType)
{
    if (ksize.width != 7 || ksize.height != 7 || sigmaX != 2 || sigmaY != 2 || borderType != BORDER_REFLECT_101)
        die("GaussianBlur");
    static oro_extractor kern;
    static bool have = false;
    if (!have) { oro_extractor_init(&kern, 1, 1.2f, 1, 20, 7); have = true; }
    Mat s = src.getMat();
    std::vector<uchar> tmp((size_t)s.cols * s.rows ? (size_t)s.cols * s.rows : 1);
    oro_gaussian_blur7(s.data, s.cols, s.rows, (int)s.step, tmp.data(), s.cols, kern.gauss_k, g_blur_mode);
    dst.create(s.rows, s.cols, CV_8UC1);
    Mat d = dst.getMat();
    for (int y = 0; y < s.rows; y++) std::memcpy(d.ptr(y), tmp.data() + (size_t)y * s.cols, (size_t)s.cols);
}

} // namespace cv
