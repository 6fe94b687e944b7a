/*
 * cv_shim.hpp -- the small slice of the OpenCV 3.x C++ API that src/ORBextractor.cc and
 * include/ORBextractor.h use, written from the public API documentation alone.  Every image
 * operation forwards to the oracle's primitive (oracle/orb_oracle.h), so the reference's own
 * ORBextractor.cc runs unmodified on top of the project's reading of OpenCV 3.1.0's arithmetic.
 *
 * TEST INFRASTRUCTURE ONLY: linked into oracle/_ref/ref_orbx (oracle/ref/ref_orbx.cc) and
 * oracle/_ref/ref_stereo (oracle/ref/ref_stereo.cc), never into the library.  Scope:
 *   - Mat: single-channel 8-bit or 32-bit float, reference counted, with ROI views (operator()(Rect),
 *     rowRange, colRange, row, adjustROI).  A view keeps its parent buffer alive.  An ROI outside
 *     the matrix aborts, as OpenCV's CV_Assert does.
 *   - what Frame::ComputeStereoMatches uses on float windows: convertTo(CV_32F), at<float>,
 *     Mat::ones, scalar * Mat and Mat - Mat (evaluated at once: MatExpr is not modelled), and
 *     norm(a, b, NORM_L1) (a double sum of |a - b|).
 *   - copyMakeBorder treats its source as an isolated image (BORDER_ISOLATED or not); the
 *     driver only hands the extractor whole images.
 *   - KeyPointsFilter::retainBest is only reached from ComputeKeyPointsOld, which the
 *     reference never calls; it aborts.
 *   - what Thirdparty/DBoW2 uses (oracle/ref/ref_dbow.cc): a descriptor is a 1 x 32 CV_8U row read through
 *     ptr<T>(); FileStorage / FileNode are no-ops that only let the yml save / load members compile
 *     (isOpened() is false, so both throw before they touch a node).
 *   - with CV_SHIM_LINALG defined (oracle/ref/solver_standin.h), and only then: CV_64F matrices and the linear algebra that
 *     src/Sim3Solver.cc, src/PnPsolver.cc and src/Initializer.cc use, in cv_linalg.hpp.  Without the macro this header is the
 *     text the pins above have always compiled.
 */
#ifndef ORBX_CV_SHIM_HPP
#define ORBX_CV_SHIM_HPP

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "orb_oracle.h"

typedef unsigned char uchar;

#define CV_8U 0
#define CV_8UC1 0
#define CV_32F 5
#define CV_32FC1 5
#define CV_PI 3.1415926535897932384626433832795
#ifdef CV_SHIM_LINALG            /* the solvers' pin (cv_linalg.hpp): double matrices beside the two above */
#define CV_64F 6
#define CV_64FC1 6
#endif

namespace cv {

enum { BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4, BORDER_ISOLATED = 16 };
enum { INTER_LINEAR = 1 };
enum { NORM_L1 = 2 };

/* GaussianBlur's column rounding (ORO_BLUR_SCALAR or ORO_BLUR_X86_SIMD); set by the driver */
void shim_set_blur_mode(int mode);

inline int cvRound(double v) { return oro_cv_round(v); }
inline int cvRound(float v) { return oro_cv_round((double)v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(double v) { return (int)std::floor(v); }
inline int cvFloor(float v) { return (int)std::floor(v); }
inline int cvCeil(double v) { return (int)std::ceil(v); }
inline int cvCeil(float v) { return (int)std::ceil(v); }
inline float fastAtan2(float y, float x) { return oro_fast_atan2(y, x); }

template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;
#ifdef CV_SHIM_LINALG
template <typename T> struct Point3_ {
    T x, y, z;
    Point3_() : x(0), y(0), z(0) {}
    Point3_(T x_, T y_, T z_) : x(x_), y(y_), z(z_) {}
};
typedef Point3_<float> Point3f;
#endif

/* OpenCV: a.x = saturate_cast<T>(a.x * b) -- a float product for Point2f */
inline Point2f &operator*=(Point2f &a, float b)
{
    a.x = a.x * b;
    a.y = a.y * b;
    return a;
}

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

struct Scalar {
    double v;
    Scalar(double a = 0) : v(a) {}
};

struct Range {
    int start, end;
    Range(int s, int e) : start(s), end(e) {}
};

class KeyPoint {
public:
    KeyPoint() : pt(0.f, 0.f), size(0.f), angle(-1.f), response(0.f), octave(0), class_id(-1) {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0,
             int class_id_ = -1)
        : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
    Point2f pt;
    float size;
    float angle;
    float response;
    int octave;
    int class_id;
};

struct MatZeros { int rows, cols, type; };
#ifdef CV_SHIM_LINALG
class MatExpr;
#endif

class Mat {
public:
    int rows, cols;
    uchar *data;
    size_t step;

    Mat() : rows(0), cols(0), data(0), step(0), type_(CV_8UC1), whole_rows_(0), whole_cols_(0), buf_() {}
    Mat(int r, int c, int type) : Mat() { create(r, c, type); }
    Mat(Size sz, int type) : Mat() { create(sz.height, sz.width, type); }
    /* user data: not owned */
    Mat(int r, int c, int type, void *ptr, size_t step_ = 0)
        : rows(r), cols(c), data((uchar *)ptr), step(step_ ? step_ : (size_t)c * elem(type)), type_(type), whole_rows_(r),
          whole_cols_(c), base_((uchar *)ptr), buf_()
    {
        check_type(type);
    }

    static MatZeros zeros(int r, int c, int type) { MatZeros z = {r, c, type}; return z; }
    static Mat ones(int r, int c, int type)
    {
        if (type != CV_32F) { std::fprintf(stderr, "cv_shim: Mat::ones is CV_32F only\n"); std::abort(); }
        Mat m(r, c, type);
        for (int y = 0; y < r; y++)
            for (int x = 0; x < c; x++) m.at<float>(y, x) = 1.0f;
        return m;
    }

    /* MatExpr assignment: evaluated into this matrix, which is reallocated only on a size change */
    Mat &operator=(const MatZeros &z)
    {
        create(z.rows, z.cols, z.type);
        for (int y = 0; y < rows; y++) std::memset(ptr(y), 0, (size_t)cols * elemSize());
        return *this;
    }

    void create(int r, int c, int type)
    {
        check_type(type);
        if (data && r == rows && c == cols && type == type_) return;
        release();
        type_ = type;
        rows = r; cols = c; step = (size_t)c * elem(type);
        whole_rows_ = r; whole_cols_ = c;
        size_t n = (size_t)r * step;
        buf_ = std::shared_ptr<std::vector<uchar> >(new std::vector<uchar>(n ? n : 1));
        data = buf_->data();
        base_ = data;
    }
    void create(Size sz, int type) { create(sz.height, sz.width, type); }
    void release() { buf_.reset(); data = 0; rows = cols = 0; step = 0; }
    bool empty() const { return data == 0 || rows == 0 || cols == 0; }
    int type() const { return type_; }
    size_t elemSize() const { return elem(type_); }
    size_t step1() const { return step / elemSize(); }
    size_t total() const { return (size_t)rows * cols; }
    Size size() const { return Size(cols, rows); }
    bool isContinuous() const { return step == (size_t)cols * elemSize() || rows == 1; }

    uchar *ptr(int y = 0) { return data + (size_t)y * step; }
    const uchar *ptr(int y = 0) const { return data + (size_t)y * step; }
    template <typename T> T *ptr(int y = 0) { return (T *)(data + (size_t)y * step); }
    template <typename T> const T *ptr(int y = 0) const { return (const T *)(data + (size_t)y * step); }
    template <typename T> T &at(int y, int x) { return *(T *)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
    template <typename T> const T &at(int y, int x) const { return *(const T *)(data + (size_t)y * step + (size_t)x * sizeof(T)); }

    Mat operator()(const Rect &r) const
    {
        check_range(r.y, r.y + r.height, rows); check_range(r.x, r.x + r.width, cols);
        Mat m(*this);
        m.data = data + (size_t)r.y * step + (size_t)r.x * elemSize();
        m.rows = r.height; m.cols = r.width;
        return m;
    }
    Mat rowRange(int a, int b) const { return (*this)(Rect(0, a, cols, b - a)); }
    Mat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }
    Mat row(int y) const { return rowRange(y, y + 1); }

    /* into a new CV_32F matrix (from 8-bit or float), then assigned to dst (which may be this matrix) */
    void convertTo(Mat &dst, int rtype) const
    {
#ifdef CV_SHIM_LINALG
        if (rtype == CV_32F && type_ == CV_64F) {                 /* each double rounded to float once */
            Mat narrow(rows, cols, CV_32F);
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < cols; x++) narrow.at<float>(y, x) = (float)at<double>(y, x);
            dst = narrow;
            return;
        }
#endif
        if (rtype != CV_32F) { std::fprintf(stderr, "cv_shim: convertTo is CV_32F only\n"); std::abort(); }
        Mat out(rows, cols, CV_32F);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) out.at<float>(y, x) = type_ == CV_32F ? at<float>(y, x) : (float)ptr(y)[x];
        dst = out;
    }

    /* grows or shrinks the view inside its parent buffer, clipped to the parent */
    Mat &adjustROI(int dtop, int dbottom, int dleft, int dright)
    {
        ptrdiff_t off = data - base_;
        int y0 = (int)(off / (ptrdiff_t)step), x0 = (int)(off % (ptrdiff_t)step);
        int ny0 = std::max(y0 - dtop, 0), nx0 = std::max(x0 - dleft, 0);
        int ny1 = std::min(y0 + rows + dbottom, whole_rows_), nx1 = std::min(x0 + cols + dright, whole_cols_);
        data = base_ + (size_t)ny0 * step + nx0;
        rows = ny1 - ny0; cols = nx1 - nx0;
        return *this;
    }

    Mat clone() const
    {
        Mat m(rows, cols, type_);
        for (int y = 0; y < rows; y++) std::memcpy(m.ptr(y), ptr(y), (size_t)cols * elemSize());
        return m;
    }
    void copyTo(Mat &dst) const
    {
        if (dst.data == data && dst.step == step && dst.rows == rows && dst.cols == cols && dst.type_ == type_) return;
        Mat tmp = clone();
        dst.create(rows, cols, type_);
        for (int y = 0; y < rows; y++) std::memcpy(dst.ptr(y), tmp.ptr(y), (size_t)cols * elemSize());
    }

#ifdef CV_SHIM_LINALG
    /* cv_linalg.hpp: what src/Sim3Solver.cc, src/PnPsolver.cc and src/Initializer.cc use beyond the above */
    Mat(int r, int c, int type, const Scalar &s);
    Mat(const MatZeros &z) : Mat() { *this = z; }
    Mat &operator=(const MatExpr &e);
    Mat &operator*=(double s);
    MatExpr t() const;
    MatExpr inv() const;
    double dot(const Mat &b) const;
    Mat cross(const Mat &b) const;
    Mat col(int x) const { return colRange(x, x + 1); }
    Mat reshape(int cn, int new_rows) const;
    static Mat eye(int r, int c, int type);
    static Mat diag(const Mat &d);
    void copyTo(Mat &&view) const;
    /* one index: a vector's element (a column vector may be a view with a step) or a matrix element in row-major order */
    template <typename T> T &at(int i)
    {
        return *(T *)(data + (cols == 1 ? (size_t)i * step : (size_t)(i / cols) * step + (size_t)(i % cols) * sizeof(T)));
    }
    template <typename T> const T &at(int i) const { return const_cast<Mat *>(this)->at<T>(i); }
#endif

private:
#ifdef CV_SHIM_LINALG
    static size_t elem(int type) { return type == CV_64F ? 8 : type == CV_32F ? 4 : 1; }
#else
    static size_t elem(int type) { return type == CV_32F ? 4 : 1; }
#endif
    static void check_type(int type)
    {
#ifdef CV_SHIM_LINALG
        if (type == CV_64F) return;
#endif
        if (type != CV_8UC1 && type != CV_32F) { std::fprintf(stderr, "cv_shim: only CV_8UC1 and CV_32F\n"); std::abort(); }
    }
    static void check_range(int a, int b, int n)
    {
        if (a < 0 || b < a || b > n) { std::fprintf(stderr, "cv_shim: ROI [%d,%d) outside [0,%d)\n", a, b, n); std::abort(); }
    }
    int type_;
    int whole_rows_, whole_cols_;
    uchar *base_ = 0;
    std::shared_ptr<std::vector<uchar> > buf_;
};

#ifndef CV_SHIM_LINALG           /* cv_linalg.hpp has both as MatExpr, with the same arithmetic */
/* scalar * Mat and Mat - Mat on CV_32F: each element rounded to float once, as saturate_cast<float> does */
inline Mat operator*(double s, const Mat &m)
{
    if (m.type() != CV_32F) { std::fprintf(stderr, "cv_shim: scalar * Mat is CV_32F only\n"); std::abort(); }
    Mat out(m.rows, m.cols, CV_32F);
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) out.at<float>(y, x) = (float)(s * (double)m.at<float>(y, x));
    return out;
}

inline Mat operator-(const Mat &a, const Mat &b)
{
    if (a.type() != CV_32F || b.type() != CV_32F || a.rows != b.rows || a.cols != b.cols) {
        std::fprintf(stderr, "cv_shim: Mat - Mat needs two CV_32F matrices of one size\n");
        std::abort();
    }
    Mat out(a.rows, a.cols, CV_32F);
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) out.at<float>(y, x) = a.at<float>(y, x) - b.at<float>(y, x);
    return out;
}
#endif

/* NORM_L1 of a - b for CV_32F: the differences in float, their absolute values summed in double */
inline double norm(const Mat &a, const Mat &b, int normType)
{
    if (normType != NORM_L1 || a.type() != CV_32F || b.type() != CV_32F || a.rows != b.rows || a.cols != b.cols) {
        std::fprintf(stderr, "cv_shim: norm is NORM_L1 of two CV_32F matrices of one size only\n");
        std::abort();
    }
    double s = 0;
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) s += std::fabs((double)(a.at<float>(y, x) - b.at<float>(y, x)));
    return s;
}

class _InputArray {
public:
    _InputArray() : m_(0) {}
    _InputArray(const Mat &m) : m_(&m) {}
    Mat getMat() const { return m_ ? *m_ : Mat(); }
    bool empty() const { return !m_ || m_->empty(); }
private:
    const Mat *m_;
};
typedef const _InputArray &InputArray;

class _OutputArray {
public:
    _OutputArray(Mat &m) : m_(&m) {}
    void create(int r, int c, int type) const { m_->create(r, c, type); }
    void create(Size sz, int type) const { m_->create(sz, type); }
    Mat getMat() const { return *m_; }
    void release() const { m_->release(); }
private:
    Mat *m_;
};
typedef const _OutputArray &OutputArray;

void FAST(InputArray image, std::vector<KeyPoint> &keypoints, int threshold, bool nonmaxSuppression = true);
void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR);
void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType,
                    const Scalar &value = Scalar());
void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0,
                  int borderType = BORDER_DEFAULT);

/* yml persistence is not provided: nothing is ever open, every node is empty */
class FileNode {
public:
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const std::string &, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](const char *) const { return FileNode(); }
};
template <typename T> inline FileStorage &operator<<(FileStorage &fs, const T &) { return fs; }

class KeyPointsFilter {
public:
    static void retainBest(std::vector<KeyPoint> &, int)
    {
        std::fprintf(stderr, "cv_shim: KeyPointsFilter::retainBest is not provided\n");
        std::abort();
    }
};

} // namespace cv

#ifdef CV_SHIM_LINALG
#include "cv_linalg.hpp"
#endif

#endif
