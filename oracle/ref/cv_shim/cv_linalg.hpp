/*
 * cv_linalg.hpp -- the linear-algebra slice of the OpenCV API that the reference's src/Sim3Solver.cc, src/PnPsolver.cc and
 * src/Initializer.cc use, written from the public API documentation and textbook algorithms alone.  Included at the end of
 * cv_shim.hpp when CV_SHIM_LINALG is defined (oracle/ref/solver_standin.h defines it); without the macro the shim is the text
 * the extractor, stereo, DBoW2 and key-frame database pins have always compiled.
 *
 * TEST INFRASTRUCTURE ONLY: linked into oracle/_ref/ref_sim3, ref_pnp, ref_init, never into the library.  It is a second
 * opinion on the library's own decompositions (csrc/orbp_*_body.h, orbm_svd4_body.h), so it shares no text with them.
 *
 * Scope -- anything else aborts with a message:
 *   - Mat: CV_32F and CV_64F; Mat(r, c, type, Scalar), Mat(MatZeros), eye, diag, t, inv (3x3), dot, cross, col, reshape(0, rows),
 *     at<T>(i), copyTo into a temporary row / column range of the same size, convertTo(CV_32F) from CV_64F, *= scalar.
 *   - Mat * Mat, Mat + Mat, Mat - Mat, -Mat, scalar * Mat, Mat * scalar, Mat / scalar on CV_32F, evaluated at once.  A result is a
 *     MatExpr (a Mat): assigned to a Mat of the same size and type it is written into that matrix's elements, as OpenCV's MatExpr
 *     assignment does (A.row(0) = ..., Pr.col(i) = ...); assigned to any other Mat it replaces it.
 *   - Mat_<float>(r, c) << a, b, ...; norm (L2), determinant (3x3), reduce(dim 1, CV_REDUCE_SUM), pow(.., 2, ..), eigen (symmetric),
 *     Rodrigues (vector to matrix), SVD::compute and SVDecomp (FULL_UV; any m x n, singular values descending, vt rows matching;
 *     for m < n, which only ComputeF21's 8 x 9 system is, u is left empty: the reference never reads it).
 *   - the C API of PnPsolver.cc on CV_64F: CvMat, cvMat, cvCreateMat, cvReleaseMat, cvSetZero, cvMulTransposed (order 1), cvSVD
 *     (CV_SVD_MODIFY_A, CV_SVD_U_T, CV_SVD_V_T), cvInvert(CV_SVD), cvSolve(CV_SVD), cvmGet, cvmSet.
 *
 * Arithmetic.  What OpenCV leaves to its internals is decided here, in two variants:
 *   variant A (the pin, default)    decompositions and inverses in double; float products (Mat * Mat, dot, determinant, reduce)
 *                                   accumulated in float, left to right
 *   variant B (-DCV_SHIM_ARITH_B)   decompositions and inverses in long double; float products accumulated in double, rounded once;
 *                                 the Jacobi sweeps visit their pairs in the opposite order, and the left vectors of zero singular
 *                                 values are completed from the other end of the unit vectors
 * The spread between the two is the part of the reference's answer that this choice decides.
 *   variant C (-DCV_SHIM_ARITH_CANON)  variant A with the small float algebra of src/ORBmatcher.cc and src/LocalMapping.cc done as DESIGN.md section 2's
 *                                 "Canonical semantics" table reads OpenCV 3.1.0 (each place cites its row).  The matcher pin
 *                                 (oracle/_ref/ref_matcher) compares integer match tables exactly, so it cannot absorb that part in a
 *                                 tolerance; variant A of the same driver (ref_matcher_a) is its sensitivity run.
 */
#ifndef ORBX_CV_LINALG_HPP
#define ORBX_CV_LINALG_HPP

#include <limits>

#define CV_REDUCE_SUM 0
#define CV_SVD 1
#define CV_SVD_MODIFY_A 1
#define CV_SVD_U_T 2
#define CV_SVD_V_T 4

namespace cv {

/* the order in which a Jacobi sweep visits the pairs (p, q), p < q: A row by row from the top, B the same walk from the bottom.  The
   order decides which basis a repeated (or zero) singular value gets, and the signs.  The left vectors of zero singular values are
   a completion of the others to an orthonormal basis (OpenCV fills them from a random generator): A completes with e_0, e_1, ...,
   B with e_(m-1), e_(m-2), ... */
#ifdef CV_SHIM_ARITH_B
typedef double shim_acc_t;
typedef long double shim_dec_t;
#define SHIM_PAIR_P(pp, qq, n) ((n) - 1 - (qq))
#define SHIM_PAIR_Q(pp, qq, n) ((n) - 1 - (pp))
#define SHIM_UNIT(k, m) ((m) - 1 - (k))
#else
typedef float shim_acc_t;
typedef double shim_dec_t;
#define SHIM_PAIR_P(pp, qq, n) (pp)
#define SHIM_PAIR_Q(pp, qq, n) (qq)
#define SHIM_UNIT(k, m) (k)
#endif

inline void shim_die(const char *what)
{
    std::fprintf(stderr, "cv_shim: %s\n", what);
    std::abort();
}

inline void shim_need_f32(const Mat &m, const char *what)
{
    if (m.type() != CV_32F || m.empty()) shim_die(what);
}

class MatExpr : public Mat {
public:
#ifdef CV_SHIM_ARITH_CANON
    MatExpr(const Mat &m) : Mat(m), alpha(0) {}
#else
    MatExpr(const Mat &m) : Mat(m) {}
#endif
#ifdef CV_SHIM_ARITH_CANON
    std::vector<float> raw;                              /* of a product: the float sums t0, row-major, for `A*B + C` (one cv::gemm) */
    Mat scaled;                                          /* of `s * Mat`: the matrix and s, for `s*A - B` (one cv::addWeighted) */
    double alpha;
#endif
};

inline Mat::Mat(int r, int c, int type, const Scalar &s) : Mat()
{
    create(r, c, type);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            if (type == CV_32F) at<float>(y, x) = (float)s.v;
            else if (type == CV_64F) at<double>(y, x) = s.v;
            else ptr(y)[x] = (uchar)s.v;
        }
}

inline Mat &Mat::operator=(const MatExpr &e)
{
    if (data && rows == e.rows && cols == e.cols && type() == e.type()) {
        if (data != e.data) {
            Mat tmp = e.clone();
            for (int y = 0; y < rows; y++) std::memcpy(ptr(y), tmp.ptr(y), (size_t)cols * elemSize());
        }
    } else {
        *this = static_cast<const Mat &>(e);
    }
    return *this;
}

/* A driver may watch the sources of copyTo(range): it is how ref_init.cc reads the motions that ReconstructH / ReconstructF hand to
   the private CheckRT (src/Initializer.cc:822-823), which it cannot wrap without editing the reference.  Null unless a driver sets it. */
inline void (*&shim_copy_to_range_hook())(const Mat &)
{
    static void (*hook)(const Mat &) = 0;
    return hook;
}

inline void Mat::copyTo(Mat &&view) const
{
    if (view.rows != rows || view.cols != cols || view.type() != type()) shim_die("copyTo into a range of another size or type");
    if (shim_copy_to_range_hook()) shim_copy_to_range_hook()(*this);
    Mat &dst = view;
    copyTo(dst);
}

inline Mat Mat::eye(int r, int c, int type)
{
    Mat m(r, c, type, Scalar(0));
    for (int i = 0; i < std::min(r, c); i++) {
        if (type == CV_32F) m.at<float>(i, i) = 1.0f;
        else if (type == CV_64F) m.at<double>(i, i) = 1.0;
        else shim_die("Mat::eye is CV_32F / CV_64F only");
    }
    return m;
}

inline Mat Mat::diag(const Mat &d)
{
    shim_need_f32(d, "Mat::diag needs a CV_32F vector");
    if (d.cols != 1 && d.rows != 1) shim_die("Mat::diag needs a vector");
    int n = (int)d.total();
    Mat m(n, n, CV_32F, Scalar(0));
    for (int i = 0; i < n; i++) m.at<float>(i, i) = d.at<float>(i);
    return m;
}

inline Mat Mat::reshape(int cn, int new_rows) const
{
    if (cn != 0 || new_rows <= 0 || !isContinuous() || total() % (size_t)new_rows) shim_die("reshape(0, rows) of a continuous matrix only");
    Mat m(*this);
    m.rows = new_rows;
    m.cols = (int)(total() / (size_t)new_rows);
    m.step = (size_t)m.cols * elemSize();
    return m;
}

inline Mat &Mat::operator*=(double s)
{
    shim_need_f32(*this, "Mat *= scalar is CV_32F only");
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) at<float>(y, x) = (float)((double)at<float>(y, x) * s);
    return *this;
}

inline MatExpr Mat::t() const
{
    shim_need_f32(*this, "t() is CV_32F only");
    Mat out(cols, rows, CV_32F);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) out.at<float>(x, y) = at<float>(y, x);
    return MatExpr(out);
}

inline double Mat::dot(const Mat &b) const
{
    shim_need_f32(*this, "dot is CV_32F only");
    if (b.type() != CV_32F || b.rows != rows || b.cols != cols) shim_die("dot needs two CV_32F matrices of one size");
#ifdef CV_SHIM_ARITH_CANON
    double s = 0;                                        /* row "`Mat::dot` of float vectors": products and sum in double (dotProd_32f) */
#else
    shim_acc_t s = 0;
#endif
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) s += (decltype(s))at<float>(y, x) * (decltype(s))b.at<float>(y, x);
    return (double)s;
}

inline Mat Mat::cross(const Mat &b) const
{
    shim_need_f32(*this, "cross is CV_32F only");
    if (total() != 3 || b.total() != 3 || b.type() != CV_32F) shim_die("cross needs two CV_32F 3-vectors");
    float a0 = at<float>(0), a1 = at<float>(1), a2 = at<float>(2), b0 = b.at<float>(0), b1 = b.at<float>(1), b2 = b.at<float>(2);
    Mat out(rows, cols, CV_32F);
    out.at<float>(0) = a1 * b2 - a2 * b1;
    out.at<float>(1) = a2 * b0 - a0 * b2;
    out.at<float>(2) = a0 * b1 - a1 * b0;
    return out;
}

/* ---- element-wise expressions and the matrix product: CV_32F, evaluated at once ---- */

inline void shim_same_f32(const Mat &a, const Mat &b, const char *what)
{
    if (a.type() != CV_32F || b.type() != CV_32F || a.rows != b.rows || a.cols != b.cols || a.empty()) shim_die(what);
}

inline MatExpr operator*(double s, const Mat &m)
{
    shim_need_f32(m, "scalar * Mat is CV_32F only");
    Mat out(m.rows, m.cols, CV_32F);
    for (int y = 0; y < m.rows; y++)
#ifdef CV_SHIM_ARITH_CANON
        /* row "`Mat / s`, `s * Mat`": alpha in double, materialised by convertTo, whose 32f kernel computes x * (float)alpha + 0.0f in float */
        for (int x = 0; x < m.cols; x++) out.at<float>(y, x) = m.at<float>(y, x) * (float)s + 0.0f;
#else
        for (int x = 0; x < m.cols; x++) out.at<float>(y, x) = (float)(s * (double)m.at<float>(y, x));
#endif
#ifdef CV_SHIM_ARITH_CANON
    MatExpr e(out);
    e.scaled = m;
    e.alpha = s;
    return e;
#else
    return MatExpr(out);
#endif
}
inline MatExpr operator*(const Mat &m, double s) { return s * m; }
inline MatExpr operator/(const Mat &m, double s) { return (1.0 / s) * m; }       /* OpenCV scales by the reciprocal */

inline MatExpr operator-(const Mat &a, const Mat &b)
{
    shim_same_f32(a, b, "Mat - Mat needs two CV_32F matrices of one size");
    Mat out(a.rows, a.cols, CV_32F);
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) out.at<float>(y, x) = a.at<float>(y, x) - b.at<float>(y, x);
    return MatExpr(out);
}

#ifdef CV_SHIM_ARITH_CANON
/* row "`alpha*row - row`": `s*A - B` is one MatOp_AddEx with alpha = s and beta = -1, cv::addWeighted(A, s, B, -1, 0), whose 32f kernel
   computes (float)(a*alpha + b*beta + gamma) in double; alpha == 1 is cv::subtract in float (MatOp_AddEx::assign) */
inline MatExpr operator-(const MatExpr &e, const Mat &b)
{
    if (e.scaled.empty()) return static_cast<const Mat &>(e) - b;
    shim_same_f32(e.scaled, b, "s * Mat - Mat needs two CV_32F matrices of one size");
    if (e.alpha == 1.0) return e.scaled - b;
    Mat out(b.rows, b.cols, CV_32F);
    for (int y = 0; y < b.rows; y++)
        for (int x = 0; x < b.cols; x++)
            out.at<float>(y, x) = (float)(((double)e.scaled.at<float>(y, x) * e.alpha + (double)b.at<float>(y, x) * -1.0) + 0.0);
    return MatExpr(out);
}
#endif

inline MatExpr operator+(const Mat &a, const Mat &b)
{
    shim_same_f32(a, b, "Mat + Mat needs two CV_32F matrices of one size");
    Mat out(a.rows, a.cols, CV_32F);
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) out.at<float>(y, x) = a.at<float>(y, x) + b.at<float>(y, x);
    return MatExpr(out);
}

inline MatExpr operator-(const Mat &m)
{
    shim_need_f32(m, "-Mat is CV_32F only");
    Mat out(m.rows, m.cols, CV_32F);
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) out.at<float>(y, x) = -m.at<float>(y, x);
    return MatExpr(out);
}

inline MatExpr operator*(const Mat &a, const Mat &b)
{
    if (a.type() != CV_32F || b.type() != CV_32F || a.cols != b.rows || a.empty() || b.empty()) shim_die("Mat * Mat needs CV_32F (m x k)(k x n)");
    Mat out(a.rows, b.cols, CV_32F);
#ifdef CV_SHIM_ARITH_CANON
    std::vector<float> raw;
#endif
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < b.cols; x++) {
#ifdef CV_SHIM_ARITH_CANON
            float s = a.at<float>(y, 0) * b.at<float>(0, x);     /* t0 = a0*b0 + a1*b1 + ..: no leading +0, a sum of -0 stays -0 */
            for (int k = 1; k < a.cols; k++) s += a.at<float>(y, k) * b.at<float>(k, x);
#else
            shim_acc_t s = 0;
            for (int k = 0; k < a.cols; k++) s += (shim_acc_t)a.at<float>(y, k) * (shim_acc_t)b.at<float>(k, x);
#endif
#ifdef CV_SHIM_ARITH_CANON
            /* row "`cv::Mat` products of a 3x3 and a 3x1 float matrix": cv::gemm's small-matrix path, the float sum t0 left to right,
               then (float)(t0*alpha + c*beta) in double; without a C operand c is a static zero and beta 0, so a zero sum comes out
               as +0.  alpha = -1 (`-Rcw.t()*tcw`, `-sR21*t12`) has been applied to the left operand, which negates t0 exactly. */
            raw.push_back(s);
            out.at<float>(y, x) = (float)((double)s * 1.0 + 0.0 * 0.0);
#else
            out.at<float>(y, x) = (float)s;
#endif
        }
#ifdef CV_SHIM_ARITH_CANON
    MatExpr e(out);
    e.raw.swap(raw);
    return e;
#else
    return MatExpr(out);
#endif
}

#ifdef CV_SHIM_ARITH_CANON
/* `A*B + C` is one cv::gemm(A, B, 1, C, 1): (float)(t0*alpha + c*beta) in double on the float sums (same row of the table) */
inline MatExpr operator+(const MatExpr &e, const Mat &c)
{
    if (e.raw.empty()) return static_cast<const Mat &>(e) + c;
    shim_same_f32(e, c, "Mat * Mat + Mat needs CV_32F matrices of one size");
    Mat out(e.rows, e.cols, CV_32F);
    for (int y = 0; y < e.rows; y++)
        for (int x = 0; x < e.cols; x++) out.at<float>(y, x) = (float)((double)e.raw[(size_t)y * e.cols + x] * 1.0 + (double)c.at<float>(y, x) * 1.0);
    return MatExpr(out);
}
#endif

/* Mat_<float>(r, c) << a, b, ...  (row-major, each value converted to float) */
struct MatCommaInit {
    Mat m;
    int idx;
    MatCommaInit &operator,(double v)
    {
        if (idx >= (int)m.total()) shim_die("too many values for Mat_<float>");
        m.at<float>(idx / m.cols, idx % m.cols) = (float)v;
        idx++;
        return *this;
    }
    operator Mat() const
    {
        if (idx != (int)m.total()) shim_die("too few values for Mat_<float>");
        return m;
    }
};

template <typename T> class Mat_ : public Mat {
public:
    Mat_(int r, int c) : Mat(r, c, CV_32F) { static_assert(sizeof(T) == 4, "Mat_<float> only"); }
};

inline MatCommaInit operator<<(const Mat_<float> &m, double v)
{
    MatCommaInit ci = {m, 0};
    ci, v;
    return ci;
}

inline double norm(const Mat &m)
{
    shim_need_f32(m, "norm is the L2 norm of a CV_32F matrix only");
    shim_dec_t s = 0;
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) s += (shim_dec_t)m.at<float>(y, x) * (shim_dec_t)m.at<float>(y, x);
    return (double)std::sqrt(s);
}

inline double determinant(const Mat &m)
{
    shim_need_f32(m, "determinant is CV_32F 3 x 3 only");
    if (m.rows != 3 || m.cols != 3) shim_die("determinant is CV_32F 3 x 3 only");
    shim_acc_t a[3][3];
    for (int y = 0; y < 3; y++)
        for (int x = 0; x < 3; x++) a[y][x] = m.at<float>(y, x);
    return (double)(a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                    a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]));
}

/* the inverse by cofactors; a zero determinant gives the zero matrix, as OpenCV's inv() does */
inline MatExpr Mat::inv() const
{
    shim_need_f32(*this, "inv is CV_32F 3 x 3 only");
    if (rows != 3 || cols != 3) shim_die("inv is CV_32F 3 x 3 only");
    shim_dec_t a[3][3], c[3][3];
    for (int y = 0; y < 3; y++)
        for (int x = 0; x < 3; x++) a[y][x] = at<float>(y, x);
    for (int y = 0; y < 3; y++)
        for (int x = 0; x < 3; x++) {
            int y1 = (y + 1) % 3, y2 = (y + 2) % 3, x1 = (x + 1) % 3, x2 = (x + 2) % 3;
            c[y][x] = a[y1][x1] * a[y2][x2] - a[y1][x2] * a[y2][x1];
        }
    shim_dec_t det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
    Mat out(3, 3, CV_32F, Scalar(0));
    if (det != 0) {
        shim_dec_t d = 1 / det;
        for (int y = 0; y < 3; y++)
            for (int x = 0; x < 3; x++) out.at<float>(y, x) = (float)(c[x][y] * d);
    }
    return MatExpr(out);
}

inline void reduce(const Mat &src, Mat &dst, int dim, int rtype)
{
    shim_need_f32(src, "reduce is CV_32F only");
    if (dim != 1 || rtype != CV_REDUCE_SUM) shim_die("reduce is (dim 1, CV_REDUCE_SUM) only");
    dst.create(src.rows, 1, CV_32F);
    for (int y = 0; y < src.rows; y++) {
        shim_acc_t s = 0;
        for (int x = 0; x < src.cols; x++) s += (shim_acc_t)src.at<float>(y, x);
        dst.at<float>(y, 0) = (float)s;
    }
}

inline void pow(const Mat &src, double power, Mat &dst)
{
    shim_need_f32(src, "pow is CV_32F only");
    if (power != 2) shim_die("pow is the square only");
    Mat in = src;                                        /* dst may be src */
    dst.create(in.rows, in.cols, CV_32F);
    for (int y = 0; y < in.rows; y++)
        for (int x = 0; x < in.cols; x++) dst.at<float>(y, x) = in.at<float>(y, x) * in.at<float>(y, x);
}

/* ---- decompositions, in shim_dec_t ---- */

/* Cyclic Jacobi on a symmetric n x n matrix (row-major a, destroyed): eigenvalues in d, eigenvectors as the COLUMNS of v */
template <typename T> void shim_jacobi_eigen(std::vector<T> &a, int n, std::vector<T> &d, std::vector<T> &v)
{
    v.assign((size_t)n * n, 0);
    for (int i = 0; i < n; i++) v[(size_t)i * n + i] = 1;
    const T eps = std::numeric_limits<T>::epsilon();
    for (int sweep = 0; sweep < 100; sweep++) {
        T off = 0, diag = 0;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) (i == j ? diag : off) += a[(size_t)i * n + j] * a[(size_t)i * n + j];
        if (off <= eps * eps * diag) break;
        for (int pp = 0; pp < n - 1; pp++)
            for (int qq = pp + 1; qq < n; qq++) {
                const int p = SHIM_PAIR_P(pp, qq, n), q = SHIM_PAIR_Q(pp, qq, n);
                T apq = a[(size_t)p * n + q];
                if (apq == 0) continue;
                T theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2 * apq);
                T t = (theta >= 0 ? 1 : -1) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
                T c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < n; k++) {            /* columns p, q */
                    T akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - s * akq;
                    a[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {            /* rows p, q */
                    T apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - s * aqk;
                    a[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    T vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - s * vkq;
                    v[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    d.resize(n);
    for (int i = 0; i < n; i++) d[i] = a[(size_t)i * n + i];
}

/*
 * One-sided Jacobi (Hestenes) SVD of the m x n row-major matrix a: a = U diag(w) Vt with w descending.  w has n entries, vt is
 * n x n; u (m x m, its columns beyond the rank completed by Gram-Schmidt) is computed only when want_u and m >= n.  For m < n the
 * matrix is padded with zero rows to n x n, which leaves w and vt as they are.
 */
template <typename T> void shim_svd(const std::vector<T> &a_in, int m_in, int n, std::vector<T> &w, std::vector<T> &u, std::vector<T> &vt, bool want_u)
{
    int m = std::max(m_in, n);
    std::vector<T> a((size_t)m * n, 0), v((size_t)n * n, 0);
    std::copy(a_in.begin(), a_in.end(), a.begin());
    for (int i = 0; i < n; i++) v[(size_t)i * n + i] = 1;
    const T eps = std::numeric_limits<T>::epsilon();
    for (int sweep = 0; sweep < 100; sweep++) {
        bool rotated = false;
        for (int pp = 0; pp < n - 1; pp++)
            for (int qq = pp + 1; qq < n; qq++) {
                const int p = SHIM_PAIR_P(pp, qq, n), q = SHIM_PAIR_Q(pp, qq, n);
                T alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < m; k++) {
                    T x = a[(size_t)k * n + p], y = a[(size_t)k * n + q];
                    alpha += x * x;
                    beta += y * y;
                    gamma += x * y;
                }
                if (gamma == 0 || std::fabs(gamma) <= eps * std::sqrt(alpha * beta)) continue;
                rotated = true;
                T zeta = (beta - alpha) / (2 * gamma);
                T t = (zeta >= 0 ? 1 : -1) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1));
                T c = 1 / std::sqrt(t * t + 1), s = c * t;
                for (int k = 0; k < m; k++) {
                    T x = a[(size_t)k * n + p], y = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * x - s * y;
                    a[(size_t)k * n + q] = s * x + c * y;
                }
                for (int k = 0; k < n; k++) {
                    T x = v[(size_t)k * n + p], y = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * x - s * y;
                    v[(size_t)k * n + q] = s * x + c * y;
                }
            }
        if (!rotated) break;
    }
    std::vector<T> sv(n);
    std::vector<int> order(n);
    for (int j = 0; j < n; j++) {
        T s = 0;
        for (int k = 0; k < m; k++) s += a[(size_t)k * n + j] * a[(size_t)k * n + j];
        sv[j] = std::sqrt(s);
        order[j] = j;
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return sv[x] > sv[y]; });
    w.resize(n);
    vt.assign((size_t)n * n, 0);
    for (int j = 0; j < n; j++) {
        w[j] = sv[order[j]];
        for (int k = 0; k < n; k++) vt[(size_t)j * n + k] = v[(size_t)k * n + order[j]];
    }
    u.clear();
    if (!want_u || m_in < n) return;
    u.assign((size_t)m * m, 0);
    const T tiny = w[0] * eps * (T)std::max(m, n);
    int filled = 0, next_unit = 0;
    for (int j = 0; j < m; j++) {
        std::vector<T> col(m, 0);
        bool from_a = j < n && w[j] > tiny;
        for (;;) {
            if (from_a) {
                for (int k = 0; k < m; k++) col[k] = a[(size_t)k * n + order[j]] / w[j];
            } else {
                if (next_unit >= m) shim_die("SVD: could not complete u");
                std::fill(col.begin(), col.end(), (T)0);
                col[SHIM_UNIT(next_unit, m)] = 1;            /* the completion starts from e_0 in variant A, from e_(m-1) in B */
                next_unit++;
            }
            for (int pass = 0; pass < 2; pass++)             /* orthogonalise against the columns already there, twice */
                for (int i = 0; i < filled; i++) {
                    T d = 0;
                    for (int k = 0; k < m; k++) d += col[k] * u[(size_t)k * m + i];
                    for (int k = 0; k < m; k++) col[k] -= d * u[(size_t)k * m + i];
                }
            T nrm = 0;
            for (int k = 0; k < m; k++) nrm += col[k] * col[k];
            nrm = std::sqrt(nrm);
            if (from_a || nrm > (T)0.5 / (T)std::sqrt((double)m)) {          /* a unit vector not (nearly) in the span so far */
                for (int k = 0; k < m; k++) u[(size_t)k * m + filled] = col[k] / nrm;
                filled++;
                break;
            }
        }
    }
}

inline std::vector<shim_dec_t> shim_load(const Mat &m)
{
    std::vector<shim_dec_t> a((size_t)m.rows * m.cols);
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) a[(size_t)y * m.cols + x] = m.type() == CV_32F ? (shim_dec_t)m.at<float>(y, x) : (shim_dec_t)m.at<double>(y, x);
    return a;
}

inline void shim_store(Mat &dst, int r, int c, int type, const std::vector<shim_dec_t> &a)
{
    dst.create(r, c, type);
    for (int y = 0; y < r; y++)
        for (int x = 0; x < c; x++) {
            if (type == CV_32F) dst.at<float>(y, x) = (float)a[(size_t)y * c + x];
            else dst.at<double>(y, x) = (double)a[(size_t)y * c + x];
        }
}

class SVD {
public:
    enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };
    static void compute(const Mat &src, Mat &w, Mat &u, Mat &vt, int flags = 0)
    {
        shim_need_f32(src, "SVD is CV_32F only");
        if (flags & NO_UV) shim_die("SVD::NO_UV is not provided");
        int m = src.rows, n = src.cols;
        if (m != n && !(flags & FULL_UV)) shim_die("SVD of a non-square matrix needs FULL_UV");
        std::vector<shim_dec_t> a = shim_load(src), sw, su, svt;
        shim_svd<shim_dec_t>(a, m, n, sw, su, svt, true);
        sw.resize(std::min(m, n));
        shim_store(w, (int)sw.size(), 1, CV_32F, sw);
        shim_store(vt, n, n, CV_32F, svt);
        if (m >= n) shim_store(u, m, m, CV_32F, su);
        else u.release();
    }
};

inline void SVDecomp(const Mat &src, Mat &w, Mat &u, Mat &vt, int flags = 0) { SVD::compute(src, w, u, vt, flags); }

/* a symmetric CV_32F matrix: eigenvalues descending (n x 1), eigenvectors as the rows of the n x n matrix */
inline bool eigen(const Mat &src, Mat &eval, Mat &evec)
{
    shim_need_f32(src, "eigen is CV_32F only");
    if (src.rows != src.cols) shim_die("eigen needs a square matrix");
    int n = src.rows;
    std::vector<shim_dec_t> a = shim_load(src), d, v;
    shim_jacobi_eigen<shim_dec_t>(a, n, d, v);
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[x] > d[y]; });
    std::vector<shim_dec_t> sd(n), sv((size_t)n * n);
    for (int j = 0; j < n; j++) {
        sd[j] = d[order[j]];
        for (int k = 0; k < n; k++) sv[(size_t)j * n + k] = v[(size_t)k * n + order[j]];
    }
    shim_store(eval, n, 1, CV_32F, sd);
    shim_store(evec, n, n, CV_32F, sv);
    return true;
}

/* rotation vector (1 x 3 or 3 x 1, CV_32F) to rotation matrix: R = cos I + (1 - cos) r r^T + sin [r]x */
inline void Rodrigues(const Mat &src, Mat &dst)
{
    shim_need_f32(src, "Rodrigues is CV_32F only");
    if (src.total() != 3 || (src.rows != 1 && src.cols != 1)) shim_die("Rodrigues is vector to matrix only");
    shim_dec_t r[3] = {src.at<float>(0), src.at<float>(1), src.at<float>(2)};
    shim_dec_t theta = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    std::vector<shim_dec_t> R(9, 0);
    R[0] = R[4] = R[8] = 1;
    if (theta >= std::numeric_limits<double>::epsilon()) {
        shim_dec_t c = std::cos(theta), s = std::sin(theta), c1 = 1 - c, x = r[0] / theta, y = r[1] / theta, z = r[2] / theta;
        shim_dec_t rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
        shim_dec_t rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
        for (int k = 0; k < 9; k++) R[k] = c * (k % 4 == 0 ? 1 : 0) + c1 * rrt[k] + s * rx[k];
    }
    shim_store(dst, 3, 3, CV_32F, R);
}

} // namespace cv

/* ---- the C API of src/PnPsolver.cc: CV_64F, row-major, contiguous ---- */

struct CvMat {
    int type;
    int step;
    union {
        uchar *ptr;
        float *fl;
        double *db;
    } data;
    int rows, cols;
    int owned;
};

inline void cv_c_need(const CvMat *m, const char *what)
{
    if (!m || m->type != CV_64F || !m->data.db || m->step != m->cols * (int)sizeof(double)) cv::shim_die(what);
}

inline CvMat cvMat(int rows, int cols, int type, void *data = 0)
{
    if (type != CV_64F) cv::shim_die("cvMat is CV_64F only");
    CvMat m;
    m.type = type;
    m.step = cols * (int)sizeof(double);
    m.data.db = (double *)data;
    m.rows = rows;
    m.cols = cols;
    m.owned = 0;
    return m;
}

inline CvMat *cvCreateMat(int rows, int cols, int type)
{
    if (rows <= 0 || cols <= 0) cv::shim_die("cvCreateMat needs positive sizes");
    CvMat *m = new CvMat(cvMat(rows, cols, type, new double[(size_t)rows * cols]()));
    m->owned = 1;
    return m;
}

inline void cvReleaseMat(CvMat **m)
{
    if (!m || !*m) return;
    if ((*m)->owned) delete[] (*m)->data.db;
    delete *m;
    *m = 0;
}

inline void cvSetZero(CvMat *m)
{
    cv_c_need(m, "cvSetZero is CV_64F only");
    std::fill(m->data.db, m->data.db + (size_t)m->rows * m->cols, 0.0);
}

inline double cvmGet(const CvMat *m, int row, int col)
{
    cv_c_need(m, "cvmGet is CV_64F only");
    if (row < 0 || row >= m->rows || col < 0 || col >= m->cols) cv::shim_die("cvmGet outside the matrix");
    return m->data.db[(size_t)row * m->cols + col];
}

inline void cvmSet(CvMat *m, int row, int col, double value)
{
    cv_c_need(m, "cvmSet is CV_64F only");
    if (row < 0 || row >= m->rows || col < 0 || col >= m->cols) cv::shim_die("cvmSet outside the matrix");
    m->data.db[(size_t)row * m->cols + col] = value;
}

/* order 1: dst = src^T src */
inline void cvMulTransposed(const CvMat *src, CvMat *dst, int order)
{
    cv_c_need(src, "cvMulTransposed is CV_64F only");
    cv_c_need(dst, "cvMulTransposed is CV_64F only");
    if (order != 1 || dst->rows != src->cols || dst->cols != src->cols) cv::shim_die("cvMulTransposed is (order 1, n x n result) only");
    int n = src->cols;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            cv::shim_dec_t s = 0;
            for (int k = 0; k < src->rows; k++) s += (cv::shim_dec_t)src->data.db[(size_t)k * n + i] * (cv::shim_dec_t)src->data.db[(size_t)k * n + j];
            dst->data.db[(size_t)i * n + j] = (double)s;
        }
}

inline void cv_c_svd(const CvMat *A, std::vector<cv::shim_dec_t> &w, std::vector<cv::shim_dec_t> &u, std::vector<cv::shim_dec_t> &vt)
{
    cv_c_need(A, "cvSVD is CV_64F only");
    if (A->rows < A->cols) cv::shim_die("cvSVD needs rows >= cols");
    std::vector<cv::shim_dec_t> a((size_t)A->rows * A->cols);
    for (size_t k = 0; k < a.size(); k++) a[k] = A->data.db[k];
    cv::shim_svd<cv::shim_dec_t>(a, A->rows, A->cols, w, u, vt, true);
}

/* A = U diag(W) V^T; W an n x 1 (or 1 x n) vector; CV_SVD_U_T / CV_SVD_V_T hand back the transposed factor */
inline void cvSVD(CvMat *A, CvMat *W, CvMat *U = 0, CvMat *V = 0, int flags = 0)
{
    std::vector<cv::shim_dec_t> w, u, vt;
    cv_c_svd(A, w, u, vt);
    int m = A->rows, n = A->cols;
    cv_c_need(W, "cvSVD: W is CV_64F only");
    if (W->rows * W->cols != n) cv::shim_die("cvSVD: W must be a vector of n singular values");
    for (int k = 0; k < n; k++) W->data.db[k] = (double)w[k];
    if (U) {
        cv_c_need(U, "cvSVD: U is CV_64F only");
        if (U->rows != m || U->cols != m) cv::shim_die("cvSVD: U must be m x m");
        for (int y = 0; y < m; y++)
            for (int x = 0; x < m; x++) U->data.db[(size_t)y * m + x] = (double)((flags & CV_SVD_U_T) ? u[(size_t)x * m + y] : u[(size_t)y * m + x]);
    }
    if (V) {
        cv_c_need(V, "cvSVD: V is CV_64F only");
        if (V->rows != n || V->cols != n) cv::shim_die("cvSVD: V must be n x n");
        for (int y = 0; y < n; y++)
            for (int x = 0; x < n; x++) V->data.db[(size_t)y * n + x] = (double)((flags & CV_SVD_V_T) ? vt[(size_t)y * n + x] : vt[(size_t)x * n + y]);
    }
}

/* x = V diag(1 / w) U^T b over the singular values above 2 eps sum(w), the rule of OpenCV's documented SVD back substitution */
inline void cv_c_backsub(const CvMat *A, const double *b, int nb, double *x)
{
    std::vector<cv::shim_dec_t> w, u, vt;
    cv_c_svd(A, w, u, vt);
    int m = A->rows, n = A->cols;
    cv::shim_dec_t threshold = 0;
    for (int k = 0; k < n; k++) threshold += w[k];
    threshold *= 2 * (cv::shim_dec_t)std::numeric_limits<double>::epsilon();
    for (int c = 0; c < nb; c++) {
        std::vector<cv::shim_dec_t> acc(n, 0);
        for (int k = 0; k < n; k++) {
            if (w[k] <= threshold) continue;
            cv::shim_dec_t s = 0;
            for (int i = 0; i < m; i++) s += u[(size_t)i * m + k] * (cv::shim_dec_t)b[(size_t)i * nb + c];
            s /= w[k];
            for (int j = 0; j < n; j++) acc[j] += s * vt[(size_t)k * n + j];
        }
        for (int j = 0; j < n; j++) x[(size_t)j * nb + c] = (double)acc[j];
    }
}

inline double cvInvert(const CvMat *src, CvMat *dst, int method)
{
    cv_c_need(src, "cvInvert is CV_64F only");
    cv_c_need(dst, "cvInvert is CV_64F only");
    if (method != CV_SVD || src->rows != src->cols || dst->rows != src->rows || dst->cols != src->cols) cv::shim_die("cvInvert is (square, CV_SVD) only");
    int n = src->rows;
    std::vector<double> eye((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) eye[(size_t)i * n + i] = 1.0;
    cv_c_backsub(src, eye.data(), n, dst->data.db);
    return 1.0;                                          /* the reference ignores the returned condition figure */
}

inline int cvSolve(const CvMat *A, const CvMat *b, CvMat *x, int method)
{
    cv_c_need(A, "cvSolve is CV_64F only");
    cv_c_need(b, "cvSolve is CV_64F only");
    cv_c_need(x, "cvSolve is CV_64F only");
    if (method != CV_SVD || b->rows != A->rows || x->rows != A->cols || x->cols != b->cols) cv::shim_die("cvSolve is (CV_SVD, matching sizes) only");
    cv_c_backsub(A, b->data.db, b->cols, x->data.db);
    return 1;
}

#endif
