// Functional stand-in for the parts of OpenCV (core, calib3d, imgproc, highgui, aruco) that the
// reference program's src/*.{h,cpp,hpp} name.  TEST INFRASTRUCTURE ONLY: it exists so that the
// reference's own loops can be compiled into oracle/_ref/arvx_ref and run on a CPU, without
// OpenCV, without a GPU and without libarvx.
//
// Written from OpenCV's public documentation (docs.opencv.org/4.x); each operation cites the
// documented behaviour it stands for.  What the documentation does not fix -- the ARITHMETIC of
// cv::gemm, cv::norm, cv::Rodrigues, Mat::inv and cv::undistort -- is this project's statement
// of it (oracle/arvx_oracle.c, G1 / G2 / N1) and stays UNPINNED: both sides of a comparison use
// the same statement.  Everything the reference's authors wrote is what the binary pins.
#ifndef ARVX_REF_STANDIN_CV_HPP
#define ARVX_REF_STANDIN_CV_HPP

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

typedef unsigned char uchar;

// core/hal/interface.h: depth codes and CV_MAKETYPE(depth, cn) = depth + ((cn - 1) << 3).
#define CV_8U 0
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn)-1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_64FC1 CV_MAKETYPE(CV_64F, 1)

namespace cv {

// cv::Ptr: "a template class for smart pointers with shared ownership" (since 3.0 an alias of
// std::shared_ptr).
template <typename T>
using Ptr = std::shared_ptr<T>;

// ---- small fixed types ------------------------------------------------------------------------

// cv::Vec<_Tp, cn>: "short numerical vectors"; elements through operator[] and operator().
template <typename T, int n>
struct Vec {
    T val[n];
    Vec() {
        for (int i = 0; i < n; ++i) val[i] = T(0);  // "default constructor: all zeros"
    }
    template <typename A, typename B, typename C>
    Vec(const A& a, const B& b, const C& c) {
        static_assert(n == 3, "three elements");
        val[0] = (T)a;
        val[1] = (T)b;
        val[2] = (T)c;
    }
    template <typename A, typename B, typename C, typename D>
    Vec(const A& a, const B& b, const C& c, const D& d) {
        static_assert(n == 4, "four elements");
        val[0] = (T)a;
        val[1] = (T)b;
        val[2] = (T)c;
        val[3] = (T)d;
    }
    T& operator[](int i) { return val[i]; }
    const T& operator[](int i) const { return val[i]; }
    T& operator()(int i) { return val[i]; }
    const T& operator()(int i) const { return val[i]; }
};
// "v1 - v2": element-wise, in the element type.
template <typename T, int n>
Vec<T, n> operator-(const Vec<T, n>& a, const Vec<T, n>& b) {
    Vec<T, n> r;
    for (int i = 0; i < n; ++i) r.val[i] = a.val[i] - b.val[i];
    return r;
}
typedef Vec<uchar, 3> Vec3b;
typedef Vec<int, 3> Vec3i;
typedef Vec<float, 3> Vec3f;
typedef Vec<float, 4> Vec4f;
typedef Vec<double, 3> Vec3d;

// cv::norm(const Matx&): the L2 norm, sqrt of normL2Sqr<float, double>.  UNPINNED arithmetic,
// stated as arvx_oracle_depth states it (N1): one unrolled step of squares summed in double.
inline double norm(const Vec4f& v) {
    const double v0 = v.val[0], v1 = v.val[1], v2 = v.val[2], v3 = v.val[3];
    double acc = 0.0;
    acc += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
    return std::sqrt(acc);
}

template <typename T>
struct Size_ {
    T width, height;
    Size_() : width(0), height(0) {}
    Size_(T w, T h) : width(w), height(h) {}
};
typedef Size_<int> Size;

// cv::Rect_: "the top-left corner and the width and height"; contains(pt): x <= pt.x < x + width
// and y <= pt.y < y + height.
template <typename T>
struct Rect_ {
    T x, y, width, height;
    Rect_() : x(0), y(0), width(0), height(0) {}
    Rect_(T x_, T y_, T w, T h) : x(x_), y(y_), width(w), height(h) {}
};
typedef Rect_<int> Rect;

// cv::Point_: inside(rect) "checks whether the point is inside the specified rectangle".
template <typename T>
struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
    bool inside(const Rect_<T>& r) const {
        return r.x <= x && x < r.x + r.width && r.y <= y && y < r.y + r.height;
    }
};
typedef Point_<int> Point;
typedef Point_<float> Point2f;

// cv::Scalar_: a 4-element vector; missing elements are zero.
struct Scalar {
    double val[4];
    Scalar(double a = 0, double b = 0, double c = 0, double d = 0) {
        val[0] = a;
        val[1] = b;
        val[2] = c;
        val[3] = d;
    }
};

struct TermCriteria {
    enum { COUNT = 1, MAX_ITER = COUNT, EPS = 2 };
    int type, maxCount;
    double epsilon;
    TermCriteria(int t = 0, int c = 0, double e = 0) : type(t), maxCount(c), epsilon(e) {}
};

// ---- the grouping of the M * world row sums (oracle/arvx_oracle.c, G2) -------------------------
// 1 = ((p0+p1)+p2)+p3 (the oracle's default), 0 = p0+((p1+p2)+p3).  A run-time switch, the twin
// of arvx_oracle_set_assoc.
namespace arvx_ref {
inline int& assoc_left() {
    static int v = 1;
    return v;
}
}  // namespace arvx_ref

// ---- Mat ----------------------------------------------------------------------------------------

// cv::Mat: "n-dimensional dense array"; here two dimensions.  Copying a Mat copies the header
// only: "the data is shared".  clone() and copyTo() make deep copies.
class Mat {
public:
    int rows, cols;
    size_t step;  // bytes between rows
    uchar* data;

    Mat() : rows(0), cols(0), step(0), data(nullptr), type_(0) {}
    // Mat(rows, cols, type): allocates; contents unspecified in OpenCV, zero here.
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(Size s, int type) { create(s.height, s.width, type); }

    // Mat::eye: "an identity matrix of the specified size and type".
    static Mat eye(int r, int c, int type) {
        Mat m(r, c, type);
        for (int i = 0; i < r && i < c; ++i) m.setd(i, i, 1.0);
        return m;
    }

    int type() const { return type_; }
    int depth() const { return type_ & 7; }
    int channels() const { return (type_ >> 3) + 1; }
    size_t elemSize() const { return depth_size(depth()) * (size_t)channels(); }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }

    // Mat::at<T>(row, col): "a reference to the specified array element"; no range check in
    // release builds, so at(0, j) of a continuous column reaches element j.
    template <typename T>
    T& at(int r, int c) {
        return *reinterpret_cast<T*>(data + (size_t)r * step + (size_t)c * sizeof(T));
    }
    template <typename T>
    const T& at(int r, int c) const {
        return *reinterpret_cast<const T*>(data + (size_t)r * step + (size_t)c * sizeof(T));
    }
    // Mat::at<T>(Point pt): "element position specified as Point(j, i)" = at(pt.y, pt.x).
    template <typename T>
    T& at(Point p) {
        return at<T>(p.y, p.x);
    }
    template <typename T>
    const T& at(Point p) const {
        return at<T>(p.y, p.x);
    }

    // Mat::clone: "a full copy of the array and the underlying data".
    Mat clone() const {
        Mat m;
        copyTo(m);
        return m;
    }
    // Mat::copyTo: "copies the matrix to another one", reallocating the destination.
    void copyTo(Mat& dst) const {
        Mat m;
        if (data) {
            m.create(rows, cols, type_);
            for (int r = 0; r < rows; ++r)
                std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step,
                            (size_t)cols * elemSize());
        }
        dst = m;
    }
    // Mat::convertTo(m, rtype): "converts an array to another data type", saturate_cast per
    // element; to CV_32F / CV_64F that is a plain C++ conversion.  dst may be *this.
    void convertTo(Mat& dst, int rtype) const {
        Mat m(rows, cols, CV_MAKETYPE(rtype & 7, channels()));
        const int cn = channels();
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols * cn; ++c) m.setd_flat(r, c, getd_flat(r, c));
        dst = m;
    }
    // Mat::operator()(const Rect&): "extracts a rectangular submatrix"; no data is copied.
    Mat operator()(const Rect& roi) const {
        Mat m(*this);
        m.rows = roi.height;
        m.cols = roi.width;
        m.data = data + (size_t)roi.y * step + (size_t)roi.x * elemSize();
        return m;
    }
    // Mat::t: "transposes a matrix".
    Mat t() const {
        Mat m(cols, rows, type_);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) m.setd(c, r, getd(r, c));
        return m;
    }
    // Mat::inv (DECOMP_LU): "inverses a matrix".  UNPINNED arithmetic: Gauss-Jordan with partial
    // pivoting in double, rounded to the matrix's type.  The tests take the pose this yields as
    // their input, so it cancels out of every comparison.
    Mat inv() const {
        const int n = rows;
        std::vector<double> a((size_t)n * 2 * n, 0.0);
        for (int r = 0; r < n; ++r) {
            for (int c = 0; c < n; ++c) a[(size_t)r * 2 * n + c] = getd(r, c);
            a[(size_t)r * 2 * n + n + r] = 1.0;
        }
        for (int k = 0; k < n; ++k) {
            int p = k;
            for (int r = k + 1; r < n; ++r)
                if (std::fabs(a[(size_t)r * 2 * n + k]) > std::fabs(a[(size_t)p * 2 * n + k])) p = r;
            if (a[(size_t)p * 2 * n + k] == 0.0) return Mat(n, n, type_);  // "singular: zeros"
            if (p != k)
                for (int c = 0; c < 2 * n; ++c) std::swap(a[(size_t)k * 2 * n + c], a[(size_t)p * 2 * n + c]);
            const double d = a[(size_t)k * 2 * n + k];
            for (int c = 0; c < 2 * n; ++c) a[(size_t)k * 2 * n + c] /= d;
            for (int r = 0; r < n; ++r) {
                if (r == k) continue;
                const double f = a[(size_t)r * 2 * n + k];
                if (f == 0.0) continue;
                for (int c = 0; c < 2 * n; ++c) a[(size_t)r * 2 * n + c] -= f * a[(size_t)k * 2 * n + c];
            }
        }
        Mat m(n, n, type_);
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) m.setd(r, c, a[(size_t)r * 2 * n + n + c]);
        return m;
    }

    // element access by depth, as double (single-channel helpers of this stand-in)
    double getd(int r, int c) const { return getd_flat(r, c); }
    void setd(int r, int c, double v) { setd_flat(r, c, v); }

private:
    int type_;
    std::shared_ptr<std::vector<uchar>> store_;

    static size_t depth_size(int depth) {
        switch (depth) {
            case CV_8U: return 1;
            case CV_32S: return 4;
            case CV_32F: return 4;
            case CV_64F: return 8;
        }
        std::fprintf(stderr, "arvx_ref stand-in: Mat depth %d is not provided\n", depth);
        std::exit(2);
    }
    void create(int r, int c, int type) {
        rows = r;
        cols = c;
        type_ = type;
        step = (size_t)c * elemSize();
        store_ = std::make_shared<std::vector<uchar>>((size_t)r * step + 1, (uchar)0);
        data = store_->data();
    }
    double getd_flat(int r, int c) const {
        const uchar* p = data + (size_t)r * step;
        switch (depth()) {
            case CV_8U: return p[c];
            case CV_32S: return reinterpret_cast<const int*>(p)[c];
            case CV_32F: return reinterpret_cast<const float*>(p)[c];
            default: return reinterpret_cast<const double*>(p)[c];
        }
    }
    void setd_flat(int r, int c, double v) {
        uchar* p = data + (size_t)r * step;
        switch (depth()) {
            case CV_8U: p[c] = (uchar)(v < 0 ? 0 : v > 255 ? 255 : std::nearbyint(v)); break;
            case CV_32S: reinterpret_cast<int*>(p)[c] = (int)std::nearbyint(v); break;
            case CV_32F: reinterpret_cast<float*>(p)[c] = (float)v; break;
            default: reinterpret_cast<double*>(p)[c] = v; break;
        }
    }
};

// cv::Mat_<float>: a typed view of a CV_32F Mat; operator()(i) is element i of a single row or
// single column.
struct Mat1f : public Mat {
    Mat1f() {}
    Mat1f(const Mat& m) : Mat(m) {
        if (!m.empty() && m.type() != CV_32FC1) m.convertTo(*this, CV_32F);
    }
    float& operator()(int i) { return cols == 1 ? at<float>(i, 0) : at<float>(0, i); }
    const float& operator()(int i) const { return cols == 1 ? at<float>(i, 0) : at<float>(0, i); }
};

// Matrix product A * B ("operator *" on Mat is cv::gemm(A, B, 1, noArray(), 0)).  UNPINNED
// arithmetic, stated exactly as oracle/arvx_oracle.c states it:
//   (G1) CV_32F, 2 <= len <= 4 and len == rows of the result (intr * pose): every output is
//        t = a0*b0 + a1*b1 + ... in float, left to right, then (float)((double)t * 1.0 + 0.0).
//   (G2) other CV_32F shapes (M * world, len 4): exact double products of the float inputs,
//        summed in double in the grouping of arvx_ref::assoc_left(), times alpha = 1.0,
//        rounded to float once.
//   CV_64F: products and sums in double, left to right.
inline Mat operator*(const Mat& A, const Mat& B) {
    const int len = A.cols;
    if (A.type() != B.type() || B.rows != len || (A.type() != CV_32FC1 && A.type() != CV_64FC1)) {
        std::fprintf(stderr, "arvx_ref stand-in: Mat * Mat of these types / shapes is not provided\n");
        std::exit(2);
    }
    Mat D(A.rows, B.cols, A.type());
    for (int r = 0; r < A.rows; ++r)
        for (int c = 0; c < B.cols; ++c) {
            if (A.type() == CV_64FC1) {
                double s = 0.0;
                for (int k = 0; k < len; ++k) s = s + A.at<double>(r, k) * B.at<double>(k, c);
                D.at<double>(r, c) = s;
            } else if (len >= 2 && len <= 4 && len == A.rows) { /* G1 */
                float t = A.at<float>(r, 0) * B.at<float>(0, c);
                for (int k = 1; k < len; ++k) t = t + A.at<float>(r, k) * B.at<float>(k, c);
                D.at<float>(r, c) = (float)((double)t * 1.0 + 0.0 * 0.0);
            } else if (len == 4) { /* G2 */
                const double p0 = (double)A.at<float>(r, 0) * (double)B.at<float>(0, c);
                const double p1 = (double)A.at<float>(r, 1) * (double)B.at<float>(1, c);
                const double p2 = (double)A.at<float>(r, 2) * (double)B.at<float>(2, c);
                const double p3 = (double)A.at<float>(r, 3) * (double)B.at<float>(3, c);
                double s0 = arvx_ref::assoc_left() ? ((p0 + p1) + p2) + p3 : p0 + ((p1 + p2) + p3);
                s0 = s0 * 1.0;
                D.at<float>(r, c) = (float)s0;
            } else {
                double s = 0.0;
                for (int k = 0; k < len; ++k)
                    s = s + (double)A.at<float>(r, k) * (double)B.at<float>(k, c);
                D.at<float>(r, c) = (float)(s * 1.0);
            }
        }
    return D;
}

template <typename T>
struct DepthOf;
template <>
struct DepthOf<float> {
    enum { value = CV_32F };
};
template <>
struct DepthOf<double> {
    enum { value = CV_64F };
};

// Mat * Vec: the Vec is taken as an n x 1 matrix of its element type ("Mat(const Vec&)"), so an
// expression A * B * v is evaluated left to right as (A * B) * v.
template <typename T, int n>
Mat operator*(const Mat& A, const Vec<T, n>& v) {
    Mat B(n, 1, DepthOf<T>::value);
    for (int i = 0; i < n; ++i) B.at<T>(i, 0) = v.val[i];
    return A * B;
}

// Unary minus: "-A" scales every element by -1 (exact).
inline Mat operator-(const Mat& A) {
    Mat D = A.clone();
    for (int r = 0; r < D.rows; ++r)
        for (int c = 0; c < D.cols * D.channels(); ++c) D.setd(r, c, -A.getd(r, c));
    return D;
}

// "~A": bitwise inversion of every element (8-bit arrays here).
inline Mat operator~(const Mat& A) {
    Mat D = A.clone();
    for (int r = 0; r < D.rows; ++r)
        for (size_t b = 0; b < (size_t)D.cols * D.elemSize(); ++b)
            D.data[(size_t)r * D.step + b] = (uchar)~D.data[(size_t)r * D.step + b];
    return D;
}

// ---- calib3d --------------------------------------------------------------------------------------

// cv::Rodrigues(rvec -> 3x3, CV_64F for a double input): theta = norm(r), r = r / theta,
// R = cos(theta) I + (1 - cos(theta)) r r^T + sin(theta) [r]x.  UNPINNED arithmetic (double);
// it cancels out of the tests with Mat::inv.
inline void Rodrigues(const Vec3d& rvec, Mat& R) {
    R = Mat::eye(3, 3, CV_64F);
    const double theta = std::sqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1] + rvec[2] * rvec[2]);
    if (theta < 2.2204460492503131e-16) return;  // "R = I" for a zero rotation
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1.0 - c;
    const double x = rvec[0] / theta, y = rvec[1] / theta, z = rvec[2] / theta;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R.at<double>(i, j) = c * (i == j ? 1.0 : 0.0) + c1 * rrt[3 * i + j] + s * rx[3 * i + j];
}

// cv::undistort: "transforms an image to compensate for lens distortion".  With every
// coefficient zero (or none given) the map is the identity and the output is an exact copy; the
// remap itself is not provided here -- the project's own statement of it is GPU code.
inline void undistort(const Mat& src, Mat& dst, const Mat& cameraMatrix, const Mat& distCoeffs) {
    (void)cameraMatrix;
    for (int r = 0; r < distCoeffs.rows; ++r)
        for (int c = 0; c < distCoeffs.cols * distCoeffs.channels(); ++c)
            if (distCoeffs.getd(r, c) != 0.0) {
                std::fprintf(stderr,
                             "arvx_ref stand-in: cv::undistort with non-zero distortion "
                             "coefficients is not provided\n");
                std::exit(2);
            }
    src.copyTo(dst);
}

enum {
    CALIB_USE_INTRINSIC_GUESS = 0x00001,
    CALIB_FIX_ASPECT_RATIO = 0x00002,
    CALIB_FIX_PRINCIPAL_POINT = 0x00004,
    CALIB_ZERO_TANGENT_DIST = 0x00008
};

template <typename V>
inline void drawFrameAxes(Mat&, const Mat&, const Mat&, const V&, const V&, float, int = 3) {}

// ---- imgproc / highgui / persistence: named by the reference's headers, never run here ------------

enum { COLOR_BGR2RGB = 4, COLOR_BGR2HSV = 40 };
enum { KMEANS_RANDOM_CENTERS = 0, KMEANS_PP_CENTERS = 2 };
inline void cvtColor(const Mat&, Mat&, int) {}
inline void inRange(const Mat&, const Scalar&, const Scalar&, Mat&) {}
inline double kmeans(const Mat&, int, Mat&, TermCriteria, int, int, Mat&) { return 0.0; }
inline void imshow(const std::string&, const Mat&) {}
inline int waitKey(int = 0) { return -1; }

class FileNode {
public:
    void operator>>(Mat&) const {}
};
class FileStorage {
public:
    enum Mode { READ = 0, WRITE = 1 };
    FileStorage(const std::string&, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const char*) const { return FileNode(); }
};
template <typename T>
inline FileStorage& operator<<(FileStorage& fs, const T&) {
    return fs;
}

// ---- aruco -------------------------------------------------------------------------------------------
// Marker detection is replaced by a registry: the driver registers the rvec / tvec of an image
// under the address of its pixel data (shallow copies of a Mat share it; the bytes are never
// touched).  detectMarkers looks the image up and reports one marker, interpolateCornersCharuco
// one corner, estimatePoseCharucoBoard "valid" with the registered pose; the drawing calls do
// nothing.
namespace arvx_ref {
struct Pose {
    Vec3d rvec, tvec;
};
inline std::map<const uchar*, Pose>& poses() {
    static std::map<const uchar*, Pose> m;
    return m;
}
inline const Pose*& current() {
    static const Pose* p = nullptr;
    return p;
}
inline void register_pose(const Mat& image, const Vec3d& rvec, const Vec3d& tvec) {
    Pose p;
    p.rvec = rvec;
    p.tvec = tvec;
    poses()[image.data] = p;
}
}  // namespace arvx_ref

namespace aruco {

enum PREDEFINED_DICTIONARY_NAME { DICT_6X6_250 = 10 };
struct Dictionary {};
struct DetectorParameters {
    static Ptr<DetectorParameters> create() { return std::make_shared<DetectorParameters>(); }
};
struct CharucoBoard {
    Ptr<Dictionary> dictionary;
    static Ptr<CharucoBoard> create(int, int, float, float, const Ptr<Dictionary>& d) {
        Ptr<CharucoBoard> b = std::make_shared<CharucoBoard>();
        b->dictionary = d;
        return b;
    }
};
inline Ptr<Dictionary> getPredefinedDictionary(int) { return std::make_shared<Dictionary>(); }

inline void detectMarkers(const Mat& image, const Ptr<Dictionary>&,
                          std::vector<std::vector<Point2f>>& corners, std::vector<int>& ids,
                          const Ptr<DetectorParameters>& = Ptr<DetectorParameters>()) {
    corners.clear();
    ids.clear();
    std::map<const uchar*, arvx_ref::Pose>::const_iterator it = arvx_ref::poses().find(image.data);
    if (it == arvx_ref::poses().end()) {
        arvx_ref::current() = nullptr;
        return;  // no marker: the caller keeps the identity pose
    }
    arvx_ref::current() = &it->second;
    corners.push_back(std::vector<Point2f>(4));
    ids.push_back(0);
}
inline void drawDetectedMarkers(Mat&, const std::vector<std::vector<Point2f>>&,
                                const std::vector<int>&) {}
inline int interpolateCornersCharuco(const std::vector<std::vector<Point2f>>&,
                                     const std::vector<int>& markerIds, const Mat&,
                                     const Ptr<CharucoBoard>&, std::vector<Point2f>& charucoCorners,
                                     std::vector<int>& charucoIds, const Mat&, const Mat&) {
    charucoCorners.clear();
    charucoIds.clear();
    if (!markerIds.empty()) {
        charucoCorners.push_back(Point2f());
        charucoIds.push_back(0);
    }
    return (int)charucoIds.size();
}
inline void drawDetectedCornersCharuco(Mat&, const std::vector<Point2f>&, const std::vector<int>&,
                                       const Scalar&) {}
inline bool estimatePoseCharucoBoard(const std::vector<Point2f>&, const std::vector<int>&,
                                     const Ptr<CharucoBoard>&, const Mat&, const Mat&, Vec3d& rvec,
                                     Vec3d& tvec) {
    if (!arvx_ref::current()) return false;
    rvec = arvx_ref::current()->rvec;
    tvec = arvx_ref::current()->tvec;
    return true;
}

}  // namespace aruco
}  // namespace cv

#endif
