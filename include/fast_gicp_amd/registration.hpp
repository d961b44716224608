// Host-side mirror of the reference's registration classes on top of the C ABI (fast_vgicp_hip.h).
//
//   fast_gicp::LsqRegistration   <- include/fast_gicp/gicp/lsq_registration.hpp + impl/lsq_registration_impl.hpp
//   fast_gicp::FastVGICPCuda     <- include/fast_gicp/gicp/fast_vgicp_cuda.hpp  + impl/fast_vgicp_cuda_impl.hpp
//   fast_gicp::NDTCuda           <- include/fast_gicp/ndt/ndt_cuda.hpp          + impl/ndt_cuda_impl.hpp
// (FastGICP and FastVGICP likewise.) What the four have in common -- the handle, the virtuals of LsqRegistration on top of it, the
// exception text -- is written once, in DeviceRegistration, against a table of C calls per correspondence model (detail::DeviceCalls).
//
// Same class / method / enum names, argument meaning and defaults as the reference, so code written
// against it (gicp_align, gicp_test, pygicp) reads the same. PCL and Eigen are not available in this
// build environment (the reference does not vendor them), so the PCL base class is replaced by the
// few members of pcl::Registration the reference's callers use, on a minimal PointCloud / Matrix4
// type. INTEGRATION.md shows the 1:1 PCL-templated shim for a tree that has PCL.
//
// Two ways to run the optimiser:
//   * setUseDeviceLM(true)  (default): fvh_*_align -- the whole LM loop on the GPU, one D2H.
//   * setUseDeviceLM(false): the reference's host loop (step_lm below) calling the virtuals
//     linearize() / compute_error() -> fvh_*_update_correspondences / fvh_*_compute_error,
//     i.e. exactly the reference's call sequence. Both give the same result to fp64 rounding.
#pragma once
#if defined(__SSE2__)
#include <immintrin.h>
#endif
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fast_vgicp_hip.h"
#include "kdtree.hpp"

namespace fast_gicp {

// gicp_settings.hpp:7-11, ndt_settings.hpp:6, fast_vgicp_cuda.hpp:18 (same ordinals)
enum class RegularizationMethod { NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS };
enum class NeighborSearchMethod { DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS };
enum class VoxelAccumulationMode { ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE };
enum class NDTDistanceMode { P2D, D2D };
enum class NearestNeighborMethod { CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL };
enum class LSQ_OPTIMIZER_TYPE { GaussNewton, LevenbergMarquardt };

struct PointXYZ {
  float x = 0, y = 0, z = 0;
};

template <typename PointT>
struct PointCloud {
  using Ptr = std::shared_ptr<PointCloud<PointT>>;
  using ConstPtr = std::shared_ptr<const PointCloud<PointT>>;
  std::vector<PointT> points;
  size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  const PointT& at(size_t i) const { return points.at(i); }
  void resize(size_t n) { points.resize(n); }
};

struct Matrix4f {  // row-major 4x4 (Eigen::Matrix4f stand-in)
  float m[16];
  static Matrix4f Identity() { Matrix4f I; std::memset(I.m, 0, sizeof(I.m)); I.m[0] = I.m[5] = I.m[10] = I.m[15] = 1.f; return I; }
  float& operator()(int r, int c) { return m[r * 4 + c]; }
  float operator()(int r, int c) const { return m[r * 4 + c]; }
};

using Matrix6d = std::array<double, 36>;  // row-major (symmetric)
using Vector6d = std::array<double, 6>;
struct Matrix4d {  // row-major 4x4 (Eigen::Matrix4d stand-in)
  double m[16];
  double& operator()(int r, int c) { return m[r * 4 + c]; }
  double operator()(int r, int c) const { return m[r * 4 + c]; }
};
/// one hypothesis of alignMulti (no reference counterpart): what align(guess k) leaves in getFinalTransformation() (here in double),
/// getFinalHessian(), hasConverged(), getNumIterations()
struct MultiAlignResult {
  Matrix4d T;
  Matrix6d H;
  double final_error;
  bool converged;
  int nr_iterations;
};

struct Isometry3d {  // row-major R | t, double
  double R[9];
  double t[3];
  static Isometry3d Identity() { Isometry3d T; std::memset(&T, 0, sizeof(T)); T.R[0] = T.R[4] = T.R[8] = 1.0; return T; }
  template <typename Matrix4>  // Matrix4f or Matrix4d
  static Isometry3d from(const Matrix4& M) {
    Isometry3d T;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T.R[i * 3 + j] = M(i, j); T.t[i] = M(i, 3); }
    return T;
  }
  Matrix4f cast_float() const {
    Matrix4f M = Matrix4f::Identity();
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) M(i, j) = (float)R[i * 3 + j]; M(i, 3) = (float)t[i]; }
    return M;
  }
  Matrix4d matrix() const {
    Matrix4d M;
    std::memset(M.m, 0, sizeof(M.m));
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) M(i, j) = R[i * 3 + j]; M(i, 3) = t[i]; }
    M(3, 3) = 1.0;
    return M;
  }
  void to_colmajor16(double* T16) const {
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T16[j * 4 + i] = R[i * 3 + j]; T16[12 + i] = t[i]; T16[i * 4 + 3] = 0.0; }
    T16[15] = 1.0;
  }
  static Isometry3d from_colmajor16(const double* T16) {
    Isometry3d T;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T.R[i * 3 + j] = T16[j * 4 + i]; T.t[i] = T16[12 + i]; }
    return T;
  }
  Isometry3d operator*(const Isometry3d& B) const {
    Isometry3d C;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) C.R[i * 3 + j] = R[i * 3] * B.R[j] + R[i * 3 + 1] * B.R[3 + j] + R[i * 3 + 2] * B.R[6 + j];
      C.t[i] = R[i * 3] * B.t[0] + R[i * 3 + 1] * B.t[1] + R[i * 3 + 2] * B.t[2] + t[i];
    }
    return C;
  }
};

// so3.hpp:58-104 (rotation first)
inline Isometry3d se3_exp(const Vector6d& a) {
  const double ox = a[0], oy = a[1], oz = a[2];
  const double theta_sq = ox * ox + oy * oy + oz * oz;
  double imag, real;
  if (theta_sq < 1e-10) {
    const double tq = theta_sq * theta_sq;
    imag = 0.5 - theta_sq / 48.0 + tq / 3840.0;
    real = 1.0 - theta_sq / 8.0 + tq / 384.0;
  } else {
    const double th = std::sqrt(theta_sq);
    imag = std::sin(0.5 * th) / th;
    real = std::cos(0.5 * th);
  }
  const double qw = real, qx = imag * ox, qy = imag * oy, qz = imag * oz;
  Isometry3d T;
  T.R[0] = 1 - 2 * (qy * qy + qz * qz); T.R[1] = 2 * (qx * qy - qz * qw);     T.R[2] = 2 * (qx * qz + qy * qw);
  T.R[3] = 2 * (qx * qy + qz * qw);     T.R[4] = 1 - 2 * (qx * qx + qz * qz); T.R[5] = 2 * (qy * qz - qx * qw);
  T.R[6] = 2 * (qx * qz - qy * qw);     T.R[7] = 2 * (qy * qz + qx * qw);     T.R[8] = 1 - 2 * (qx * qx + qy * qy);
  const double theta = std::sqrt(theta_sq);
  double V[9];
  if (theta < 1e-10) {
    std::memcpy(V, T.R, sizeof(V));
  } else {
    const double A = (1.0 - std::cos(theta)) / theta_sq, B = (theta - std::sin(theta)) / (theta_sq * theta);
    const double O[9] = {0, -oz, oy, oz, 0, -ox, -oy, ox, 0};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double o2 = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
        V[i * 3 + j] = (i == j ? 1.0 : 0.0) + A * O[i * 3 + j] + B * o2;
      }
  }
  for (int i = 0; i < 3; i++) T.t[i] = V[i * 3] * a[3] + V[i * 3 + 1] * a[4] + V[i * 3 + 2] * a[5];
  return T;
}

namespace detail {
// A pivot with |d| <= DBL_MIN is handled like Eigen::LDLT (column left unscaled, pseudo-inverse of D in the solve): an
// all-zero system (no correspondences) gives d = 0 and the optimiser returns the guess, converged, as the reference does.
inline void ldlt6_solve(const Matrix6d& A, const Vector6d& rhs, Vector6d& x) {
  double L[36] = {0}, D[6], y[6];
  constexpr double tiny = 2.2250738585072014e-308;
  for (int j = 0; j < 6; j++) {
    double d = A[j * 6 + j];
    for (int k = 0; k < j; k++) d -= L[j * 6 + k] * L[j * 6 + k] * D[k];
    D[j] = d;
    L[j * 6 + j] = 1.0;
    for (int i = j + 1; i < 6; i++) {
      double s = A[i * 6 + j];
      for (int k = 0; k < j; k++) s -= L[i * 6 + k] * L[j * 6 + k] * D[k];
      L[i * 6 + j] = std::fabs(d) > tiny ? s / d : s;
    }
  }
  for (int i = 0; i < 6; i++) { double s = rhs[i]; for (int k = 0; k < i; k++) s -= L[i * 6 + k] * y[k]; y[i] = s; }
  for (int i = 0; i < 6; i++) y[i] = std::fabs(D[i]) > tiny ? y[i] / D[i] : 0.0;
  for (int i = 5; i >= 0; i--) { double s = y[i]; for (int k = i + 1; k < 6; k++) s -= L[k * 6 + i] * x[k]; x[i] = s; }
}
/// the C ABI's 6x6 is column-major, the classes' Matrix6d row-major
inline Matrix6d transposed6(const double* H36) {
  Matrix6d H;
  for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) H[i * 6 + j] = H36[j * 6 + i];
  return H;
}
/// the table LsqRegistration::step_lm prints with setDebugPrint(true) (lsq_registration_impl.hpp:143-149), from the rows the
/// device LM recorded ({i, y0, yi, rho, lambda, |delta|} per trial step)
inline void print_lm_trace(const std::vector<double>& rows) {
  for (size_t r = 0; r + 5 < rows.size(); r += 6) {
    if ((int)rows[r] == 0) std::printf("--- LM optimization ---\n%5s %15s %15s %15s %15s %15s %5s\n", "i", "y0", "yi", "rho", "lambda", "|delta|", "dec");
    std::printf("%5d %15g %15g %15g %15g %15g %5c\n", (int)rows[r], rows[r + 1], rows[r + 2], rows[r + 3], rows[r + 4], rows[r + 5], rows[r + 3] > 0.0 ? 'x' : ' ');
  }
  std::fflush(stdout);  // (std::endl in the reference)
}
/// xyz of a cloud as the C ABI wants it: when the point type starts with three packed floats and is 12 or 16 bytes (PointXYZ
/// here, pcl::PointXYZ upstream) the cloud's own storage is handed over with its stride -- no 200 KB repack per setInputSource;
/// any other point type is packed into `scratch` (stride 3)
template <typename PointT>
struct XyzView {
  const float* data;
  int stride;
  XyzView(const PointCloud<PointT>& c, std::vector<float>& scratch) {
    constexpr bool direct = (sizeof(PointT) == 12 || sizeof(PointT) == 16) && offsetof(PointT, x) == 0 && offsetof(PointT, y) == 4 && offsetof(PointT, z) == 8;
    if (direct) {
      data = c.size() ? &c.points[0].x : nullptr;
      stride = (int)(sizeof(PointT) / sizeof(float));
    } else {
      scratch.resize(c.size() * 3);
      for (size_t i = 0; i < c.size(); i++) { scratch[3 * i] = c.points[i].x; scratch[3 * i + 1] = c.points[i].y; scratch[3 * i + 2] = c.points[i].z; }
      data = scratch.data();
      stride = 3;
    }
  }
};
// out[i] = in[i] with (x, y, z) <- M (x, y, z, 1): pcl::transformPointCloud for the output cloud of align(). It runs between the
// end of one registration and the first launch of the next with the GPU idle, so packed xyz / xyzw points (12- or 16-byte structs)
// go four at a time through SSE (the scalar loop: 50 us for 17k points, ~15 % of a registration). Every lane evaluates
// ((m0 x + m1 y) + m2 z) + m3 in that order without fusing: bit for bit the scalar loop's result.
template <typename PointT>
inline void transform_points_scalar(const PointT* in, PointT* out, size_t begin, size_t n, const float* m) {
  for (size_t i = begin; i < n; i++) {
    PointT q = in[i];
    const float x = q.x, y = q.y, z = q.z;
    q.x = m[0] * x + m[1] * y + m[2] * z + m[3];
    q.y = m[4] * x + m[5] * y + m[6] * z + m[7];
    q.z = m[8] * x + m[9] * y + m[10] * z + m[11];
    out[i] = q;
  }
}
#if defined(__SSE2__)
inline void fvh_sse_rows(const float* m, __m128 X, __m128 Y, __m128 Z, __m128& ox, __m128& oy, __m128& oz) {
  auto row = [&](int r) {
    const __m128 a = _mm_mul_ps(_mm_set1_ps(m[4 * r]), X), b = _mm_mul_ps(_mm_set1_ps(m[4 * r + 1]), Y), c = _mm_mul_ps(_mm_set1_ps(m[4 * r + 2]), Z);
    return _mm_add_ps(_mm_add_ps(_mm_add_ps(a, b), c), _mm_set1_ps(m[4 * r + 3]));
  };
  ox = row(0); oy = row(1); oz = row(2);
}
#endif
template <typename PointT>
inline void transform_points(const PointT* in, PointT* out, size_t n, const float* m) {
  size_t done = 0;
#if defined(__SSE2__)
  constexpr bool xyz_first = offsetof(PointT, x) == 0 && offsetof(PointT, y) == 4 && offsetof(PointT, z) == 8;
  if constexpr (xyz_first && sizeof(PointT) == 16) {  // x y z w: a 4 x 4 transpose each way
    const float* src = reinterpret_cast<const float*>(in);
    float* dst = reinterpret_cast<float*>(out);
    for (; done + 4 <= n; done += 4) {
      __m128 p0 = _mm_loadu_ps(src + 4 * done), p1 = _mm_loadu_ps(src + 4 * done + 4), p2 = _mm_loadu_ps(src + 4 * done + 8), p3 = _mm_loadu_ps(src + 4 * done + 12);
      _MM_TRANSPOSE4_PS(p0, p1, p2, p3);  // p0 = x's, p1 = y's, p2 = z's, p3 = w's
      __m128 ox, oy, oz;
      fvh_sse_rows(m, p0, p1, p2, ox, oy, oz);
      _MM_TRANSPOSE4_PS(ox, oy, oz, p3);
      _mm_storeu_ps(dst + 4 * done, ox); _mm_storeu_ps(dst + 4 * done + 4, oy); _mm_storeu_ps(dst + 4 * done + 8, oz); _mm_storeu_ps(dst + 4 * done + 12, p3);
    }
  } else if constexpr (xyz_first && sizeof(PointT) == 12) {  // x y z packed: 4 points = 3 vectors
    const float* src = reinterpret_cast<const float*>(in);
    float* dst = reinterpret_cast<float*>(out);
    for (; done + 4 <= n; done += 4) {
      const __m128 a = _mm_loadu_ps(src + 3 * done);      // x0 y0 z0 x1
      const __m128 b = _mm_loadu_ps(src + 3 * done + 4);  // y1 z1 x2 y2
      const __m128 c = _mm_loadu_ps(src + 3 * done + 8);  // z2 x3 y3 z3
      const __m128 x2y2x3y3 = _mm_shuffle_ps(b, c, _MM_SHUFFLE(2, 1, 3, 2));
      const __m128 y0z0y1z1 = _mm_shuffle_ps(a, b, _MM_SHUFFLE(1, 0, 2, 1));
      const __m128 X = _mm_shuffle_ps(a, x2y2x3y3, _MM_SHUFFLE(2, 0, 3, 0));         // x0 x1 x2 x3
      const __m128 Y = _mm_shuffle_ps(y0z0y1z1, x2y2x3y3, _MM_SHUFFLE(3, 1, 2, 0));  // y0 y1 y2 y3
      const __m128 Z = _mm_shuffle_ps(y0z0y1z1, c, _MM_SHUFFLE(3, 0, 3, 1));         // z0 z1 z2 z3
      __m128 ox, oy, oz;
      fvh_sse_rows(m, X, Y, Z, ox, oy, oz);
      // back to x0 y0 z0 x1 | y1 z1 x2 y2 | z2 x3 y3 z3
      const __m128 x0x2y0y2 = _mm_shuffle_ps(ox, oy, _MM_SHUFFLE(2, 0, 2, 0));
      const __m128 y1y3z1z3 = _mm_shuffle_ps(oy, oz, _MM_SHUFFLE(3, 1, 3, 1));
      const __m128 z0z2x1x3 = _mm_shuffle_ps(oz, ox, _MM_SHUFFLE(3, 1, 2, 0));
      const __m128 ra = _mm_shuffle_ps(x0x2y0y2, z0z2x1x3, _MM_SHUFFLE(2, 0, 2, 0));  // x0 y0 z0 x1
      const __m128 rb = _mm_shuffle_ps(y1y3z1z3, x0x2y0y2, _MM_SHUFFLE(3, 1, 2, 0));  // y1 z1 x2 y2
      const __m128 rc = _mm_shuffle_ps(z0z2x1x3, y1y3z1z3, _MM_SHUFFLE(3, 1, 3, 1));  // z2 x3 y3 z3
      _mm_storeu_ps(dst + 3 * done, ra); _mm_storeu_ps(dst + 3 * done + 4, rb); _mm_storeu_ps(dst + 3 * done + 8, rc);
    }
  }
#endif
  transform_points_scalar(in, out, done, n, m);
}

template <typename PointT>
inline std::vector<float> pack_xyz(const PointCloud<PointT>& c) {
  std::vector<float> xyz(c.size() * 3);
  for (size_t i = 0; i < c.size(); i++) { xyz[3 * i] = c.points[i].x; xyz[3 * i + 1] = c.points[i].y; xyz[3 * i + 2] = c.points[i].z; }
  return xyz;
}
/// k nearest neighbours of every point from the host kd-tree on `threads` OpenMP threads, n x k (find_neighbors_parallel_kdtree,
/// fast_vgicp_cuda_impl.hpp:152-167). A cloud with fewer than k points: the reference's zero-initialised vector keeps index 0 in the
/// unfilled entries (:155,162; fast_gicp_impl.hpp:253-265)
template <typename PointT>
inline std::vector<int> host_kdtree_neighbors(const PointCloud<PointT>& cloud, int k, int threads) {
  const std::vector<float> xyz = pack_xyz(cloud);
  const int n = (int)cloud.size();
  host::KdTree tree(xyz.data(), n);
  std::vector<int> neighbors((size_t)n * k);
#pragma omp parallel for schedule(guided, 8) num_threads(threads) if (threads > 1)
  for (int i = 0; i < n; i++) {
    int* row = &neighbors[(size_t)i * k];
    tree.knn(&xyz[3 * (size_t)i], k, row);
    for (int j = 0; j < k; j++) if (row[j] < 0) row[j] = 0;
  }
  return neighbors;
}
/// where align() spends its host time (apps/gicp_align, GICP_ALIGN_BREAKDOWN): off unless a caller switches it on
struct HostTiming { bool on = false; double optimize_us = 0, transform_us = 0; };
inline HostTiming& host_timing() { static HostTiming t; return t; }
}  // namespace detail

/// LsqRegistration (lsq_registration.hpp:14-83) minus the PCL base: the members of pcl::Registration its callers use.
template <typename PointSource, typename PointTarget>
class LsqRegistration {
public:
  using PointCloudSource = PointCloud<PointSource>;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = PointCloud<PointTarget>;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;

  LsqRegistration() { final_hessian_.fill(0.0); for (int i = 0; i < 6; i++) final_hessian_[i * 7] = 1.0; }  // lsq_registration_impl.hpp:9-22
  virtual ~LsqRegistration() {}

  void setRotationEpsilon(double eps) { rotation_epsilon_ = eps; }
  void setTransformationEpsilon(double eps) { transformation_epsilon_ = eps; }
  void setMaximumIterations(int n) { max_iterations_ = n; }
  void setInitialLambdaFactor(double f) { lm_init_lambda_factor_ = f; }
  void setDebugPrint(bool p) { lm_debug_print_ = p; }
  void setUseDeviceLM(bool on) { use_device_lm_ = on; }
  /// lsq_optimizer_type_ (lsq_registration.hpp:78: protected there, set by subclasses; LevenbergMarquardt by default, :15). Gauss-Newton
  /// (step_gn, :108-121) is device-resident too (fvh_lm_params::optimizer); setUseDeviceLM(false) runs the reference's host loop on the device's linearize().
  void setLSQType(LSQ_OPTIMIZER_TYPE type) { lsq_optimizer_type_ = type; }
  const Matrix6d& getFinalHessian() const { return final_hessian_; }
  const Matrix4f& getFinalTransformation() const { return final_transformation_; }
  bool hasConverged() const { return converged_; }
  int getNumIterations() const { return nr_iterations_; }

  double evaluateCost(const Matrix4f& relative_pose, Matrix6d* H = nullptr, Vector6d* b = nullptr) { return this->linearize(Isometry3d::from(relative_pose), H, b); }

  virtual void swapSourceAndTarget() {}
  virtual void clearSource() {}
  virtual void clearTarget() {}
  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) { input_ = cloud; }
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) { target_ = cloud; }
  PointCloudSourceConstPtr getInputSource() const { return input_; }
  PointCloudTargetConstPtr getInputTarget() const { return target_; }

  /// pcl::Registration::align
  void align(PointCloudSource& output, const Matrix4f& guess = Matrix4f::Identity()) {
    if (!input_ || (!target_ && !has_device_target())) throw std::invalid_argument("align: source / target cloud not set");
    computeTransformation(output, guess);
  }
  /// pcl::Registration::getFitnessScore(max_range): mean squared exact-NN distance of T*source to the target
  virtual double getFitnessScore(double max_range = std::numeric_limits<double>::max()) = 0;

  /// K initial guesses of the same source / target pair registered in ONE device launch (C ABI: fvh_vgicp_align_multi / fvh_ndt_align_multi;
  /// no reference counterpart). Result k is, bit for bit, what align(guesses[k]) computes under the same grid plan (see the C ABI); the
  /// class's getters are left as the last of K align() calls leaves the device handle. 1 <= K <= 64. Classes whose device LM does not go
  /// through fvh_vgicp_align / fvh_ndt_align (FastGICP) throw.
  std::vector<MultiAlignResult> alignMulti(const std::vector<Matrix4f>& guesses) {
    if (!input_ || (!target_ && !has_device_target())) throw std::invalid_argument("alignMulti: source / target cloud not set");
    const int k = (int)guesses.size();
    std::vector<double> g16(16 * (size_t)k);
    for (int i = 0; i < k; i++) Isometry3d::from(guesses[i]).to_colmajor16(&g16[16 * (size_t)i]);
    const fvh_lm_params p = lm_params();
    std::vector<fvh_lm_result> r((size_t)std::max(k, 1));
    device_align_multi(k, g16.data(), &p, r.data(), &multi_grid_blocks_);
    std::vector<MultiAlignResult> out((size_t)k);
    for (int i = 0; i < k; i++) out[i] = unpack(r[i]);
    return out;
  }
  /// alignMulti, then the pose with the lowest device fitness score (getFitnessScore(max_range) at that pose; ties go to the lowest index)
  /// becomes the result as align() would set it: getFinalTransformation(), hasConverged(), getNumIterations(), getFinalHessian(), `output`.
  /// Returns the chosen index.
  int alignBest(const std::vector<Matrix4f>& guesses, double max_range, PointCloudSource& output) {
    const std::vector<MultiAlignResult> rs = alignMulti(guesses);
    int best = -1;
    double best_score = 0.0;
    for (int i = 0; i < (int)rs.size(); i++) {
      double T16[16];
      Isometry3d::from(rs[i].T).to_colmajor16(T16);
      const double score = device_fitness(T16, max_range);
      if (best < 0 || score < best_score) { best = i; best_score = score; }
    }
    if (best < 0) throw std::invalid_argument("alignBest: no guesses");
    final_transformation_ = take_result(rs[best]).cast_float();
    output.points.resize(input_->size());
    detail::transform_points(input_->points.data(), output.points.data(), input_->size(), final_transformation_.m);
    return best;
  }
  /// workgroups per hypothesis of the last alignMulti (fvh_*_align_multi's grid_blocks_out)
  int getMultiGridBlocks() const { return multi_grid_blocks_; }

protected:
  virtual void computeTransformation(PointCloudSource& output, const Matrix4f& guess) {  // lsq_registration_impl.hpp:53-79
    Isometry3d x0 = Isometry3d::from(guess);
    lm_lambda_ = -1.0;
    converged_ = false;
    detail::HostTiming& ht = detail::host_timing();
    std::chrono::steady_clock::time_point ht0, ht1;
    if (ht.on) ht0 = std::chrono::steady_clock::now();
    if (use_device_lm_ && device_align(x0)) {  // (both optimiser types: Levenberg-Marquardt and, since round 5, Gauss-Newton run inside the kernel)
      // whole loop ran on the GPU
    } else {
      for (int i = 0; i < max_iterations_ && !converged_; i++) {
        nr_iterations_ = i;
        Isometry3d delta;
        if (!step_optimize(x0, delta)) {
          std::fprintf(stderr, "lm not converged!!\n");
          break;
        }
        converged_ = is_converged(delta);
      }
    }
    final_transformation_ = x0.cast_float();
    if (ht.on) ht1 = std::chrono::steady_clock::now();
    output.points.resize(input_->size());  // pcl::transformPointCloud(*input_, output, final_transformation_)
    detail::transform_points(input_->points.data(), output.points.data(), input_->size(), final_transformation_.m);
    if (ht.on) {
      ht.optimize_us += std::chrono::duration<double, std::micro>(ht1 - ht0).count();
      ht.transform_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - ht1).count();
    }
  }

  bool is_converged(const Isometry3d& delta) const {  // :82-91
    double rmax = 0, tmax = 0;
    for (int i = 0; i < 9; i++) rmax = std::max(rmax, std::fabs(delta.R[i] - (i % 4 == 0 ? 1.0 : 0.0)) / rotation_epsilon_);
    for (int i = 0; i < 3; i++) tmax = std::max(tmax, std::fabs(delta.t[i]) / transformation_epsilon_);
    return std::max(rmax, tmax) < 1;
  }

  virtual double linearize(const Isometry3d& trans, Matrix6d* H = nullptr, Vector6d* b = nullptr) = 0;
  virtual double compute_error(const Isometry3d& trans) = 0;
  /// subclasses with a device-resident LM return true after updating x0 / converged_ / nr_iterations_ / final_hessian_
  virtual bool device_align(Isometry3d& x0) { (void)x0; return false; }
  /// the registration target lives on the device without a host cloud behind it (FastVGICPCuda's incremental target map)
  virtual bool has_device_target() const { return false; }
  /// alignMulti / alignBest: the subclass's fvh_*_align_multi and fvh_*_fitness_score
  virtual void device_align_multi(int k, const double* guesses16, const fvh_lm_params* p, fvh_lm_result* results, int* grid_blocks) {
    (void)k; (void)guesses16; (void)p; (void)results; (void)grid_blocks;
    throw std::runtime_error("alignMulti: not offered by this class");
  }
  virtual double device_fitness(const double* T16, double max_range) { (void)T16; (void)max_range; throw std::runtime_error("alignBest: not offered by this class"); }
  int multi_grid_blocks_ = 0;

  /// the parameters of the device-resident optimiser loop, from the setters
  fvh_lm_params lm_params() const {
    return fvh_lm_params{max_iterations_, rotation_epsilon_, transformation_epsilon_, lm_max_iterations_, lm_init_lambda_factor_,
                         lsq_optimizer_type_ == LSQ_OPTIMIZER_TYPE::GaussNewton ? 1 : 0};
  }
  /// a result of the device LM as the classes hand it on: pose and Hessian row-major
  static MultiAlignResult unpack(const fvh_lm_result& r) {
    return MultiAlignResult{Isometry3d::from_colmajor16(r.T).matrix(), detail::transposed6(r.H), r.final_error, r.converged != 0, r.nr_iterations};
  }
  /// ... becomes what the getters report (hasConverged, getNumIterations, getFinalHessian); the pose is returned, where it goes is the caller's
  Isometry3d take_result(const MultiAlignResult& m) {
    converged_ = m.converged;
    nr_iterations_ = m.nr_iterations;
    final_hessian_ = m.H;
    return Isometry3d::from(m.T);
  }
  /// ... straight from the device, with the reference's complaint about a failed LM step (lsq_registration_impl.hpp:69-72)
  Isometry3d take_result(const fvh_lm_result& r) {
    const Isometry3d x = take_result(unpack(r));
    if (r.lm_failed) std::fprintf(stderr, "lm not converged!!\n");
    return x;
  }

  bool step_optimize(Isometry3d& x0, Isometry3d& delta) {  // :94-104
    return lsq_optimizer_type_ == LSQ_OPTIMIZER_TYPE::GaussNewton ? step_gn(x0, delta) : step_lm(x0, delta);
  }
  bool step_gn(Isometry3d& x0, Isometry3d& delta) {  // :108-121
    Matrix6d H;
    Vector6d b, nb, d;
    linearize(x0, &H, &b);
    for (int j = 0; j < 6; j++) nb[j] = -b[j];
    detail::ldlt6_solve(H, nb, d);
    delta = se3_exp(d);
    x0 = delta * x0;
    final_hessian_ = H;
    return true;
  }
  bool step_lm(Isometry3d& x0, Isometry3d& delta) {  // :123-168
    Matrix6d H;
    Vector6d b;
    const double y0 = linearize(x0, &H, &b);
    if (lm_lambda_ < 0.0) {
      double mx = 0;
      for (int i = 0; i < 6; i++) mx = std::max(mx, std::fabs(H[i * 7]));
      lm_lambda_ = lm_init_lambda_factor_ * mx;
    }
    double nu = 2.0;
    for (int i = 0; i < lm_max_iterations_; i++) {
      Matrix6d A = H;
      Vector6d nb, d;
      for (int j = 0; j < 6; j++) { A[j * 7] += lm_lambda_; nb[j] = -b[j]; }
      detail::ldlt6_solve(A, nb, d);
      delta = se3_exp(d);
      const Isometry3d xi = delta * x0;
      const double yi = compute_error(xi);
      double denom = 0;
      for (int j = 0; j < 6; j++) denom += d[j] * (lm_lambda_ * d[j] - b[j]);
      const double rho = (y0 - yi) / denom;
      if (lm_debug_print_) {
        double dn = 0;
        for (int j = 0; j < 6; j++) dn += d[j] * d[j];
        if (i == 0) std::printf("--- LM optimization ---\n%5s %15s %15s %15s %15s %15s %5s\n", "i", "y0", "yi", "rho", "lambda", "|delta|", "dec");
        std::printf("%5d %15g %15g %15g %15g %15g %5c\n", i, y0, yi, rho, lm_lambda_, std::sqrt(dn), rho > 0.0 ? 'x' : ' ');
        std::fflush(stdout);
      }
      if (rho < 0) {
        if (is_converged(delta)) return true;
        lm_lambda_ = nu * lm_lambda_;
        nu = 2 * nu;
        continue;
      }
      x0 = xi;
      lm_lambda_ = lm_lambda_ * std::max(1.0 / 3.0, 1 - std::pow(2 * rho - 1, 3));
      final_hessian_ = H;
      return true;
    }
    return false;
  }

protected:
  PointCloudSourceConstPtr input_;
  PointCloudTargetConstPtr target_;
  Matrix4f final_transformation_ = Matrix4f::Identity();
  int nr_iterations_ = 0;
  int max_iterations_ = 64;               // :11
  double transformation_epsilon_ = 5e-4;  // :13
  bool converged_ = false;
  double rotation_epsilon_ = 2e-3;        // :12
  LSQ_OPTIMIZER_TYPE lsq_optimizer_type_ = LSQ_OPTIMIZER_TYPE::LevenbergMarquardt;
  int lm_max_iterations_ = 10;            // :17
  double lm_init_lambda_factor_ = 1e-9;   // :18
  double lm_lambda_ = -1.0;
  bool lm_debug_print_ = false;
  bool use_device_lm_ = true;
  Matrix6d final_hessian_;
};

/// what clearTargetAlongRays() reports: voxels removed, rays that were walked (not skipped)
struct RayClearing { int removed = 0, rays_used = 0; };

/// what scoreTarget() reports (C ABI: fvh_map_score + the per-point rows): how well the target voxel map explains the source at a pose
struct MapScore {
  int n_points = 0, n_used = 0, n_in_voxel = 0, n_near = 0, n_explained = 0;
  double sum_best_m2 = 0.0, sum_score_max = 0.0, sum_score_all = 0.0;
  std::vector<int> found, best;   // with per_point: one row per source point, in input order (skipped points: -1, -1, NaN)
  std::vector<double> best_m2;
  double overlap() const { return n_used ? (double)n_in_voxel / n_used : std::numeric_limits<double>::quiet_NaN(); }   // share of points inside occupied voxels
  double nvtl() const { return n_near ? sum_score_max / n_near : std::numeric_limits<double>::quiet_NaN(); }           // nearest voxel transformation likelihood
  double tp() const { return n_used ? sum_score_all / n_used : std::numeric_limits<double>::quiet_NaN(); }             // transform probability
};

/// what castRays() / castRaysToSource() report (C ABI: fvh_ray_cast + the per-ray rows): what the target voxel map says a sensor should see
struct RayCast {
  int n_rays = 0, n_used = 0, n_hit = 0, n_hit_at_origin = 0;
  long long n_cells = 0;
  std::vector<int> hit, cell;      // with per_ray: hit one row per ray in input order (1, 0 no hit, -1 skipped), cell three per ray
  std::vector<double> range, m2;   // ... the range of the hit in metres and its squared Mahalanobis distance (+inf without a hit, NaN when skipped)
  double hitRatio() const { return n_used ? (double)n_hit / n_used : std::numeric_limits<double>::quiet_NaN(); }  // share of used rays that hit the map
};

/// A snapshot of an incremental target map (FastVGICPCuda / NDTCuda exportTargetMap / importTargetMap; C ABI: fvh_vgicp_voxelmap_export /
/// _import, fvh_ndt_voxelmap_export / _import): per voxel coords[3], the device's ten fp64 sums and an age, rows in ascending packed-key
/// order (z-major, then y, then x).
struct TargetMapSnapshot {
  double resolution = 1.0;
  int mode = 0;          // 0 additive, 2 multiplicative (FastVGICPCuda); 3 = FVH_VOXEL_NDT_SUMS (NDTCuda)
  int num_inserts = 0;   // the map's insert count
  long long num_points = 0;
  std::vector<int> coords;      // 3 per voxel
  std::vector<double> sums;     // 10 per voxel: {sum p | sum C^-1 p (3), sum C | sum C^-1 | sum p p^T (6), count}
  std::vector<unsigned> ages;   // inserts since the voxel was last touched
  int num_voxels() const { return (int)ages.size(); }
};

namespace detail {
inline void write_map_file(const std::string& path, const TargetMapSnapshot& m);  // (below: "Map snapshot files")
inline TargetMapSnapshot read_map_file(const std::string& path);
inline void check(int rc, const char* what, const char* err) {
  if (rc != 0) throw std::runtime_error(std::string(what) + " failed (status " + std::to_string(rc) + "): " + (err ? err : ""));
}

/// One C ABI call and the label detail::check puts into the exception text when it fails
template <typename Fn>
struct DeviceCall {
  Fn fn;
  const char* label;
};
/// What the registration classes ask of a handle whatever its correspondence model: the table DeviceRegistration works through
/// (a null fn: the model has no such call)
template <typename Handle>
struct DeviceCalls {
  const char* (*last_error)(const Handle*);
  DeviceCall<int (*)(Handle*, const float*, int, int)> set_source_cloud_strided, set_target_cloud_strided;
  DeviceCall<int (*)(Handle*, const double*)> update_correspondences;
  DeviceCall<int (*)(Handle*, const double*, double*, double*, double*)> compute_error;
  DeviceCall<int (*)(Handle*, const double*, const fvh_lm_params*, fvh_lm_result*)> align;
  DeviceCall<int (*)(Handle*, int, const double*, const fvh_lm_params*, fvh_lm_result*, int*)> align_multi;
  DeviceCall<int (*)(Handle*, const double*, double, double*)> fitness_score;
  DeviceCall<int (*)(Handle*, int)> set_lm_trace;
  DeviceCall<int (*)(Handle*, int*, double*)> get_lm_trace;
  DeviceCall<int (*)(Handle*, const double*, const fvh_lm_params*)> align_async;
  DeviceCall<int (*)(Handle*, fvh_lm_result*)> align_wait;
};
/// VGICP: voxels of the target (FastVGICPCuda, FastVGICP)
inline constexpr DeviceCalls<fvh_vgicp> kVgicpVoxelCalls{
    fvh_vgicp_last_error,
    {fvh_vgicp_set_source_cloud_strided, "set_source_cloud"}, {fvh_vgicp_set_target_cloud_strided, "set_target_cloud"},
    {fvh_vgicp_update_correspondences, "update_correspondences"}, {fvh_vgicp_compute_error, "compute_error"},
    {fvh_vgicp_align, "align"}, {fvh_vgicp_align_multi, "align_multi"}, {fvh_vgicp_fitness_score, "fitness_score"},
    {fvh_vgicp_set_lm_trace, "set_lm_trace"}, {fvh_vgicp_get_lm_trace, "get_lm_trace"},
    {fvh_vgicp_align_async, "align_async"}, {fvh_vgicp_align_wait, "align_wait"}};
/// GICP: the nearest target point, on the same handle (FastGICP); no multi-hypothesis and no asynchronous align
inline constexpr DeviceCalls<fvh_vgicp> kVgicpNearestPointCalls{
    fvh_vgicp_last_error,
    {fvh_vgicp_set_source_cloud_strided, "set_source_cloud"}, {fvh_vgicp_set_target_cloud_strided, "set_target_cloud"},
    {fvh_vgicp_gicp_update_correspondences, "gicp_update_correspondences"}, {fvh_vgicp_gicp_compute_error, "gicp_compute_error"},
    {fvh_vgicp_gicp_align, "gicp_align"}, {nullptr, "align_multi"}, {fvh_vgicp_fitness_score, "fitness_score"},
    {fvh_vgicp_set_lm_trace, "set_lm_trace"}, {fvh_vgicp_get_lm_trace, "get_lm_trace"},
    {nullptr, "align_async"}, {nullptr, "align_wait"}};
/// NDT (NDTCuda)
inline constexpr DeviceCalls<fvh_ndt> kNdtCalls{
    fvh_ndt_last_error,
    {fvh_ndt_set_source_cloud_strided, "set_source_cloud"}, {fvh_ndt_set_target_cloud_strided, "set_target_cloud"},
    {fvh_ndt_update_correspondences, "update_correspondences"}, {fvh_ndt_compute_error, "compute_error"},
    {fvh_ndt_align, "align"}, {fvh_ndt_align_multi, "align_multi"}, {fvh_ndt_fitness_score, "fitness_score"},
    {fvh_ndt_set_lm_trace, "set_lm_trace"}, {fvh_ndt_get_lm_trace, "get_lm_trace"},
    {fvh_ndt_align_async, "align_async"}, {fvh_ndt_align_wait, "align_wait"}};
/// The incremental target map, its snapshots and the map score (FastVGICPCuda, NDTCuda; the score: FastVGICP too). Not part of the tables above: these are inline functions of a
/// class template, so a program refers to a handle type's map calls only if it uses them
template <typename Handle>
struct MapCalls;
template <>
struct MapCalls<fvh_vgicp> {
  static int begin(fvh_vgicp* h, int expected_voxels) { return fvh_vgicp_map_begin(h, expected_voxels); }
  static int insert_source(fvh_vgicp* h, const double* T16) { return fvh_vgicp_map_insert_source(h, T16); }
  static int prune(fvh_vgicp* h, const double* c3, double radius, int max_age, int* removed) { return fvh_vgicp_map_prune(h, c3, radius, max_age, removed); }
  static int clear_rays_source(fvh_vgicp* h, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, int* removed, int* rays_used) { return fvh_vgicp_clear_rays_source(h, T16, origin3, min_range, max_range, end_margin, min_misses, removed, rays_used); }
  static int export_rows(fvh_vgicp* h, int* n, double* res, int* mode, int* inserts, long long* points, int* coords, double* sums, unsigned* ages) { return fvh_vgicp_voxelmap_export(h, n, res, mode, inserts, points, coords, sums, ages); }
  static int import_rows(fvh_vgicp* h, int n, const int* coords, const double* sums, const unsigned* ages, double res, int mode, int inserts, long long points) { return fvh_vgicp_voxelmap_import(h, n, coords, sums, ages, res, mode, inserts, points); }
  static int merge_from(fvh_vgicp* h, fvh_vgicp* other) { return fvh_vgicp_voxelmap_merge_from(h, other); }
  static int merge_from_posed(fvh_vgicp* h, fvh_vgicp* other, const double* T16, int* rows_skipped) { return fvh_vgicp_posed_merge_from(h, other, T16, rows_skipped); }
  static int transform(fvh_vgicp* h, const double* T16, int* rows_skipped) { return fvh_vgicp_transform_map(h, T16, rows_skipped); }
  static int target_from_map(fvh_vgicp* h, int min_points, int* num_points) { return fvh_vgicp_target_from_map(h, min_points, num_points); }
  static int num_source_points(fvh_vgicp* h, int* n) { return fvh_vgicp_get_num_source_points(h, n); }
  static int cast_rays_source(fvh_vgicp* h, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2) { return fvh_vgicp_cast_rays_source(h, T16, origin3, min_range, max_range, min_points, max_m2, out, hit, cell3, range, m2); }
  static int cast_rays_cloud(fvh_vgicp* h, const float* xyz, int n, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2) { return fvh_vgicp_cast_rays_cloud(h, xyz, n, 3, 0, T16, origin3, min_range, max_range, min_points, max_m2, out, hit, cell3, range, m2); }
  static int score_source(fvh_vgicp* h, const double* T16, int neighbors, int min_points, double max_m2, double score_scale, fvh_map_score* out, int* found, int* best, double* best_m2) { return fvh_vgicp_score_source(h, T16, neighbors, min_points, max_m2, score_scale, out, found, best, best_m2); }
};
template <>
struct MapCalls<fvh_ndt> {
  static int begin(fvh_ndt* h, int expected_voxels) { return fvh_ndt_map_begin(h, expected_voxels); }
  static int insert_source(fvh_ndt* h, const double* T16) { return fvh_ndt_map_insert_source(h, T16); }
  static int prune(fvh_ndt* h, const double* c3, double radius, int max_age, int* removed) { return fvh_ndt_map_prune(h, c3, radius, max_age, removed); }
  static int clear_rays_source(fvh_ndt* h, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, int* removed, int* rays_used) { return fvh_ndt_clear_rays_source(h, T16, origin3, min_range, max_range, end_margin, min_misses, removed, rays_used); }
  static int export_rows(fvh_ndt* h, int* n, double* res, int* mode, int* inserts, long long* points, int* coords, double* sums, unsigned* ages) { return fvh_ndt_voxelmap_export(h, n, res, mode, inserts, points, coords, sums, ages); }
  static int import_rows(fvh_ndt* h, int n, const int* coords, const double* sums, const unsigned* ages, double res, int mode, int inserts, long long points) { return fvh_ndt_voxelmap_import(h, n, coords, sums, ages, res, mode, inserts, points); }
  static int merge_from(fvh_ndt* h, fvh_ndt* other) { return fvh_ndt_voxelmap_merge_from(h, other); }
  static int merge_from_posed(fvh_ndt* h, fvh_ndt* other, const double* T16, int* rows_skipped) { return fvh_ndt_posed_merge_from(h, other, T16, rows_skipped); }
  static int transform(fvh_ndt* h, const double* T16, int* rows_skipped) { return fvh_ndt_transform_map(h, T16, rows_skipped); }
  static int target_from_map(fvh_ndt* h, int min_points, int* num_points) { return fvh_ndt_target_from_map(h, min_points, num_points); }
  static int num_source_points(fvh_ndt* h, int* n) { return fvh_ndt_get_num_source_points(h, n); }
  static int cast_rays_source(fvh_ndt* h, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2) { return fvh_ndt_cast_rays_source(h, T16, origin3, min_range, max_range, min_points, max_m2, out, hit, cell3, range, m2); }
  static int cast_rays_cloud(fvh_ndt* h, const float* xyz, int n, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2) { return fvh_ndt_cast_rays_cloud(h, xyz, n, 3, 0, T16, origin3, min_range, max_range, min_points, max_m2, out, hit, cell3, range, m2); }
  static int score_source(fvh_ndt* h, const double* T16, int neighbors, int min_points, double max_m2, double score_scale, fvh_map_score* out, int* found, int* best, double* best_m2) { return fvh_ndt_score_source(h, T16, neighbors, min_points, max_m2, score_scale, out, found, best, best_m2); }
};
}  // namespace detail

/// What FastVGICPCuda, FastGICP, FastVGICP and NDTCuda share (no reference counterpart): the device handle and LsqRegistration's
/// virtuals on top of it, written once against a detail::DeviceCalls table. The classes create and destroy the handle and add what
/// is theirs: parameters, covariances, voxel maps.
template <typename Handle, typename PointSource, typename PointTarget>
class DeviceRegistration : public LsqRegistration<PointSource, PointTarget> {
  using Base = LsqRegistration<PointSource, PointTarget>;
  using Map = detail::MapCalls<Handle>;

public:
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;

  DeviceRegistration(const DeviceRegistration&) = delete;
  DeviceRegistration& operator=(const DeviceRegistration&) = delete;

  void clearSource() override { this->input_.reset(); }
  void clearTarget() override { this->target_.reset(); }
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    double T16[16];
    Isometry3d::from(this->final_transformation_).to_colmajor16(T16);
    return device_fitness(T16, max_range);
  }
  Handle* core() { return core_; }

protected:
  explicit DeviceRegistration(const detail::DeviceCalls<Handle>* calls) : calls_(calls) {}

  /// the first half of setInputSource / setInputTarget: false when `cloud` is the one already set, else it is kept and uploaded
  bool take_source(const PointCloudSourceConstPtr& cloud) {
    if (cloud == this->input_) return false;
    this->input_ = cloud;
    const detail::XyzView<PointSource> view(*cloud, scratch_xyz_);
    call(calls_->set_source_cloud_strided, view.data, (int)cloud->size(), view.stride);
    return true;
  }
  bool take_target(const PointCloudTargetConstPtr& cloud) {
    if (cloud == this->target_) return false;
    this->target_ = cloud;
    const detail::XyzView<PointTarget> view(*cloud, scratch_xyz_);
    call(calls_->set_target_cloud_strided, view.data, (int)cloud->size(), view.stride);
    return true;
  }
  /// the registration as a two-stage pipeline: the classes whose handle offers it make these two public. alignWait() returns the pose
  /// without transforming a host cloud.
  void alignAsync(const Matrix4f& guess = Matrix4f::Identity()) {
    double g16[16];
    Isometry3d::from(guess).to_colmajor16(g16);
    const fvh_lm_params p = this->lm_params();
    call(calls_->align_async, g16, &p);
  }
  const Matrix4f& alignWait() {
    fvh_lm_result r;
    call(calls_->align_wait, &r);
    return this->final_transformation_ = this->take_result(r).cast_float();
  }

  // ---- incremental target map and its snapshots (no reference counterpart; C ABI: fvh_vgicp_map_* / fvh_ndt_map_*, fvh_*_voxelmap_*, through detail::MapCalls): the
  // classes whose handle offers them (FastVGICPCuda, NDTCuda) make these public; what is theirs -- setInputTarget ending the mode,
  // loadTargetMap choosing the voxel type -- stays with them.
  void beginIncrementalTarget(int expected_voxels = 0) {
    call(Map::begin(core_, expected_voxels), "map_begin");
    this->target_.reset();
    incremental_target_ = true;
  }
  /// adds the current source (as setInputSource left it) to the map at pose T
  void insertSourceIntoTarget(const Matrix4f& T) {
    if (!this->input_) throw std::invalid_argument("insertSourceIntoTarget: source cloud not set");
    double T16[16];
    Isometry3d::from(T).to_colmajor16(T16);
    call(Map::insert_source(core_, T16), "map_insert_source");
  }
  /// ... at the final transformation of the last align()
  void insertSourceIntoTarget() { insertSourceIntoTarget(this->final_transformation_); }
  /// drops voxels further than `radius` from `center` (null: no distance rule) and those untouched by the last max_age inserts (<= 0: no age rule); returns the number removed
  int pruneTarget(const double* center3, double radius, int max_age = 0) {
    int removed = 0;
    call(Map::prune(core_, center3, radius, max_age, &removed), "map_prune");
    return removed;
  }
  /// Free-space carving (fvh_*_clear_rays_source): drops the voxels that at least min_misses rays of this call cross and none ends in. The
  /// rays run from origin3 (scan frame; null: the origin) to the current source points, all at pose T -- the pose insertSourceIntoTarget(T)
  /// would add the scan at: call this first, then insert. Rays outside [min_range, max_range] metres are skipped and a walk stops end_margin
  /// metres in front of its endpoint; end_margin (a voxel or two) and min_misses > 1 keep grazing rays from eroding the ground.
  RayClearing clearTargetAlongRays(const Matrix4f& T, const double* origin3 = nullptr, double min_range = 0.0, double max_range = 100.0, double end_margin = 0.0, int min_misses = 1) {
    if (!this->input_) throw std::invalid_argument("clearTargetAlongRays: source cloud not set");
    double T16[16];
    Isometry3d::from(T).to_colmajor16(T16);
    RayClearing out;
    call(Map::clear_rays_source(core_, T16, origin3, min_range, max_range, end_margin, min_misses, &out.removed, &out.rays_used), "clear_rays_source");
    return out;
  }
  /// How well the target voxel map (batch or incremental) explains the current source at pose T (fvh_*_score_source through
  /// detail::MapCalls, read-only on the handle; public on the classes that own a voxel map: FastVGICPCuda, FastVGICP, NDTCuda): around
  /// every point the voxels of `neighbors` (DIRECT1 / DIRECT7 / DIRECT27) with >= min_points points are looked up and the squared
  /// Mahalanobis distance to each voxel's Gaussian is formed; a point is explained when its best one is finite and <= max_m2; scores are
  /// exp(-0.5 * score_scale * m2). per_point: also found / best / best_m2 per source point. The source is the HANDLE's -- one set by
  /// setInputSource or one adopted from a device-side preparation, which leaves no host cloud behind: the rows are sized by the handle's count.
  MapScore scoreTarget(const Matrix4f& T, NeighborSearchMethod neighbors = NeighborSearchMethod::DIRECT7, int min_points = 1,
                       double max_m2 = std::numeric_limits<double>::infinity(), double score_scale = 1.0, bool per_point = false) {
    double T16[16];
    Isometry3d::from(T).to_colmajor16(T16);
    MapScore out;
    fvh_map_score s;
    int rows = 0;
    if (per_point) call(Map::num_source_points(core_, &rows), "get_num_source_points");
    const size_t n = (size_t)rows;
    out.found.resize(n); out.best.resize(n); out.best_m2.resize(n);
    call(Map::score_source(core_, T16, (int)neighbors, min_points, max_m2, score_scale, &s, n ? out.found.data() : nullptr, n ? out.best.data() : nullptr, n ? out.best_m2.data() : nullptr), "score_source");
    out.n_points = s.n_points; out.n_used = s.n_used; out.n_in_voxel = s.n_in_voxel; out.n_near = s.n_near; out.n_explained = s.n_explained;
    out.sum_best_m2 = s.sum_best_m2; out.sum_score_max = s.sum_score_max; out.sum_score_all = s.sum_score_all;
    return out;
  }
  /// ... at the final transformation of the last align()
  MapScore scoreTarget() { return scoreTarget(this->final_transformation_); }
  /// What the target voxel map (batch or incremental) says a sensor at pose T should see along each ray (fvh_*_cast_rays_cloud through
  /// detail::MapCalls, read-only on the handle; public on the classes that own a voxel map: FastVGICPCuda, FastVGICP, NDTCuda). A ray is
  /// the segment from origin3 (scan frame; null: the origin) to an endpoint (endpoints_xyz: three floats per ray, scan frame); it is walked
  /// through the grid, in every voxel with >= min_points points its point of smallest squared Mahalanobis distance to the voxel's Gaussian
  /// is found, and the first voxel where that is <= max_m2 (and beyond min_range metres) is the hit. Rays longer than max_range are
  /// skipped. per_ray: also hit / cell / range / m2 per ray. The intended loop: align, castRaysToSource(T) and compare with the measured
  /// ranges, clearTargetAlongRays(T), insertSourceIntoTarget(T).
  RayCast castRays(const Matrix4f& T, const std::vector<float>& endpoints_xyz, const double* origin3 = nullptr, double min_range = 0.0, double max_range = 100.0, int min_points = 1,
                   double max_m2 = std::numeric_limits<double>::infinity(), bool per_ray = true) {
    if (endpoints_xyz.size() % 3) throw std::invalid_argument("castRays: endpoints_xyz must hold three floats per ray");
    return cast_rays(T, endpoints_xyz.data(), (int)(endpoints_xyz.size() / 3), false, origin3, min_range, max_range, min_points, max_m2, per_ray);
  }
  /// ... with the handle's current source points as the endpoints (fvh_*_cast_rays_source): the rows are sized by the handle's count
  RayCast castRaysToSource(const Matrix4f& T, const double* origin3 = nullptr, double min_range = 0.0, double max_range = 100.0, int min_points = 1,
                           double max_m2 = std::numeric_limits<double>::infinity(), bool per_ray = true) {
    return cast_rays(T, nullptr, 0, true, origin3, min_range, max_range, min_points, max_m2, per_ray);
  }
  bool hasIncrementalTarget() const { return incremental_target_; }
private:
  RayCast cast_rays(const Matrix4f& T, const float* xyz, int n, bool to_source, const double* origin3, double min_range, double max_range, int min_points, double max_m2, bool per_ray) {
    double T16[16];
    Isometry3d::from(T).to_colmajor16(T16);
    RayCast out;
    fvh_ray_cast s;
    int rows = n;
    if (to_source) { rows = 0; if (per_ray) call(Map::num_source_points(core_, &rows), "get_num_source_points"); }
    const size_t m = per_ray ? (size_t)rows : 0;
    out.hit.resize(m); out.cell.resize(3 * m); out.range.resize(m); out.m2.resize(m);
    int* hit = m ? out.hit.data() : nullptr;
    int* cell = m ? out.cell.data() : nullptr;
    double* range = m ? out.range.data() : nullptr;
    double* m2 = m ? out.m2.data() : nullptr;
    if (to_source) call(Map::cast_rays_source(core_, T16, origin3, min_range, max_range, min_points, max_m2, &s, hit, cell, range, m2), "cast_rays_source");
    else call(Map::cast_rays_cloud(core_, n ? xyz : nullptr, n, T16, origin3, min_range, max_range, min_points, max_m2, &s, hit, cell, range, m2), "cast_rays_cloud");
    out.n_rays = s.n_rays; out.n_used = s.n_used; out.n_hit = s.n_hit; out.n_hit_at_origin = s.n_hit_at_origin; out.n_cells = s.n_cells;
    return out;
  }
protected:
  /// The live map becomes the handle's target CLOUD as well: one point per voxel with >= min_points points (the voxel's mean; VGICP: + its
  /// covariance), rows in ascending key order -- the row order of exportTargetMap(). getFitnessScore() and alignBest() then work on the map.
  /// A snapshot: call it again after an insert or a prune. The map stays the align target. Returns the number of points.
  int targetCloudFromMap(int min_points = 1) {
    int n = 0;
    call(Map::target_from_map(core_, min_points, &n), "target_from_map");
    return n;
  }
  TargetMapSnapshot exportTargetMap() {
    TargetMapSnapshot m;
    int n = 0;
    call(Map::export_rows(core_, &n, &m.resolution, &m.mode, &m.num_inserts, &m.num_points, nullptr, nullptr, nullptr), "voxelmap_export");
    m.coords.resize(3 * (size_t)n); m.sums.resize(10 * (size_t)n); m.ages.resize((size_t)n);
    if (n) call(Map::export_rows(core_, &n, &m.resolution, &m.mode, &m.num_inserts, &m.num_points, m.coords.data(), m.sums.data(), m.ages.data()), "voxelmap_export");
    return m;
  }
  /// adds the snapshot's voxels into the live incremental target (same resolution and mode)
  void importTargetMap(const TargetMapSnapshot& m) {
    const size_t n = m.ages.size();
    if (m.coords.size() != 3 * n || m.sums.size() != 10 * n) throw std::invalid_argument("importTargetMap: coords, sums and ages differ in length");
    call(Map::import_rows(core_, (int)n, n ? m.coords.data() : nullptr, n ? m.sums.data() : nullptr, n ? m.ages.data() : nullptr, m.resolution, m.mode, m.num_inserts, m.num_points), "voxelmap_import");
  }
  void merge_target_from(DeviceRegistration& other) { call(Map::merge_from(core_, other.core_), "voxelmap_merge_from"); }  // (the classes' mergeTargetFrom takes their own type)
  /// `other`'s live map, seen from pose T (other's frame -> this map's frame, rigid), added into this one on the device: every voxel's sums are
  /// transformed in closed form and go to the voxel of their own mean (C ABI: fvh_*_posed_merge_from). Returns the rows skipped because
  /// their mean left the key range. (the classes' mergeTargetFromPosed takes their own type)
  int merge_target_from_posed(DeviceRegistration& other, const Isometry3d& T) {
    double T16[16];
    int skipped = 0;
    T.to_colmajor16(T16);
    call(Map::merge_from_posed(core_, other.core_, T16, &skipped), "posed_merge_from");
    return skipped;
  }
  /// re-anchors the live incremental target by the rigid pose T in place (fvh_*_transform_map); insert count, point count and ages stay
  int transformTargetMap(const Isometry3d& T) {
    double T16[16];
    int skipped = 0;
    T.to_colmajor16(T16);
    call(Map::transform(core_, T16, &skipped), "transform_map");
    return skipped;
  }
  void saveTargetMap(const std::string& path) { detail::write_map_file(path, exportTargetMap()); }
  bool has_device_target() const override { return incremental_target_; }
  bool incremental_target_ = false;  // beginIncrementalTarget .. setInputTarget

  double linearize(const Isometry3d& trans, Matrix6d* H, Vector6d* b) override {
    double T16[16], err = 0, Hc[36];
    trans.to_colmajor16(T16);
    call(calls_->update_correspondences, T16);
    call(calls_->compute_error, T16, (H && b) ? Hc : nullptr, (H && b) ? b->data() : nullptr, &err);
    if (H && b) *H = detail::transposed6(Hc);
    return err;
  }
  double compute_error(const Isometry3d& trans) override {
    double T16[16], err = 0;
    trans.to_colmajor16(T16);
    call(calls_->compute_error, T16, nullptr, nullptr, &err);
    return err;
  }
  /// the whole LM loop on the device; with setDebugPrint(true) the rows it recorded are printed afterwards
  bool device_align(Isometry3d& x0) override {
    double g16[16];
    x0.to_colmajor16(g16);
    const fvh_lm_params p = this->lm_params();
    fvh_lm_result r;
    call(calls_->set_lm_trace, this->lm_debug_print_ ? 1 : 0);
    call(calls_->align, g16, &p, &r);
    if (this->lm_debug_print_) {
      int n = 0;
      call(calls_->get_lm_trace, &n, nullptr);
      std::vector<double> rows(6 * (size_t)n);
      if (n) call(calls_->get_lm_trace, &n, rows.data());
      detail::print_lm_trace(rows);
    }
    x0 = this->take_result(r);
    return true;
  }
  void device_align_multi(int k, const double* guesses16, const fvh_lm_params* p, fvh_lm_result* results, int* grid_blocks) override {
    if (!calls_->align_multi.fn) return Base::device_align_multi(k, guesses16, p, results, grid_blocks);  // (throws: not offered)
    call(calls_->align_multi, k, guesses16, p, results, grid_blocks);
  }
  double device_fitness(const double* T16, double max_range) override {
    double score = 0;
    call(calls_->fitness_score, T16, max_range, &score);
    return score;
  }

  /// throws "<what> failed (status N): <the handle's last error>" unless rc is FVH_OK
  void call(int rc, const char* what) const { detail::check(rc, what, calls_->last_error(core_)); }
  template <typename Fn, typename... Args>
  void call(const detail::DeviceCall<Fn>& c, Args... args) const {
    if (!c.fn) throw std::runtime_error(std::string(c.label) + ": not offered by this class");
    call(c.fn(core_, args...), c.label);
  }

  const detail::DeviceCalls<Handle>* calls_;
  Handle* core_ = nullptr;
  std::vector<float> scratch_xyz_;  // only used for point types that are not 12 / 16 bytes of packed xyz
};

namespace detail {
// Map snapshot files, little-endian (INTEGRATION.md "Map snapshot files"; fast_gicp_amd/capi.py write_map_file / read_map_file write the same bytes):
// magic "FVHVMAP\0" | version u32 = 1 | mode i32 | num_inserts i32 | num_voxels i32 | num_points i64 | resolution f64 | coords | sums | ages
constexpr char kMapFileMagic[8] = {'F', 'V', 'H', 'V', 'M', 'A', 'P', '\0'};
constexpr unsigned kMapFileVersion = 1;
constexpr size_t kMapFileHeaderBytes = 40;
inline void write_map_file(const std::string& path, const TargetMapSnapshot& m) {
  const size_t n = m.ages.size();
  if (m.coords.size() != 3 * n || m.sums.size() != 10 * n) throw std::invalid_argument("write_map_file: coords, sums and ages differ in length");
  unsigned char hdr[kMapFileHeaderBytes];
  const unsigned version = kMapFileVersion;
  const int nv = (int)n;
  std::memcpy(hdr, kMapFileMagic, 8);
  std::memcpy(hdr + 8, &version, 4);
  std::memcpy(hdr + 12, &m.mode, 4);
  std::memcpy(hdr + 16, &m.num_inserts, 4);
  std::memcpy(hdr + 20, &nv, 4);
  std::memcpy(hdr + 24, &m.num_points, 8);
  std::memcpy(hdr + 32, &m.resolution, 8);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("write_map_file: cannot open " + path);
  bool ok = std::fwrite(hdr, 1, sizeof(hdr), f) == sizeof(hdr);
  if (n) {
    ok = ok && std::fwrite(m.coords.data(), sizeof(int), 3 * n, f) == 3 * n;
    ok = ok && std::fwrite(m.sums.data(), sizeof(double), 10 * n, f) == 10 * n;
    ok = ok && std::fwrite(m.ages.data(), sizeof(unsigned), n, f) == n;
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) throw std::runtime_error("write_map_file: write to " + path + " failed");
}
inline TargetMapSnapshot read_map_file(const std::string& path) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("read_map_file: cannot open " + path);
  struct Closer { std::FILE* f; ~Closer() { std::fclose(f); } } closer{f};
  unsigned char hdr[kMapFileHeaderBytes];
  if (std::fread(hdr, 1, sizeof(hdr), f) != sizeof(hdr)) throw std::runtime_error("read_map_file: " + path + " is not a map snapshot (shorter than the header)");
  if (std::memcmp(hdr, kMapFileMagic, 8) != 0) throw std::runtime_error("read_map_file: " + path + " is not a map snapshot (magic)");
  unsigned version = 0;
  int nv = 0;
  TargetMapSnapshot m;
  std::memcpy(&version, hdr + 8, 4);
  std::memcpy(&m.mode, hdr + 12, 4);
  std::memcpy(&m.num_inserts, hdr + 16, 4);
  std::memcpy(&nv, hdr + 20, 4);
  std::memcpy(&m.num_points, hdr + 24, 8);
  std::memcpy(&m.resolution, hdr + 32, 8);
  if (version != kMapFileVersion) throw std::runtime_error("read_map_file: " + path + " has version " + std::to_string(version) + ", this build reads " + std::to_string(kMapFileVersion));
  // the size is checked before anything is allocated from the header's count
  if (std::fseek(f, 0, SEEK_END) != 0) throw std::runtime_error("read_map_file: cannot seek in " + path);
  const long long size = (long long)std::ftell(f);
  if (nv < 0 || size != (long long)kMapFileHeaderBytes + 96LL * nv) throw std::runtime_error("read_map_file: " + path + " is truncated or corrupt");
  std::fseek(f, (long)kMapFileHeaderBytes, SEEK_SET);
  const size_t n = (size_t)nv;
  m.coords.resize(3 * n); m.sums.resize(10 * n); m.ages.resize(n);
  if (n && (std::fread(m.coords.data(), sizeof(int), 3 * n, f) != 3 * n || std::fread(m.sums.data(), sizeof(double), 10 * n, f) != 10 * n || std::fread(m.ages.data(), sizeof(unsigned), n, f) != n))
    throw std::runtime_error("read_map_file: " + path + " is truncated");
  return m;
}
}  // namespace detail

/// FastVGICPCuda (fast_vgicp_cuda.hpp:24-85, impl/fast_vgicp_cuda_impl.hpp)
template <typename PointSource, typename PointTarget>
class FastVGICPCuda : public DeviceRegistration<fvh_vgicp, PointSource, PointTarget> {
  using Base = DeviceRegistration<fvh_vgicp, PointSource, PointTarget>;
  using Base::call;
  using Base::core_;
  using Base::incremental_target_;
  using Base::input_;
  using Base::scratch_xyz_;
  using Base::target_;

public:
  using PointCloudSource = typename Base::PointCloudSource;
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;

  explicit FastVGICPCuda(int device = 0) : Base(&detail::kVgicpVoxelCalls) {  // fast_vgicp_cuda_impl.hpp:21-32
    detail::check(fvh_vgicp_create(device, &core_), "fvh_vgicp_create", "cannot create the HIP engine (no GPU? there is no CPU fallback)");
    call(fvh_vgicp_set_resolution(core_, voxel_resolution_), "set_resolution");
    call(fvh_vgicp_set_kernel_params(core_, 0.5, 3.0), "set_kernel_params");
  }
  ~FastVGICPCuda() override { if (core_) fvh_vgicp_destroy(core_); }

  void setCorrespondenceRandomness(int) {}  // empty in the reference too (:38): k stays 20
  void setResolution(double resolution) { call(fvh_vgicp_set_resolution(core_, resolution), "set_resolution"); }
  /// FastVGICP::setVoxelAccumulationMode (fast_vgicp_impl.hpp:41-43; CPU class only in the reference -- the CUDA core has the
  /// additive voxel alone): takes effect when the target voxel map is next built (setInputTarget / swapSourceAndTarget)
  void setVoxelAccumulationMode(VoxelAccumulationMode mode) {
    call(fvh_vgicp_set_voxel_accumulation_mode(core_, static_cast<int>(mode)), "set_voxel_accumulation_mode");
    if (this->target_) call(fvh_vgicp_create_target_voxelmap(core_), "create_target_voxelmap");  // (setInputTarget left cloud + covariances on the device)
  }
  void setKernelWidth(double kernel_width, double max_dist = -1.0) {  // :45-51
    if (max_dist <= 0.0) max_dist = kernel_width * 5.0;
    call(fvh_vgicp_set_kernel_params(core_, kernel_width, max_dist), "set_kernel_params");
  }
  void setRegularizationMethod(RegularizationMethod method) { regularization_method_ = method; }
  void setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0) { call(fvh_vgicp_set_neighbor_search_method(core_, (int)method, radius), "set_neighbor_search_method"); }
  void setNearestNeighborSearchMethod(NearestNeighborMethod method) { neighbor_search_method_ = method; }
  /// NearestNeighborMethod::CPU_PARALLEL_KDTREE -- the reference's DEFAULT (fast_vgicp_cuda_impl.hpp:27,152-167) -- asks for EXACT k-NN lists from a
  /// host kd-tree. The engine's device search returns the same lists (fp32 distances, ties to the lower index: equal to the kd-tree's at 17k / 100k /
  /// 1M points, tests/test_gpu_parity*.py, test_neighbor_methods_agree) in 35 us instead of the ~4 ms a host tree + a PCIe round trip of N x k
  /// indices costs per cloud, so by default that enum value is SERVED BY THE DEVICE. setHostKdTree(true) (or FVH_HOST_KDTREE=1 in the
  /// environment) restores the host tree of kdtree.hpp for callers who want the reference's data flow.
  void setHostKdTree(bool on) { host_kdtree_ = on; }
  bool getHostKdTree() const { return host_kdtree_; }
  void setComputePrecision(int fvh_precision) { call(fvh_vgicp_set_precision(core_, fvh_precision), "set_precision"); }

  void swapSourceAndTarget() override {  // :69-72
    call(fvh_vgicp_swap_source_and_target(core_), "swap_source_and_target");
    input_.swap(target_);
  }

  void setInputSource(const PointCloudSourceConstPtr& cloud) override {  // :85-111
    if (!this->take_source(cloud)) return;
    switch (effective_neighbor_method(cloud->size())) {
      case NearestNeighborMethod::CPU_PARALLEL_KDTREE: {
        const std::vector<int> nb = find_neighbors_parallel_kdtree(*cloud);
        call(fvh_vgicp_set_source_neighbors(core_, k_correspondences_, nb.data()), "set_source_neighbors");
        call(fvh_vgicp_calculate_source_covariances(core_, (int)regularization_method_), "calculate_source_covariances");
      } break;
      case NearestNeighborMethod::GPU_BRUTEFORCE:
        call(fvh_vgicp_find_source_neighbors(core_, k_correspondences_), "find_source_neighbors");
        call(fvh_vgicp_calculate_source_covariances(core_, (int)regularization_method_), "calculate_source_covariances");
        break;
      case NearestNeighborMethod::GPU_RBF_KERNEL:
        call(fvh_vgicp_calculate_source_covariances_rbf(core_, (int)regularization_method_), "calculate_source_covariances_rbf");
        break;
    }
  }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // :114-141
    if (cloud == target_) return;
    incremental_target_ = false;  // (create_target_voxelmap below replaces an incremental map by the batch map of this cloud)
    this->take_target(cloud);
    switch (effective_neighbor_method(cloud->size())) {
      case NearestNeighborMethod::CPU_PARALLEL_KDTREE: {
        const std::vector<int> nb = find_neighbors_parallel_kdtree(*cloud);
        call(fvh_vgicp_set_target_neighbors(core_, k_correspondences_, nb.data()), "set_target_neighbors");
        call(fvh_vgicp_calculate_target_covariances(core_, (int)regularization_method_), "calculate_target_covariances");
      } break;
      case NearestNeighborMethod::GPU_BRUTEFORCE:
        call(fvh_vgicp_find_target_neighbors(core_, k_correspondences_), "find_target_neighbors");
        call(fvh_vgicp_calculate_target_covariances(core_, (int)regularization_method_), "calculate_target_covariances");
        break;
      case NearestNeighborMethod::GPU_RBF_KERNEL:
        call(fvh_vgicp_calculate_target_covariances_rbf(core_, (int)regularization_method_), "calculate_target_covariances_rbf");
        break;
    }
    call(fvh_vgicp_create_target_voxelmap(core_), "create_target_voxelmap");
  }

  // ---- incremental target map (no reference counterpart; C ABI: fvh_vgicp_map_begin / _insert_source / _prune). Scan-to-map loops:
  //     beginIncrementalTarget(); setInputSource(scan 0); insertSourceIntoTarget(Identity);
  //     per scan: setInputSource(scan); align(out, guess); insertSourceIntoTarget(); pruneTarget(position, radius);
  // The map has no host cloud behind it: getInputTarget() is null, align() does not ask for one, swapSourceAndTarget() throws
  // (FVH_ERR_BAD_STATE) and getFitnessScore() needs a target cloud as before: targetCloudFromMap() makes one of the map (one point per
  // voxel), after which getFitnessScore() and alignBest() work in this mode. setInputTarget() ends the mode.
  // (the calls themselves: DeviceRegistration, shared with NDTCuda; the source is added with its points + covariances as setInputSource left them)
  using Base::beginIncrementalTarget;
  using Base::insertSourceIntoTarget;
  using Base::pruneTarget;
  using Base::clearTargetAlongRays;
  using Base::scoreTarget;
  using Base::castRays;
  using Base::castRaysToSource;
  using Base::hasIncrementalTarget;
  using Base::targetCloudFromMap;

  // ---- snapshots of the incremental target map (C ABI: fvh_vgicp_voxelmap_export / _import / _merge_from): save, restore, merge.
  // Restore = loadTargetMap(path) on a fresh object, or beginIncrementalTarget() + importTargetMap(). Import and merge ADD: sums and
  // counts add per voxel (exactly: both voxel types are pure sums), ages and the insert count carry over, so pruneTarget(max_age) means on
  // a restored map what it meant on the original.
  using Base::exportTargetMap;
  using Base::importTargetMap;
  /// adds the live incremental target of `other` (same device, resolution and mode) into this one, device to device; `other` is unchanged
  void mergeTargetFrom(FastVGICPCuda& other) { this->merge_target_from(other); }
  int mergeTargetFromPosed(FastVGICPCuda& other, const Isometry3d& T) { return this->merge_target_from_posed(other, T); }
  using Base::transformTargetMap;
  using Base::saveTargetMap;
  /// adds the file's map into the incremental target; an object without one takes the file's resolution and voxel mode and starts one sized for it
  void loadTargetMap(const std::string& path) {
    const TargetMapSnapshot m = detail::read_map_file(path);
    if (!incremental_target_) {
      call(fvh_vgicp_set_resolution(core_, m.resolution), "set_resolution");
      call(fvh_vgicp_set_voxel_accumulation_mode(core_, m.mode == 2 ? 2 : 0), "set_voxel_accumulation_mode");
      beginIncrementalTarget(std::max(m.num_voxels(), 1));
    }
    importTargetMap(m);
  }

  // ---- scan streams as a two-stage pipeline (no reference counterpart; C ABI: fvh_vgicp_align_async / _wait, fvh_vgicp_prepare_source_device /
  // _adopt_prepared_source). kitti.cpp:95-128 with the preparation of scan k+1 hidden under the registration of scan k:
  //     alignAsync(); prepareNextSourceDevice(next scan); alignWait(); swapSourceAndTarget(); adoptPreparedSource();
  // The prepared source lives on the device only: getInputSource() is null for it and alignWait() returns the pose without transforming a host
  // cloud. Neighbours and covariances follow setNearestNeighborSearchMethod (the host kd-tree cannot be served here: device search instead,
  // identical lists) and setRegularizationMethod. `stages`: see fvh_vgicp_prepare_source_device (2: order, neighbours, covariances).
  void prepareNextSourceDevice(const float* d_xyz, int n, int stride_floats = 3, int stages = 2) {
    const int rbf = neighbor_search_method_ == NearestNeighborMethod::GPU_RBF_KERNEL ? 1 : 0;
    prepared_stages_ = stages;
    prepared_cloud_.reset();
    call(fvh_vgicp_prepare_source_device(core_, d_xyz, n, stride_floats, k_correspondences_, (int)regularization_method_, rbf, stages), "prepare_source_device");
  }
  /// the same for a host cloud (consumed before the call returns); adoptPreparedSource() then makes it getInputSource()
  void prepareNextSource(const PointCloudSourceConstPtr& cloud, int stages = 2) {
    const int rbf = neighbor_search_method_ == NearestNeighborMethod::GPU_RBF_KERNEL ? 1 : 0;
    prepared_stages_ = stages;
    const detail::XyzView<PointSource> view(*cloud, scratch_xyz_);
    call(fvh_vgicp_prepare_source(core_, view.data, (int)cloud->size(), view.stride, k_correspondences_, (int)regularization_method_, rbf, stages), "prepare_source");
    prepared_cloud_ = cloud;
  }
  void adoptPreparedSource() {
    call(fvh_vgicp_adopt_prepared_source(core_), "adopt_prepared_source");
    input_ = prepared_cloud_;
    prepared_cloud_.reset();
    if (prepared_stages_ < 2) {
      if (neighbor_search_method_ == NearestNeighborMethod::GPU_RBF_KERNEL) call(fvh_vgicp_calculate_source_covariances_rbf(core_, (int)regularization_method_), "calculate_source_covariances_rbf");
      else call(fvh_vgicp_calculate_source_covariances(core_, (int)regularization_method_), "calculate_source_covariances");
    }
  }
  using Base::alignAsync;
  using Base::alignWait;

protected:
  /// the enum value the switch statements act on: the default one is served by the device search unless the host tree was asked for
  /// (a cloud with fewer points than k keeps the host path: the reference pads those lists with index 0, :155,162)
  NearestNeighborMethod effective_neighbor_method(size_t n_points) const {
    if (neighbor_search_method_ != NearestNeighborMethod::CPU_PARALLEL_KDTREE || host_kdtree_ || n_points < (size_t)k_correspondences_) return neighbor_search_method_;
    return NearestNeighborMethod::GPU_BRUTEFORCE;
  }
  static bool host_kdtree_default() {
    static const bool on = [] { const char* v = std::getenv("FVH_HOST_KDTREE"); return v && std::atoi(v) != 0; }();
    return on;
  }
  /// find_neighbors_parallel_kdtree (:152-167): host kd-tree + OpenMP (hundreds of threads on a 17k-point loop only add contention)
  template <typename CloudT>
  std::vector<int> find_neighbors_parallel_kdtree(const CloudT& cloud) const {
    return detail::host_kdtree_neighbors(cloud, k_correspondences_, host::omp_threads_for((int)cloud.size()));
  }

private:
  int k_correspondences_ = 20;                                                                   // :24
  double voxel_resolution_ = 1.0;                                                                // :25
  RegularizationMethod regularization_method_ = RegularizationMethod::PLANE;                     // :26
  NearestNeighborMethod neighbor_search_method_ = NearestNeighborMethod::CPU_PARALLEL_KDTREE;    // :27
  bool host_kdtree_ = host_kdtree_default();                                                     // setHostKdTree
  int prepared_stages_ = 2;                                                                         // prepareNextSourceDevice
  PointCloudSourceConstPtr prepared_cloud_;                                                         // prepareNextSource (host cloud): becomes input_ on adoption
};

/// FastGICP (gicp/fast_gicp.hpp:24-98, impl/fast_gicp_impl.hpp) on the HIP engine: the reference class is CPU/OpenMP only;
/// here the covariances (exact k-NN + regularisation), the nearest-target-point correspondences and the cost sums run on
/// the device; the LM recursion runs on the device too (setUseDeviceLM(false): the reference's host loop, LsqRegistration::step_lm).
template <typename PointSource, typename PointTarget>
class FastGICP : public DeviceRegistration<fvh_vgicp, PointSource, PointTarget> {
  using Base = DeviceRegistration<fvh_vgicp, PointSource, PointTarget>;

protected:
  using Base::call;
  using Base::core_;
  using Base::input_;
  using Base::target_;

public:
  using PointCloudSource = typename Base::PointCloudSource;
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;

  explicit FastGICP(int device = 0) : Base(&detail::kVgicpNearestPointCalls) {  // fast_gicp_impl.hpp:9-23
    detail::check(fvh_vgicp_create(device, &core_), "fvh_vgicp_create", "cannot create the HIP engine (no GPU? there is no CPU fallback)");
  }
  ~FastGICP() override { if (core_) fvh_vgicp_destroy(core_); }

  void setNumThreads(int) {}  // :29-38: OpenMP threads of the CPU class; the device needs none
  void setCorrespondenceRandomness(int k) { k_correspondences_ = k; }  // :41-43
  void setRegularizationMethod(RegularizationMethod method) { regularization_method_ = method; }  // :46-48
  void setMaxCorrespondenceDistance(double d) { call(fvh_vgicp_gicp_set_max_correspondence_distance(core_, d), "gicp_set_max_correspondence_distance"); }  // pcl::Registration

  void swapSourceAndTarget() override {  // :51-62
    call(fvh_vgicp_gicp_swap_source_and_target(core_), "gicp_swap_source_and_target");
    input_.swap(target_);
  }

  void setInputSource(const PointCloudSourceConstPtr& cloud) override {  // :77-85 (covariances: :103-112, computed eagerly here)
    if (this->take_source(cloud)) estimate_covariances(*cloud, true);
  }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // :88-95
    if (this->take_target(cloud)) estimate_covariances(*cloud, false);
  }
  /// gicp/fast_gicp.hpp:60-70: covariances computed elsewhere / read back. The reference carries them as 4x4 doubles with a
  /// zero last row and column; here a covariance is its 3x3 block, 9 doubles per point (symmetric, so any major).
  using Covariances = std::vector<std::array<double, 9>>;
  void setSourceCovariances(const Covariances& covs) {
    if (!input_ || covs.size() != input_->size()) throw std::invalid_argument("setSourceCovariances: one covariance per source point, after setInputSource");
    call(fvh_vgicp_set_source_covariances(core_, covs.empty() ? nullptr : covs[0].data()), "set_source_covariances");
  }
  virtual void setTargetCovariances(const Covariances& covs) {  // (virtual: FastVGICP's target voxel map is made of them)
    if (!target_ || covs.size() != target_->size()) throw std::invalid_argument("setTargetCovariances: one covariance per target point, after setInputTarget");
    call(fvh_vgicp_set_target_covariances(core_, covs.empty() ? nullptr : covs[0].data()), "set_target_covariances");
  }
  Covariances getSourceCovariances() const { return get_covariances(input_ ? input_->size() : 0, true); }
  Covariances getTargetCovariances() const { return get_covariances(target_ ? target_->size() : 0, false); }

protected:
  Covariances get_covariances(size_t n, bool source) const {
    std::vector<float> f(9 * n);
    if (n) call(source ? fvh_vgicp_get_source_covariances(core_, f.data()) : fvh_vgicp_get_target_covariances(core_, f.data()), "get_covariances");
    Covariances out(n);
    for (size_t i = 0; i < n; i++) for (int j = 0; j < 9; j++) out[i][j] = f[9 * i + j];
    return out;
  }
  /// calculate_covariances (fast_gicp_impl.hpp:244-301): k nearest neighbours of every point + regularisation. The device's exact
  /// search serves k <= 64 on clouds of at least k points; what the reference's kd-tree also accepts -- larger k, or fewer points than
  /// k (nearestKSearch then returns them all; the unfilled entries of its index vector stay 0) -- goes through the host kd-tree.
  template <typename CloudT>
  void estimate_covariances(const CloudT& cloud, bool source) {
    const int n = (int)cloud.size(), k = k_correspondences_;
    if (k < 1) throw std::invalid_argument("setCorrespondenceRandomness: k must be >= 1");
    if (n == 0) return;
    if (k <= 64 && n >= k) {
      call(source ? fvh_vgicp_find_source_neighbors(core_, k) : fvh_vgicp_find_target_neighbors(core_, k), "find_neighbors");
    } else {
      if (k > 64) throw std::invalid_argument("setCorrespondenceRandomness: more than 64 neighbours per point are not supported by the covariance kernel");
      const std::vector<int> nb = detail::host_kdtree_neighbors(cloud, k, 1);
      call(source ? fvh_vgicp_set_source_neighbors(core_, k, nb.data()) : fvh_vgicp_set_target_neighbors(core_, k, nb.data()), "set_neighbors");
    }
    call(source ? fvh_vgicp_calculate_source_covariances(core_, (int)regularization_method_) : fvh_vgicp_calculate_target_covariances(core_, (int)regularization_method_), "calculate_covariances");
  }

protected:
  int k_correspondences_ = 20;                                                // :17
  RegularizationMethod regularization_method_ = RegularizationMethod::PLANE;  // :21
};

/// FastVGICP -- the reference's CPU / OpenMP class (gicp/fast_vgicp.hpp:28-78, impl/fast_vgicp_impl.hpp) -- served by the same HIP
/// engine in its fp64 arithmetic. As in the reference it EXTENDS FastGICP (fast_vgicp.hpp:28): the cloud / covariance side --
/// `setCorrespondenceRandomness(k)` honoured (FastGICP::k_correspondences_, fast_gicp_impl.hpp:41-43,253-265; the CUDA class ignores
/// it, fast_vgicp_cuda_impl.hpp:38), covariances from EXACT k nearest neighbours (the reference's kd-tree; here the device's exact
/// search: identical lists), `setNumThreads` (a no-op: there is no OpenMP team to size), the covariance accessors -- is FastGICP's;
/// what it replaces is the correspondence model: voxels of the target instead of its nearest points (fast_vgicp_impl.hpp:73-204).
/// The neighbour search takes no radius (DIRECT1 / 7 / 27 only, fast_vgicp_voxel.hpp:16-43).
template <typename PointSource, typename PointTarget>
class FastVGICP : public FastGICP<PointSource, PointTarget> {
  using Base = FastGICP<PointSource, PointTarget>;
  using Base::core_;
  using Base::input_;
  using Base::target_;

public:
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
  using Base::scoreTarget;  // (this class owns a voxel map; FastGICP does not)
  using Base::castRays;
  using Base::castRaysToSource;

  explicit FastVGICP(int device = 0) : Base(device) {  // fast_vgicp_impl.hpp:19-25
    this->calls_ = &detail::kVgicpVoxelCalls;  // what it replaces in FastGICP: voxel correspondences, and the calls only they have
    this->call(fvh_vgicp_set_resolution(core_, 1.0), "set_resolution");
    this->call(fvh_vgicp_set_neighbor_search_method(core_, (int)NeighborSearchMethod::DIRECT1, -1.0), "set_neighbor_search_method");
  }
  // The reference builds the voxel map lazily, inside the first linearisation of every align (fast_vgicp_impl.hpp:120-123), from
  // whatever resolution and target covariances are current then; this class builds it eagerly -- so every setter the map depends on
  // rebuilds it when a target is set (setResolution, setTargetCovariances, setVoxelAccumulationMode).
  void setResolution(double resolution) {  // :36-38
    this->call(fvh_vgicp_set_resolution(core_, resolution), "set_resolution");
    if (target_) this->call(fvh_vgicp_create_target_voxelmap(core_), "create_target_voxelmap");
  }
  void setTargetCovariances(const typename Base::Covariances& covs) override {  // gicp/fast_gicp.hpp:66-68, consumed by :129-156 of the impl
    Base::setTargetCovariances(covs);
    this->call(fvh_vgicp_create_target_voxelmap(core_), "create_target_voxelmap");
  }
  void setNeighborSearchMethod(NeighborSearchMethod method) {  // :46-48
    if (method == NeighborSearchMethod::DIRECT_RADIUS) detail::check(FVH_ERR_INVALID_ARGUMENT, "setNeighborSearchMethod", "FastVGICP has no DIRECT_RADIUS (fast_vgicp_voxel.hpp:16-43): use FastVGICPCuda");
    this->call(fvh_vgicp_set_neighbor_search_method(core_, (int)method, -1.0), "set_neighbor_search_method");
  }
  void setVoxelAccumulationMode(VoxelAccumulationMode mode) {  // :41-43; takes effect when the target voxel map is next built
    this->call(fvh_vgicp_set_voxel_accumulation_mode(core_, static_cast<int>(mode)), "set_voxel_accumulation_mode");
    if (target_) this->call(fvh_vgicp_create_target_voxelmap(core_), "create_target_voxelmap");
  }
  void setMaxCorrespondenceDistance(double) {}  // inherited from pcl::Registration; FastVGICP never reads it (voxel correspondences)

  void swapSourceAndTarget() override {  // fast_vgicp_impl.hpp:46-53: swaps clouds and covariances, drops the voxel map (rebuilt here, not lazily)
    this->call(fvh_vgicp_swap_source_and_target(core_), "swap_source_and_target");
    input_.swap(target_);
  }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // :56-63
    if (cloud == target_) return;
    Base::setInputTarget(cloud);
    this->call(fvh_vgicp_create_target_voxelmap(core_), "create_target_voxelmap");
  }
};

/// NDTCuda (ndt_cuda.hpp:23-69, impl/ndt_cuda_impl.hpp)
template <typename PointSource, typename PointTarget>
class NDTCuda : public DeviceRegistration<fvh_ndt, PointSource, PointTarget> {
  using Base = DeviceRegistration<fvh_ndt, PointSource, PointTarget>;
  using Base::call;
  using Base::core_;
  using Base::incremental_target_;
  using Base::input_;
  using Base::scratch_xyz_;
  using Base::target_;

public:
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;

  explicit NDTCuda(int device = 0) : Base(&detail::kNdtCalls) { detail::check(fvh_ndt_create(device, &core_), "fvh_ndt_create", "cannot create the HIP engine (no GPU? there is no CPU fallback)"); }
  ~NDTCuda() override { if (core_) fvh_ndt_destroy(core_); }

  void setDistanceMode(NDTDistanceMode mode) { call(fvh_ndt_set_distance_mode(core_, (int)mode), "set_distance_mode"); }
  void setResolution(double resolution) { call(fvh_ndt_set_resolution(core_, resolution), "set_resolution"); }
  void setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0) { call(fvh_ndt_set_neighbor_search_method(core_, (int)method, radius), "set_neighbor_search_method"); }

  void swapSourceAndTarget() override { call(fvh_ndt_swap_source_and_target(core_), "swap_source_and_target"); input_.swap(target_); }
  void setInputSource(const PointCloudSourceConstPtr& cloud) override { this->take_source(cloud); }  // ndt_cuda_impl.hpp:52-60
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // :63-73
    if (this->take_target(cloud)) incremental_target_ = false;  // (the next align builds the batch map of this cloud: an incremental target ends)
  }

  // ---- incremental target map (no reference counterpart; C ABI: fvh_ndt_map_begin / _insert_source / _prune, fvh_ndt_voxelmap_*), the calls
  // FastVGICPCuda has for its own, for scan-to-map localisation:
  //     beginIncrementalTarget(); setInputSource(scan 0); insertSourceIntoTarget(Identity);
  //     per scan: setInputSource(scan); align(out, guess); insertSourceIntoTarget(); pruneTarget(position, radius);
  // The voxels are sums of the inserted POINTS (sum p, sum p p^T): the map is the one setInputTarget(all inserted points) would give. It has no
  // host cloud behind it: getInputTarget() is null, align() does not ask for one, swapSourceAndTarget() throws (FVH_ERR_BAD_STATE) and
  // getFitnessScore() needs a target cloud as before: targetCloudFromMap() makes one of the map (one point per voxel), after which
  // getFitnessScore() and alignBest() work in this mode. setInputTarget() ends the mode. Snapshots carry mode 3 (FVH_VOXEL_NDT_SUMS).
  using Base::beginIncrementalTarget;
  using Base::insertSourceIntoTarget;
  using Base::pruneTarget;
  using Base::clearTargetAlongRays;
  using Base::scoreTarget;
  using Base::castRays;
  using Base::castRaysToSource;
  using Base::hasIncrementalTarget;
  using Base::targetCloudFromMap;
  using Base::exportTargetMap;
  using Base::importTargetMap;
  void mergeTargetFrom(NDTCuda& other) { this->merge_target_from(other); }
  int mergeTargetFromPosed(NDTCuda& other, const Isometry3d& T) { return this->merge_target_from_posed(other, T); }
  using Base::transformTargetMap;
  using Base::saveTargetMap;
  /// adds the file's map into the incremental target; an object without one takes the file's resolution and starts one sized for it
  void loadTargetMap(const std::string& path) {
    const TargetMapSnapshot m = detail::read_map_file(path);
    if (!incremental_target_) {
      call(fvh_ndt_set_resolution(core_, m.resolution), "set_resolution");
      beginIncrementalTarget(std::max(m.num_voxels(), 1));
    }
    importTargetMap(m);
  }

  // ---- frame streams as a two-stage pipeline (no reference counterpart; C ABI: fvh_ndt_align_async / _wait, fvh_ndt_prepare_source_device /
  // _adopt_prepared_source). kitti.cpp:95-128 with the preparation of frame k+1 hidden under the registration of frame k:
  //     adoptPreparedSource(); alignAsync(); [filter frame k+1 on the prepare stream; prepareNextSourceDevice()]; alignWait(); swapSourceAndTarget();
  // The prepared source lives on the device only: getInputSource() is null for it and alignWait() returns the pose without
  // transforming a host cloud. Same kernels on the same data as the sequential calls: same registration.
  void prepareNextSourceDevice(const float* d_xyz, int n, int stride_floats = 3) { prepared_cloud_.reset(); call(fvh_ndt_prepare_source_device(core_, d_xyz, n, stride_floats), "prepare_source_device"); }
  /// the output of the filter's last ApproximateVoxelGrid call becomes the prepared source without a copy (fvh_ndt_prepare_source_from_voxelgrid)
  void prepareNextSourceFromFilter(fvh_voxelgrid* filter) { prepared_cloud_.reset(); call(fvh_ndt_prepare_source_from_voxelgrid(core_, filter), "prepare_source_from_voxelgrid"); }
  /// the same for a host cloud (consumed before the call returns); adoptPreparedSource() then makes it getInputSource()
  void prepareNextSource(const PointCloudSourceConstPtr& cloud) {
    const detail::XyzView<PointSource> view(*cloud, scratch_xyz_);
    call(fvh_ndt_prepare_source(core_, view.data, (int)cloud->size(), view.stride), "prepare_source");
    prepared_cloud_ = cloud;
  }
  void adoptPreparedSource() { call(fvh_ndt_adopt_prepared_source(core_), "adopt_prepared_source"); input_ = prepared_cloud_; prepared_cloud_.reset(); }
  using Base::alignAsync;  // (not preceded by create_voxelmaps, unlike align and alignMulti below)
  using Base::alignWait;

protected:
  void computeTransformation(typename Base::PointCloudSource& output, const Matrix4f& guess) override {  // :76-79
    call(fvh_ndt_create_voxelmaps(core_), "create_voxelmaps");
    Base::computeTransformation(output, guess);
  }
  void device_align_multi(int k, const double* guesses16, const fvh_lm_params* p, fvh_lm_result* results, int* grid_blocks) override {
    call(fvh_ndt_create_voxelmaps(core_), "create_voxelmaps");
    Base::device_align_multi(k, guesses16, p, results, grid_blocks);
  }

private:
  PointCloudSourceConstPtr prepared_cloud_;  // prepareNextSource (host cloud): becomes input_ on adoption
};

}  // namespace fast_gicp
