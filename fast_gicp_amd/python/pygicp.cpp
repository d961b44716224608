// pygicp -- Python bindings with the surface of the reference's src/python/main.cpp:152-223, on the
// host-side C++ mirror (include/fast_gicp_amd/registration.hpp) -> C ABI -> HIP engine.
// Eigen is not available here, so Nx3 / 4x4 arguments are numpy arrays (same shapes and dtypes the
// reference's pybind11/eigen.h conversions accept and return).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <iostream>

#include "fast_gicp_amd/registration.hpp"
#include "fast_gicp_amd/voxelgrid.hpp"

namespace py = pybind11;
using namespace fast_gicp;

using Cloud = PointCloud<PointXYZ>;
using Lsq = LsqRegistration<PointXYZ, PointXYZ>;
using VGICPCuda = FastVGICPCuda<PointXYZ, PointXYZ>;
using VGICP = FastVGICP<PointXYZ, PointXYZ>;
using GICP = FastGICP<PointXYZ, PointXYZ>;
using NDT = NDTCuda<PointXYZ, PointXYZ>;
struct NDTMap : NDT { using NDT::NDT; };  // the C++ class again, bound as its own Python class (NDTCudaMap)
using Points = py::array_t<double, py::array::c_style | py::array::forcecast>;
using Mat4 = py::array_t<double, py::array::c_style | py::array::forcecast>;

static NeighborSearchMethod search_method(const std::string& s) {  // main.cpp:21-34
  if (s == "DIRECT1") return NeighborSearchMethod::DIRECT1;
  if (s == "DIRECT7") return NeighborSearchMethod::DIRECT7;
  if (s == "DIRECT27") return NeighborSearchMethod::DIRECT27;
  if (s == "DIRECT_RADIUS") return NeighborSearchMethod::DIRECT_RADIUS;
  std::cerr << "error: unknown neighbor search method " << s << std::endl;
  return NeighborSearchMethod::DIRECT1;
}
static RegularizationMethod regularization_method(const std::string& s) {
  if (s == "NONE") return RegularizationMethod::NONE;
  if (s == "MIN_EIG") return RegularizationMethod::MIN_EIG;
  if (s == "NORMALIZED_MIN_EIG") return RegularizationMethod::NORMALIZED_MIN_EIG;
  if (s == "PLANE") return RegularizationMethod::PLANE;
  if (s == "FROBENIUS") return RegularizationMethod::FROBENIUS;
  throw std::invalid_argument("unknown regularization method " + s);
}
static VoxelAccumulationMode voxel_accumulation_mode(const std::string& s) {  // FastVGICP::setVoxelAccumulationMode (fast_vgicp_impl.hpp:41-43)
  if (s == "ADDITIVE") return VoxelAccumulationMode::ADDITIVE;
  if (s == "ADDITIVE_WEIGHTED") return VoxelAccumulationMode::ADDITIVE_WEIGHTED;
  if (s == "MULTIPLICATIVE") return VoxelAccumulationMode::MULTIPLICATIVE;
  throw std::invalid_argument("unknown voxel accumulation mode: " + s);
}
static NearestNeighborMethod nn_method(const std::string& s) {
  if (s == "CPU_PARALLEL_KDTREE") return NearestNeighborMethod::CPU_PARALLEL_KDTREE;
  if (s == "GPU_BRUTEFORCE") return NearestNeighborMethod::GPU_BRUTEFORCE;
  if (s == "GPU_RBF_KERNEL") return NearestNeighborMethod::GPU_RBF_KERNEL;
  throw std::invalid_argument("unknown nearest neighbor method " + s);
}

static Cloud::Ptr numpy2cloud(const Points& pts) {  // eigen2pcl, main.cpp:36-44
  if (pts.ndim() != 2 || pts.shape(1) != 3) throw std::invalid_argument("points must be an (N, 3) array");
  auto cloud = std::make_shared<Cloud>();
  cloud->resize(pts.shape(0));
  auto r = pts.unchecked<2>();
  for (py::ssize_t i = 0; i < pts.shape(0); i++) {
    cloud->points[i].x = (float)r(i, 0); cloud->points[i].y = (float)r(i, 1); cloud->points[i].z = (float)r(i, 2);
  }
  return cloud;
}
static py::array_t<double> cloud2numpy(const Cloud& c) {
  py::array_t<double> out({(py::ssize_t)c.size(), (py::ssize_t)3});
  auto w = out.mutable_unchecked<2>();
  for (size_t i = 0; i < c.size(); i++) { w(i, 0) = c.points[i].x; w(i, 1) = c.points[i].y; w(i, 2) = c.points[i].z; }
  return out;
}
static Matrix4f numpy2mat4(const Mat4& m) {
  if (m.ndim() != 2 || m.shape(0) != 4 || m.shape(1) != 4) throw std::invalid_argument("pose must be a (4, 4) array");
  Matrix4f M;
  auto r = m.unchecked<2>();
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) M(i, j) = (float)r(i, j);
  return M;
}
static fast_gicp::Isometry3d numpy2iso(const Mat4& m) {  // a pose kept in double (the upper three rows: a rigid pose's last row is (0, 0, 0, 1))
  if (m.ndim() != 2 || m.shape(0) != 4 || m.shape(1) != 4) throw std::invalid_argument("pose must be a (4, 4) array");
  fast_gicp::Matrix4d M;
  auto r = m.unchecked<2>();
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) M(i, j) = r(i, j);
  return fast_gicp::Isometry3d::from(M);
}
static std::vector<Matrix4f> numpy2mat4s(const Mat4& m) {  // (K, 4, 4) -> K poses
  if (m.ndim() != 3 || m.shape(1) != 4 || m.shape(2) != 4) throw std::invalid_argument("poses must be a (K, 4, 4) array");
  std::vector<Matrix4f> out((size_t)m.shape(0));
  auto r = m.unchecked<3>();
  for (py::ssize_t k = 0; k < m.shape(0); k++) for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) out[k](i, j) = (float)r(k, i, j);
  return out;
}
template <typename T = float>  // (the class methods return float32 like the reference's Matrix4f, align_points float64)
static py::array_t<T> mat4_to_numpy(const Matrix4f& M) {
  py::array_t<T> out({4, 4});
  auto w = out.template mutable_unchecked<2>();
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) w(i, j) = M(i, j);
  return out;
}
static py::array_t<double> identity4() {
  py::array_t<double> I({4, 4});
  auto w = I.mutable_unchecked<2>();
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) w(i, j) = i == j ? 1.0 : 0.0;
  return I;
}

static py::array_t<double> downsample(const Points& points, double resolution) {  // main.cpp:46-62
  Cloud filtered;
  approximate_voxel_grid(*numpy2cloud(points), (float)resolution, filtered);
  return cloud2numpy(filtered);
}

// A filter handle for the length of one binding call: destroyed with the scope; check() throws with the handle's last error
struct TempVoxelGrid {
  fvh_voxelgrid* vg = nullptr;
  explicit TempVoxelGrid(int device) { detail::check(fvh_voxelgrid_create(device, &vg), "fvh_voxelgrid_create", "cannot create the HIP engine (no GPU? there is no CPU fallback)"); }
  ~TempVoxelGrid() { fvh_voxelgrid_destroy(vg); }
  TempVoxelGrid(const TempVoxelGrid&) = delete;
  TempVoxelGrid& operator=(const TempVoxelGrid&) = delete;
  operator fvh_voxelgrid*() const { return vg; }
  void check(int rc, const char* what) const { if (rc) detail::check(rc, what, fvh_voxelgrid_last_error(vg)); }
};

// The n points of the handle's last call as an (n, 3) float64 array (fvh_voxelgrid_get_points); a refused call (rc) throws as `what`
static py::array_t<double> filtered_points(const TempVoxelGrid& vg, int rc, int n, const char* what) {
  std::vector<float> out((size_t)3 * n);
  if (!rc) rc = fvh_voxelgrid_get_points(vg, out.data());
  vg.check(rc, what);
  py::array_t<double> res({(py::ssize_t)n, (py::ssize_t)3});
  auto w = res.mutable_unchecked<2>();
  for (int i = 0; i < n; i++) for (int a = 0; a < 3; a++) w(i, a) = out[3 * (size_t)i + a];
  return res;
}

// ... optionally with their indices into the input (fvh_voxelgrid_get_kept_indices)
static py::object filtered_result(const TempVoxelGrid& vg, int rc, int n, bool return_indices, const char* what) {
  py::array_t<double> res = filtered_points(vg, rc, n, what);
  if (!return_indices) return std::move(res);
  py::array_t<int> ids((py::ssize_t)n);
  vg.check(fvh_voxelgrid_get_kept_indices(vg, ids.mutable_data()), what);
  return py::make_tuple(res, ids);
}

// downsample on the device: the same filter (pcl::ApproximateVoxelGrid semantics, or pcl::VoxelGrid with exact=True), bit-identical
// output in the same order, computed by fvh_voxelgrid_* (kernels_downsample.hpp)
static py::array_t<double> downsample_device(const Points& points, double resolution, bool exact, int device) {
  auto cloud = numpy2cloud(points);
  const std::vector<float> xyz = detail::pack_xyz(*cloud);
  TempVoxelGrid vg(device);
  int n = 0;
  const int rc = fvh_voxelgrid_filter(vg, exact ? FVH_VOXELGRID_EXACT : FVH_VOXELGRID_APPROXIMATE, xyz.data(), (int)cloud->size(), (float)resolution, &n);
  return filtered_points(vg, rc, n, "fvh_voxelgrid_filter");
}

// the origin / range filter of the reference's callers (src/align.cpp:127-133) on the device: fvh_voxelgrid_crop_range
static py::object crop_range_device(const Points& points, double min_sq_norm, double max_sq_norm, bool return_indices, int device) {
  auto cloud = numpy2cloud(points);
  const std::vector<float> xyz = detail::pack_xyz(*cloud);
  TempVoxelGrid vg(device);
  int n = 0;
  const int rc = fvh_voxelgrid_crop_range(vg, xyz.data(), (int)cloud->size(), min_sq_norm, max_sq_norm, &n);
  return filtered_result(vg, rc, n, return_indices, "fvh_voxelgrid_crop_range");
}

// statistical / radius outlier removal on the device (fvh_voxelgrid_remove_statistical_outliers / _remove_radius_outliers)
static py::object remove_outliers_device(const Points& points, const std::string& method, int mean_k, double stddev_mul, double radius, int min_neighbors, bool return_indices,
                                         int device) {
  if (method != "STATISTICAL" && method != "RADIUS") throw std::invalid_argument("unknown outlier removal method " + method + " (STATISTICAL, RADIUS)");
  auto cloud = numpy2cloud(points);
  const std::vector<float> xyz = detail::pack_xyz(*cloud);
  TempVoxelGrid vg(device);
  int n = 0;
  const bool stat = method == "STATISTICAL";
  const int rc = stat ? fvh_voxelgrid_remove_statistical_outliers(vg, xyz.data(), (int)cloud->size(), mean_k, stddev_mul, &n)
                      : fvh_voxelgrid_remove_radius_outliers(vg, xyz.data(), (int)cloud->size(), radius, min_neighbors, &n);
  return filtered_result(vg, rc, n, return_indices, stat ? "fvh_voxelgrid_remove_statistical_outliers" : "fvh_voxelgrid_remove_radius_outliers");
}

// Euclidean cluster extraction on the device (fvh_voxelgrid_cluster_euclidean): (labels int32[n], cluster number per input point or -1;
// sizes int32[num_clusters]); clusters are numbered by their smallest input index
static py::tuple cluster_euclidean_device(const Points& points, double tolerance, int min_cluster_size, int max_cluster_size, int device) {
  auto cloud = numpy2cloud(points);
  const std::vector<float> xyz = detail::pack_xyz(*cloud);
  TempVoxelGrid vg(device);
  int n = 0, nc = 0;
  vg.check(fvh_voxelgrid_cluster_euclidean(vg, xyz.data(), (int)cloud->size(), tolerance, min_cluster_size, max_cluster_size, &nc, &n), "fvh_voxelgrid_cluster_euclidean");
  py::array_t<int> labels((py::ssize_t)cloud->size()), sizes((py::ssize_t)nc);
  vg.check(fvh_voxelgrid_get_cluster_labels(vg, labels.mutable_data(), sizes.mutable_data()), "fvh_voxelgrid_cluster_euclidean");
  return py::make_tuple(labels, sizes);
}

// RANSAC plane segmentation on the device (fvh_voxelgrid_segment_plane): (coefficients float64[4]: unit normal and d >= 0; int32 indices
// of the kept points in input order: the plane's inliers, or with keep_outliers everything else)
static py::tuple segment_plane_device(const Points& points, double distance_threshold, int max_iterations, unsigned long long seed, const py::object& axis, double eps_angle,
                                      bool keep_outliers, bool refine, int device) {
  auto cloud = numpy2cloud(points);
  const std::vector<float> xyz = detail::pack_xyz(*cloud);
  std::vector<double> ax;
  if (!axis.is_none()) {
    ax = axis.cast<std::vector<double>>();
    if (ax.size() != 3) throw std::invalid_argument("segment_plane_device: axis must have 3 components");
  }
  TempVoxelGrid vg(device);
  int n = 0, inliers = 0;
  py::array_t<double> co((py::ssize_t)4);
  vg.check(fvh_voxelgrid_segment_plane(vg, xyz.data(), (int)cloud->size(), distance_threshold, max_iterations, seed, ax.empty() ? nullptr : ax.data(), eps_angle,
                                       (keep_outliers ? FVH_PLANE_KEEP_OUTLIERS : 0) | (refine ? FVH_PLANE_REFINE : 0), co.mutable_data(), &inliers, &n),
           "fvh_voxelgrid_segment_plane");
  py::array_t<int> ids((py::ssize_t)n);
  vg.check(fvh_voxelgrid_get_kept_indices(vg, ids.mutable_data()), "fvh_voxelgrid_segment_plane");
  return py::make_tuple(co, ids);
}

// motion compensation of a sweep on the device (fvh_voxelgrid_deskew): every point into the sensor frame of t_ref along the trajectory
// through the knot poses ((K, 4, 4), sensor-at-that-instant -> one fixed frame); (n, 3) out, input order
static py::array_t<double> deskew_device(const Points& points, const py::array_t<double, py::array::c_style | py::array::forcecast>& times,
                                         const py::array_t<double, py::array::c_style | py::array::forcecast>& knot_times, const Mat4& knot_poses, const py::object& t_ref, int device) {
  auto cloud = numpy2cloud(points);
  const std::vector<float> xyz = detail::pack_xyz(*cloud);
  if (times.ndim() != 1 || (size_t)times.shape(0) != cloud->size()) throw std::invalid_argument("times must be an (N,) array, one per point");
  if (knot_times.ndim() != 1) throw std::invalid_argument("knot_times must be a (K,) array");
  if (knot_poses.ndim() != 3 || knot_poses.shape(0) != knot_times.shape(0) || knot_poses.shape(1) != 4 || knot_poses.shape(2) != 4) throw std::invalid_argument("knot_poses must be a (K, 4, 4) array");
  const int K = (int)knot_times.shape(0);
  if (K < 1) throw std::invalid_argument("no knots");
  std::vector<float> t(cloud->size());
  for (size_t i = 0; i < t.size(); i++) t[i] = (float)times.data()[i];
  std::vector<double> poses((size_t)16 * K);  // column-major, as the ABI takes them
  auto r = knot_poses.unchecked<3>();
  for (int k = 0; k < K; k++) for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) poses[(size_t)16 * k + j * 4 + i] = r(k, i, j);
  const double ref = t_ref.is_none() ? knot_times.data()[K - 1] : t_ref.cast<double>();
  TempVoxelGrid vg(device);
  int n = 0;
  const int rc = fvh_voxelgrid_deskew(vg, xyz.data(), (int)cloud->size(), t.data(), 1, knot_times.data(), poses.data(), K, ref, &n);
  return filtered_points(vg, rc, n, "fvh_voxelgrid_deskew");
}

// align_points, main.cpp:64-150. "VGICP" (the CPU FastVGICP in the reference, main.cpp:102-108) runs on the same GPU engine in
// its fp64 arithmetic WITH k_correspondences honoured (class FastVGICP of registration.hpp; "VGICP_CUDA" ignores it like the
// reference's FastVGICPCuda: k = 20); "GICP" (nearest-point correspondences, no voxels) runs on the device too.
static py::array_t<double> align_points(const Points& target, const Points& source, const std::string& method, double downsample_resolution, int k_correspondences,
                                        double max_correspondence_distance, double voxel_resolution, int /*num_threads*/, const std::string& neighbor_search_method,
                                        double neighbor_search_radius, const Mat4& initial_guess) {
  Cloud::Ptr target_cloud = numpy2cloud(target), source_cloud = numpy2cloud(source);
  if (downsample_resolution > 0.0) {
    auto ft = std::make_shared<Cloud>(), fs = std::make_shared<Cloud>();
    approximate_voxel_grid(*target_cloud, (float)downsample_resolution, *ft);
    approximate_voxel_grid(*source_cloud, (float)downsample_resolution, *fs);
    target_cloud = ft; source_cloud = fs;
  }
  std::shared_ptr<Lsq> reg;
  if (method == "VGICP") {  // main.cpp:102-108
    auto vgicp = std::make_shared<VGICP>();
    vgicp->setCorrespondenceRandomness(k_correspondences);
    vgicp->setResolution(voxel_resolution);
    if (search_method(neighbor_search_method) == fast_gicp::NeighborSearchMethod::DIRECT_RADIUS) {
      std::cerr << "error: FastVGICP has no DIRECT_RADIUS neighbor search (use VGICP_CUDA)" << std::endl;
      return identity4();
    }
    vgicp->setNeighborSearchMethod(search_method(neighbor_search_method));
    vgicp->setNumThreads(0);
    reg = vgicp;
  } else if (method == "VGICP_CUDA") {
    auto vgicp = std::make_shared<VGICPCuda>();
    vgicp->setCorrespondenceRandomness(k_correspondences);  // a no-op, as in the reference (k = 20)
    vgicp->setNeighborSearchMethod(search_method(neighbor_search_method), neighbor_search_radius);
    vgicp->setResolution(voxel_resolution);
    reg = vgicp;
  } else if (method == "NDT_CUDA") {
    auto ndt = std::make_shared<NDT>();
    ndt->setResolution(voxel_resolution);
    ndt->setNeighborSearchMethod(search_method(neighbor_search_method), neighbor_search_radius);
    reg = ndt;
  } else if (method == "GICP") {  // main.cpp:96-101
    auto gicp = std::make_shared<GICP>();
    gicp->setMaxCorrespondenceDistance(max_correspondence_distance);
    gicp->setCorrespondenceRandomness(k_correspondences);
    reg = gicp;
  } else {
    std::cerr << "error: registration method " << method << " is not provided by the MI355X engine (GICP, VGICP, VGICP_CUDA, NDT_CUDA)" << std::endl;
    return identity4();
  }
  reg->setInputTarget(target_cloud);
  reg->setInputSource(source_cloud);
  Cloud aligned;
  reg->align(aligned, numpy2mat4(initial_guess));
  return mat4_to_numpy<double>(reg->getFinalTransformation());
}

static py::array_t<double> covs_to_numpy(const GICP::Covariances& covs) {
  py::array_t<double> out({(py::ssize_t)covs.size(), (py::ssize_t)3, (py::ssize_t)3});
  double* o = out.mutable_data();
  for (size_t i = 0; i < covs.size(); i++) std::memcpy(o + 9 * i, covs[i].data(), 9 * sizeof(double));
  return out;
}
static GICP::Covariances numpy_to_covs(const py::array_t<double, py::array::c_style | py::array::forcecast>& c) {
  if (c.ndim() != 3 || c.shape(1) != 3 || c.shape(2) != 3) throw std::invalid_argument("covariances must be an (N, 3, 3) array");
  GICP::Covariances covs((size_t)c.shape(0));
  for (size_t i = 0; i < covs.size(); i++) std::memcpy(covs[i].data(), c.data() + 9 * i, 9 * sizeof(double));
  return covs;
}

// not in the reference: an incremental target map for scan-to-map loops, the same methods on FastVGICPCuda and NDTCudaMap
// (include/fast_vgicp_hip.h: fvh_vgicp_map_begin ... / fvh_ndt_map_begin ...).
//   reg.begin_incremental_target(); reg.set_input_source(scan0); reg.insert_source_into_target(np.eye(4))
//   per scan: reg.set_input_source(scan); T = reg.align(guess); reg.insert_source_into_target(); reg.prune_target(T[:3, 3], radius)
template <typename Reg, typename PyClass>
static void def_incremental_target(PyClass& c) {
  c.def("begin_incremental_target", [](Reg& v, int expected_voxels) { v.beginIncrementalTarget(expected_voxels); }, py::arg("expected_voxels") = 0)
      .def("insert_source_into_target", [](Reg& v, const py::object& T) {  // T = None: the final transformation of the last align
        if (T.is_none()) v.insertSourceIntoTarget();
        else v.insertSourceIntoTarget(numpy2mat4(T.cast<Mat4>()));
      }, py::arg("T") = py::none())
      .def("prune_target", [](Reg& v, const py::object& center, double radius, int max_age) {
        if (center.is_none()) return v.pruneTarget(nullptr, radius, max_age);
        const auto c = center.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
        if (c.size() != 3) throw std::invalid_argument("prune_target: center must have 3 elements");
        return v.pruneTarget(c.data(), radius, max_age);
      }, py::arg("center") = py::none(), py::arg("radius") = 0.0, py::arg("max_age") = 0)
      // free-space carving (fvh_*_clear_rays_source): the voxels that >= min_misses rays origin -> source point at `pose` cross and none ends
      // in are dropped; call it before insert_source_into_target(pose). -> (voxels removed, rays used)
      .def("clear_target_rays", [](Reg& v, const Mat4& pose, const py::object& origin, double min_range, double max_range, double end_margin, int min_misses) {
        fast_gicp::RayClearing r;
        if (origin.is_none()) {
          r = v.clearTargetAlongRays(numpy2mat4(pose), nullptr, min_range, max_range, end_margin, min_misses);
        } else {
          const auto o = origin.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
          if (o.size() != 3) throw std::invalid_argument("clear_target_rays: origin must have 3 elements");
          r = v.clearTargetAlongRays(numpy2mat4(pose), o.data(), min_range, max_range, end_margin, min_misses);
        }
        return py::make_tuple(r.removed, r.rays_used);
      }, py::arg("pose"), py::arg("origin") = py::none(), py::arg("min_range") = 0.0, py::arg("max_range") = 100.0, py::arg("end_margin") = 0.0, py::arg("min_misses") = 1)
      // how well the target voxel map (batch or incremental) explains the source at `pose` (fvh_*_score_source; read-only): -> dict of the
      // counts and sums, overlap / nvtl / tp, and with per_point the arrays found, best (int32) and best_m2 (float64), one row per source point
      .def("score_target", [](Reg& v, const Mat4& pose, int neighbors, int min_points, double max_m2, double score_scale, bool per_point) {
        const fast_gicp::MapScore s = v.scoreTarget(numpy2mat4(pose), (fast_gicp::NeighborSearchMethod)neighbors, min_points, max_m2, score_scale, per_point);
        py::dict d;
        d["n_points"] = s.n_points; d["n_used"] = s.n_used; d["n_in_voxel"] = s.n_in_voxel; d["n_near"] = s.n_near; d["n_explained"] = s.n_explained;
        d["sum_best_m2"] = s.sum_best_m2; d["sum_score_max"] = s.sum_score_max; d["sum_score_all"] = s.sum_score_all;
        d["overlap"] = s.overlap(); d["nvtl"] = s.nvtl(); d["tp"] = s.tp();
        if (per_point) {
          d["found"] = py::array_t<int>((py::ssize_t)s.found.size(), s.found.data());
          d["best"] = py::array_t<int>((py::ssize_t)s.best.size(), s.best.data());
          d["best_m2"] = py::array_t<double>((py::ssize_t)s.best_m2.size(), s.best_m2.data());
        }
        return d;
      }, py::arg("pose"), py::arg("neighbors") = 1 /* DIRECT7 */, py::arg("min_points") = 1, py::arg("max_m2") = std::numeric_limits<double>::infinity(), py::arg("score_scale") = 1.0,
         py::arg("per_point") = false)
      // what the target voxel map (batch or incremental) says a sensor at `pose` should see along each ray (fvh_*_cast_rays_cloud / _source;
      // read-only): rays run from `origin` (scan frame, None: the origin) to `endpoints` (m x 3, scan frame; None: the source points). -> dict
      // of the counts, hit_ratio, and with per_ray the arrays hit (int32), cell (m x 3 int32), range and m2 (float64), one row per ray
      .def("cast_rays", [](Reg& v, const Mat4& pose, const py::object& endpoints, const py::object& origin, double min_range, double max_range, int min_points, double max_m2, bool per_ray) {
        std::array<double, 3> o3{};
        const double* o = nullptr;
        if (!origin.is_none()) {
          const auto oa = origin.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
          if (oa.size() != 3) throw std::invalid_argument("cast_rays: origin must have 3 elements");
          std::copy(oa.data(), oa.data() + 3, o3.begin());
          o = o3.data();
        }
        fast_gicp::RayCast s;
        if (endpoints.is_none()) {
          s = v.castRaysToSource(numpy2mat4(pose), o, min_range, max_range, min_points, max_m2, per_ray);
        } else {
          const auto e = endpoints.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
          if (e.size() % 3) throw std::invalid_argument("cast_rays: endpoints must be m x 3");
          s = v.castRays(numpy2mat4(pose), std::vector<float>(e.data(), e.data() + e.size()), o, min_range, max_range, min_points, max_m2, per_ray);
        }
        py::dict d;
        d["n_rays"] = s.n_rays; d["n_used"] = s.n_used; d["n_hit"] = s.n_hit; d["n_hit_at_origin"] = s.n_hit_at_origin; d["n_cells"] = s.n_cells;
        d["hit_ratio"] = s.hitRatio();
        if (per_ray) {
          d["hit"] = py::array_t<int>((py::ssize_t)s.hit.size(), s.hit.data());
          d["cell"] = py::array_t<int>(std::vector<py::ssize_t>{(py::ssize_t)s.hit.size(), 3}, s.cell.data());
          d["range"] = py::array_t<double>((py::ssize_t)s.range.size(), s.range.data());
          d["m2"] = py::array_t<double>((py::ssize_t)s.m2.size(), s.m2.data());
        }
        return d;
      }, py::arg("pose"), py::arg("endpoints") = py::none(), py::arg("origin") = py::none(), py::arg("min_range") = 0.0, py::arg("max_range") = 100.0, py::arg("min_points") = 1,
         py::arg("max_m2") = std::numeric_limits<double>::infinity(), py::arg("per_ray") = true)
      // the map as the handle's target cloud too (one point per voxel with >= min_points points; a snapshot): get_fitness_score() and
      // align_best() then work in this mode. -> number of points
      .def("target_cloud_from_map", [](Reg& v, int min_points) { return v.targetCloudFromMap(min_points); }, py::arg("min_points") = 1)
      // snapshots of the incremental target: save / restore / merge (fvh_*_voxelmap_export / _import / _merge_from). The dict is
      // {resolution, mode, num_inserts, num_points, num_voxels, coords (n, 3) int32, sums (n, 10) float64, ages (n,) uint32}
      .def("export_target_map", [](Reg& v) {
        const fast_gicp::TargetMapSnapshot m = v.exportTargetMap();
        const py::ssize_t n = (py::ssize_t)m.ages.size();
        py::array_t<int> coords({n, (py::ssize_t)3});
        py::array_t<double> sums({n, (py::ssize_t)10});
        py::array_t<unsigned> ages(n);
        if (n) {
          std::memcpy(coords.mutable_data(), m.coords.data(), sizeof(int) * m.coords.size());
          std::memcpy(sums.mutable_data(), m.sums.data(), sizeof(double) * m.sums.size());
          std::memcpy(ages.mutable_data(), m.ages.data(), sizeof(unsigned) * m.ages.size());
        }
        py::dict d;
        d["resolution"] = m.resolution; d["mode"] = m.mode; d["num_inserts"] = m.num_inserts; d["num_points"] = m.num_points; d["num_voxels"] = (int)n;
        d["coords"] = coords; d["sums"] = sums; d["ages"] = ages;
        return d;
      })
      .def("import_target_map", [](Reg& v, const py::dict& d) {
        fast_gicp::TargetMapSnapshot m;
        m.resolution = d["resolution"].cast<double>(); m.mode = d["mode"].cast<int>(); m.num_inserts = d["num_inserts"].cast<int>(); m.num_points = d["num_points"].cast<long long>();
        const auto coords = d["coords"].cast<py::array_t<int, py::array::c_style | py::array::forcecast>>();
        const auto sums = d["sums"].cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
        m.coords.assign(coords.data(), coords.data() + coords.size());
        m.sums.assign(sums.data(), sums.data() + sums.size());
        if (d.contains("ages") && !d["ages"].is_none()) {
          const auto ages = d["ages"].cast<py::array_t<unsigned, py::array::c_style | py::array::forcecast>>();
          m.ages.assign(ages.data(), ages.data() + ages.size());
        } else {
          m.ages.assign(m.coords.size() / 3, 0u);
        }
        v.importTargetMap(m);
      }, py::arg("snapshot"))
      .def("merge_target_from", [](Reg& v, Reg& other) { v.mergeTargetFrom(other); }, py::arg("other"))
      // a map built in another frame added under the rigid pose T (other's frame -> this map's), and the live map re-anchored in place
      // (fvh_*_posed_merge_from / fvh_*_transform_map). -> rows skipped because their mean left the key range
      .def("merge_target_from_posed", [](Reg& v, Reg& other, const Mat4& T) { return v.mergeTargetFromPosed(other, numpy2iso(T)); }, py::arg("other"), py::arg("T"))
      .def("transform_target_map", [](Reg& v, const Mat4& T) { return v.transformTargetMap(numpy2iso(T)); }, py::arg("T"))
      .def("save_target_map", [](Reg& v, const std::string& path) { v.saveTargetMap(path); }, py::arg("path"))
      .def("load_target_map", [](Reg& v, const std::string& path) { v.loadTargetMap(path); }, py::arg("path"));
}

PYBIND11_MODULE(pygicp, m) {
  m.doc() = "pygicp on the MI355X HIP engine (surface of koide3/fast_gicp src/python/main.cpp)";
  m.def("downsample", &downsample, "downsample points", py::arg("points"), py::arg("downsample_resolution"));
  m.def("downsample_device", &downsample_device, "downsample points on the GPU (bit-identical to downsample; exact=True: pcl::VoxelGrid)", py::arg("points"),
        py::arg("downsample_resolution"), py::arg("exact") = false, py::arg("device") = 0);
  m.def("crop_range_device", &crop_range_device, "keep the finite points with min_sq_norm <= |p|^2 <= max_sq_norm, on the GPU (the defaults: the origin filter)", py::arg("points"),
        py::arg("min_sq_norm") = 1e-3, py::arg("max_sq_norm") = std::numeric_limits<double>::infinity(), py::arg("return_indices") = false, py::arg("device") = 0);
  m.def("remove_outliers_device", &remove_outliers_device, "statistical (mean_k, stddev_mul) or radius (radius, min_neighbors) outlier removal on the GPU; kept points in input order",
        py::arg("points"), py::arg("method") = "STATISTICAL", py::arg("mean_k") = 20, py::arg("stddev_mul") = 1.0, py::arg("radius") = 0.8, py::arg("min_neighbors") = 2,
        py::arg("return_indices") = false, py::arg("device") = 0);
  m.def("cluster_euclidean_device", &cluster_euclidean_device, "Euclidean cluster extraction on the GPU: (labels per input point or -1, cluster sizes); clusters numbered by their smallest input index",
        py::arg("points"), py::arg("tolerance"), py::arg("min_cluster_size") = 1, py::arg("max_cluster_size") = 0, py::arg("device") = 0);
  m.def("segment_plane_device", &segment_plane_device, "RANSAC plane segmentation on the GPU: (coefficients (a, b, c, d), indices of the kept points: the inliers, or with keep_outliers everything else)",
        py::arg("points"), py::arg("distance_threshold"), py::arg("max_iterations") = 256, py::arg("seed") = 0ull, py::arg("axis") = py::none(), py::arg("eps_angle") = 0.0,
        py::arg("keep_outliers") = false, py::arg("refine") = false, py::arg("device") = 0);
  m.def("deskew_device", &deskew_device, "motion-compensate a sweep on the GPU: points (n, 3) with one time each, moved along the trajectory through the knot poses into the sensor frame of t_ref",
        py::arg("points"), py::arg("times"), py::arg("knot_times"), py::arg("knot_poses"), py::arg("t_ref") = py::none(), py::arg("device") = 0);
  m.def("align_points", &align_points, "align two point sets", py::arg("target"), py::arg("source"), py::arg("method") = "VGICP_CUDA", py::arg("downsample_resolution") = -1.0,
        py::arg("k_correspondences") = 15, py::arg("max_correspondence_distance") = std::numeric_limits<double>::max(), py::arg("voxel_resolution") = 1.0,
        py::arg("num_threads") = 0, py::arg("neighbor_search_method") = "DIRECT1", py::arg("neighbor_search_radius") = 1.5, py::arg("initial_guess") = identity4());

  py::class_<Lsq, std::shared_ptr<Lsq>>(m, "LsqRegistration")
      .def("set_input_target", [](Lsq& reg, const Points& p) { reg.setInputTarget(numpy2cloud(p)); })
      .def("set_input_source", [](Lsq& reg, const Points& p) { reg.setInputSource(numpy2cloud(p)); })
      .def("swap_source_and_target", &Lsq::swapSourceAndTarget)
      .def("clear_source", &Lsq::clearSource)
      .def("clear_target", &Lsq::clearTarget)
      .def("get_final_hessian", [](Lsq& reg) {
        py::array_t<double> H({6, 6});
        std::memcpy(H.mutable_data(), reg.getFinalHessian().data(), 36 * sizeof(double));
        return H;
      })
      .def("get_final_transformation", [](Lsq& reg) { return mat4_to_numpy(reg.getFinalTransformation()); })
      .def("get_fitness_score", [](Lsq& reg, double max_range) { return reg.getFitnessScore(max_range); }, py::arg("max_range") = std::numeric_limits<double>::max())
      .def("has_converged", &Lsq::hasConverged)
      .def("set_maximum_iterations", &Lsq::setMaximumIterations)
      .def("set_transformation_epsilon", &Lsq::setTransformationEpsilon)
      .def("set_rotation_epsilon", &Lsq::setRotationEpsilon)
      .def("set_initial_lambda_factor", &Lsq::setInitialLambdaFactor)
      .def("set_debug_print", &Lsq::setDebugPrint)
      .def("set_use_device_lm", &Lsq::setUseDeviceLM)
      .def("set_lsq_type", [](Lsq& reg, const std::string& t) {  // lsq_optimizer_type_ (lsq_registration.hpp:13,78): "LM" (default) or "GN"
        if (t == "LM" || t == "LevenbergMarquardt") reg.setLSQType(fast_gicp::LSQ_OPTIMIZER_TYPE::LevenbergMarquardt);
        else if (t == "GN" || t == "GaussNewton") reg.setLSQType(fast_gicp::LSQ_OPTIMIZER_TYPE::GaussNewton);
        else throw std::invalid_argument("unknown optimizer type " + t + " (LM, GN)");
      })
      .def("evaluate_cost", [](Lsq& reg, const Mat4& pose) {
        Matrix6d H; Vector6d b;
        const double e = reg.evaluateCost(numpy2mat4(pose), &H, &b);
        py::array_t<double> Hn({6, 6}), bn(6);
        std::memcpy(Hn.mutable_data(), H.data(), 36 * sizeof(double));
        std::memcpy(bn.mutable_data(), b.data(), 6 * sizeof(double));
        return py::make_tuple(e, Hn, bn);
      })
      .def("align", [](Lsq& reg, const Mat4& initial_guess) {
        Cloud aligned;
        reg.align(aligned, numpy2mat4(initial_guess));
        return mat4_to_numpy(reg.getFinalTransformation());
      }, py::arg("initial_guess") = identity4())
      // not in the reference: K initial guesses of the same pair in ONE device launch (include/fast_vgicp_hip.h: fvh_vgicp_align_multi /
      // fvh_ndt_align_multi; FastVGICPCuda, FastVGICP, NDTCuda -- FastGICP raises). (K, 4, 4) ->
      // (T (K, 4, 4) float64, final_error (K,), converged (K,) bool, iterations (K,) int: getNumIterations() of align(guess k))
      .def("align_multi", [](Lsq& reg, const Mat4& guesses) {
        const std::vector<MultiAlignResult> rs = reg.alignMulti(numpy2mat4s(guesses));
        const py::ssize_t k = (py::ssize_t)rs.size();
        py::array_t<double> T({k, (py::ssize_t)4, (py::ssize_t)4}), err(k);
        py::array_t<bool> conv(k);
        py::array_t<int> its(k);
        for (py::ssize_t i = 0; i < k; i++) {
          std::memcpy(T.mutable_data() + 16 * i, rs[i].T.m, 16 * sizeof(double));
          err.mutable_data()[i] = rs[i].final_error;
          conv.mutable_data()[i] = rs[i].converged;
          its.mutable_data()[i] = rs[i].nr_iterations;
        }
        return py::make_tuple(T, err, conv, its);
      }, py::arg("guesses"))
      // ... and the pose with the lowest fitness score becomes the result as align() would leave it: (get_final_transformation(), index)
      .def("align_best", [](Lsq& reg, const Mat4& guesses, double max_range) {
        Cloud aligned;
        const int best = reg.alignBest(numpy2mat4s(guesses), max_range, aligned);
        return py::make_tuple(mat4_to_numpy(reg.getFinalTransformation()), best);
      }, py::arg("guesses"), py::arg("max_range") = std::numeric_limits<double>::max());

  py::class_<VGICPCuda, Lsq, std::shared_ptr<VGICPCuda>> vgicp_cuda(m, "FastVGICPCuda");
  vgicp_cuda
      .def(py::init([](int device) { return std::make_shared<VGICPCuda>(device); }), py::arg("device") = 0)
      .def("set_resolution", &VGICPCuda::setResolution)
      .def("set_voxel_accumulation_mode", [](VGICPCuda& v, const std::string& mode) { v.setVoxelAccumulationMode(voxel_accumulation_mode(mode)); })
      .def("set_neighbor_search_method", [](VGICPCuda& v, const std::string& method, double radius) { v.setNeighborSearchMethod(search_method(method), radius); },
           py::arg("method") = "DIRECT1", py::arg("radius") = 1.5)
      .def("set_correspondence_randomness", &VGICPCuda::setCorrespondenceRandomness)
      .def("set_kernel_width", &VGICPCuda::setKernelWidth, py::arg("kernel_width"), py::arg("max_dist") = -1.0)
      .def("set_regularization_method", [](VGICPCuda& v, const std::string& s) { v.setRegularizationMethod(regularization_method(s)); })
      .def("set_nearest_neighbor_search_method", [](VGICPCuda& v, const std::string& s) { v.setNearestNeighborSearchMethod(nn_method(s)); })
      // not in the reference: CPU_PARALLEL_KDTREE (the default enum value) is served by the device's exact search unless the host tree is asked for
      .def("set_host_kdtree", &VGICPCuda::setHostKdTree, py::arg("on") = true)
      // not in the reference: the scan stream as a two-stage pipeline (include/fast_vgicp_hip.h: fvh_vgicp_prepare_source / _align_async ...).
      //   reg.align_async(); reg.prepare_next_source(next_scan); T = reg.align_wait(); reg.swap_source_and_target(); reg.adopt_prepared_source()
      // The numpy conversion, the staging copy and the device's sort / k-NN / covariances of the next scan all run while the LM kernel of the current pair does.
      .def("prepare_next_source", [](VGICPCuda& v, const Points& p, int stages) { v.prepareNextSource(numpy2cloud(p), stages); }, py::arg("points"), py::arg("stages") = 2)
      .def("adopt_prepared_source", &VGICPCuda::adoptPreparedSource)
      .def("align_async", [](VGICPCuda& v, const Mat4& initial_guess) { v.alignAsync(numpy2mat4(initial_guess)); }, py::arg("initial_guess") = identity4())
      .def("align_wait", [](VGICPCuda& v) { return mat4_to_numpy(v.alignWait()); });
  def_incremental_target<VGICPCuda>(vgicp_cuda);

  py::class_<GICP, Lsq, std::shared_ptr<GICP>>(m, "FastGICP")  // main.cpp:183-190
      .def(py::init([](int device) { return std::make_shared<GICP>(device); }), py::arg("device") = 0)
      .def("set_num_threads", &GICP::setNumThreads)
      .def("set_correspondence_randomness", &GICP::setCorrespondenceRandomness)
      .def("set_max_correspondence_distance", &GICP::setMaxCorrespondenceDistance)
      .def("set_regularization_method", [](GICP& g, const std::string& s) { g.setRegularizationMethod(regularization_method(s)); })
      // not in the reference's bindings (its C++ class has them: gicp/fast_gicp.hpp:60-70): (N, 3, 3) arrays
      .def("get_source_covariances", [](GICP& g) { return covs_to_numpy(g.getSourceCovariances()); })
      .def("get_target_covariances", [](GICP& g) { return covs_to_numpy(g.getTargetCovariances()); })
      .def("set_source_covariances", [](GICP& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& c) { g.setSourceCovariances(numpy_to_covs(c)); })
      .def("set_target_covariances", [](GICP& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& c) { g.setTargetCovariances(numpy_to_covs(c)); });

  // The reference's CPU class (main.cpp:192-196; as there it derives from FastGICP: set_num_threads, set_correspondence_randomness,
  // set_max_correspondence_distance, the covariance accessors), served by the GPU engine in its fp64 arithmetic; k IS honoured.
  py::class_<VGICP, GICP, std::shared_ptr<VGICP>>(m, "FastVGICP")
      .def(py::init([](int device) { return std::make_shared<VGICP>(device); }), py::arg("device") = 0)
      .def("set_max_correspondence_distance", &VGICP::setMaxCorrespondenceDistance)  // (FastVGICP never reads it: voxel correspondences)
      .def("set_resolution", &VGICP::setResolution)
      .def("set_voxel_accumulation_mode", [](VGICP& v, const std::string& mode) { v.setVoxelAccumulationMode(voxel_accumulation_mode(mode)); })
      .def("set_neighbor_search_method", [](VGICP& v, const std::string& method) { v.setNeighborSearchMethod(search_method(method)); }, py::arg("method") = "DIRECT1");

  py::class_<NDT, Lsq, std::shared_ptr<NDT>> ndt_cuda(m, "NDTCuda");
  ndt_cuda
      .def(py::init([](int device) { return std::make_shared<NDT>(device); }), py::arg("device") = 0)
      .def("set_neighbor_search_method", [](NDT& n, const std::string& method, double radius) { n.setNeighborSearchMethod(search_method(method), radius); },
           py::arg("method") = "DIRECT1", py::arg("radius") = 1.5)
      .def("set_resolution", &NDT::setResolution)
      .def("set_distance_mode", [](NDT& n, const std::string& s) {
        if (s == "P2D") n.setDistanceMode(NDTDistanceMode::P2D);
        else if (s == "D2D") n.setDistanceMode(NDTDistanceMode::D2D);
        else throw std::invalid_argument("unknown NDT distance mode " + s);
      })
      // not in the reference: the frame stream as a two-stage pipeline (as FastVGICPCuda's)
      .def("prepare_next_source", [](NDT& n, const Points& p) { n.prepareNextSource(numpy2cloud(p)); }, py::arg("points"))
      .def("adopt_prepared_source", &NDT::adoptPreparedSource)
      .def("align_async", [](NDT& n, const Mat4& initial_guess) { n.alignAsync(numpy2mat4(initial_guess)); }, py::arg("initial_guess") = identity4())
      .def("align_wait", [](NDT& n) { return mat4_to_numpy(n.alignWait()); });
  // not in the reference: NDTCuda with an incremental target map (C++: the same NDTCuda methods; fvh_ndt_map_* / fvh_ndt_voxelmap_*). Its own
  // Python class, so that NDTCuda keeps the reference's surface: everything of NDTCuda + the incremental-target methods of FastVGICPCuda,
  // same names. The voxels are sums of the inserted points: snapshots carry mode 3.
  py::class_<NDTMap, NDT, std::shared_ptr<NDTMap>> ndt_map(m, "NDTCudaMap");
  ndt_map.def(py::init([](int device) { return std::make_shared<NDTMap>(device); }), py::arg("device") = 0);
  def_incremental_target<NDTMap>(ndt_map);

  // testing hook: the host kd-tree behind NearestNeighborMethod::CPU_PARALLEL_KDTREE
  m.def("_kdtree_knn", [](const Points& points, int k) {
    auto cloud = numpy2cloud(points);
    const std::vector<float> xyz = detail::pack_xyz(*cloud);
    const int n = (int)cloud->size();
    host::KdTree tree(xyz.data(), n);
    py::array_t<int> out({(py::ssize_t)n, (py::ssize_t)k});
    int* o = out.mutable_data();
#pragma omp parallel for schedule(guided, 8) num_threads(host::omp_threads_for(n))
    for (int i = 0; i < n; i++) tree.knn(&xyz[3 * (size_t)i], k, o + (size_t)i * k);
    return out;
  });
  m.attr("__version__") = "dev";
}
