// ORACLE (test infrastructure, NOT product code).  Only tests/, __graft_entry__.smoke()
// and bench.py's cpu_baseline leg may use anything under oracle/.
//
// Dependency-free C++17 + OpenMP fp64 restatement of the reference's CPU path
// FastVGICP (koide3/fast_gicp @ 2024-10-22), plus fp64 restatements of the CUDA-only
// formulas that have no CPU counterpart (RBF covariances, NDT voxel maps and costs).
// The reference itself cannot be built here (needs PCL, Eigen, Boost, FLANN; all
// absent, thirdparty/ submodules empty), so this is a "port" oracle.  It is pinned
// against (tests/test_oracle.py):
//   * README.md:116 point counts 17,249/17,518 (ApproximateVoxelGrid restatement),
//   * data/relative.txt with gicp_test.cpp:148-149 tolerances (0.05 m, 1 deg, converged),
//   * README.md:118-134 fitness scores as a +-1 % band,
//   * an independent numpy/scipy twin (oracle/np_twin.py).
// Everything finer than that is "parity unpinned" (no golden H/b in the reference).
//
// Each function cites the reference file:line it follows (paths relative to the
// reference root).
#pragma once
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "oracle_math.hpp"

namespace orc {

// gicp_settings.hpp:7-11 / ndt_settings.hpp:6 (enum order preserved)
enum RegularizationMethod { NONE = 0, MIN_EIG = 1, NORMALIZED_MIN_EIG = 2, PLANE = 3, FROBENIUS = 4 };
enum NeighborSearchMethod { DIRECT27 = 0, DIRECT7 = 1, DIRECT1 = 2, DIRECT_RADIUS = 3 };
enum NDTDistanceMode { P2D = 0, D2D = 1 };

struct KdTree;

struct Cloud {
  std::vector<float> xyz;  // packed x,y,z (pcl::PointXYZ data, fp32)
  size_t size() const { return xyz.size() / 3; }
  const float* pt(size_t i) const { return &xyz[3 * i]; }
};
using CloudPtr = std::shared_ptr<const Cloud>;

// ---- I/O and preprocessing (align.cpp:118-147; PCL restated) ----
bool load_pcd(const std::string& path, Cloud& out);
void remove_origin_points(Cloud& c);                                     // align.cpp:127-133
void approximate_voxel_grid(const Cloud& in, float leaf, Cloud& out);    // pcl::ApproximateVoxelGrid
void voxel_grid(const Cloud& in, float leaf, Cloud& out);                // pcl::VoxelGrid (gicp_test.cpp:55-65)

// ---- exact k-NN (pcl::search::KdTree / FLANN stand-in) ----
struct KdTree {
  explicit KdTree(const Cloud& c);
  // k nearest incl. the query itself if it is in the cloud; fp32 squared distances
  // ((dx*dx + dy*dy) + dz*dz, no FMA), ties broken by lower index; sorted ascending.
  void knn(const float* q, int k, int* out_idx, float* out_sqdist) const;
  const Cloud& cloud;
  struct Node { int left, right, begin, end, dim; float split; };
  std::vector<Node> nodes;
  std::vector<int> order;
  int build(int begin, int end);
};

void knn_all(const Cloud& c, int k, int num_threads, std::vector<int>& idx);  // fast_vgicp_cuda_impl.hpp:152-167

// ---- covariances ----
M3 regularize(const M3& cov, RegularizationMethod m);                                              // fast_gicp_impl.hpp:267-297
void covariances_from_neighbors(const Cloud& c, int k, const std::vector<int>& idx, RegularizationMethod m, int num_threads,
                                std::vector<M3>& covs);                                                // fast_gicp_impl.hpp:244-301
void covariances_rbf(const Cloud& c, double kernel_width, double max_dist, RegularizationMethod m, int num_threads,
                     std::vector<M3>& covs);                                                           // covariance_estimation_rbf.cu:40-109

// ---- Gaussian voxel map (fast_vgicp_voxel.hpp:124-182; gaussian_voxelmap.cu:178-198 for NDT) ----
struct VoxelKey { int x, y, z; bool operator==(const VoxelKey& o) const { return x == o.x && y == o.y && z == o.z; } };
struct VoxelKeyHash { size_t operator()(const VoxelKey& k) const; };
struct Voxel { int num_points = 0; V3 mean{{0, 0, 0}}; M3 cov = m3_zero(); };

struct VoxelMap {
  double resolution;
  std::unordered_map<VoxelKey, int, VoxelKeyHash> index;  // coord -> voxel slot (insertion order)
  std::vector<VoxelKey> coords;
  std::vector<Voxel> voxels;
  explicit VoxelMap(double res) : resolution(res) {}
  VoxelKey coord(const V3& x) const;                                               // fast_vgicp_voxel.hpp:158-160
  void create_vgicp(const Cloud& c, const std::vector<M3>& covs, int mode = 0);    // :129-156, AdditiveGaussianVoxel :105-122, MultiplicativeGaussianVoxel :79-103
  void create_ndt(const Cloud& c);                                                 // gaussian_voxelmap.cu:122-148,178-198 + ndt_cuda.cu:128,139
  int lookup(const VoxelKey& k) const;                                             // :167-174
};

std::vector<VoxelKey> neighbor_offsets(NeighborSearchMethod m, double radius = 0.0);  // fast_vgicp_voxel.hpp:10-43; fast_vgicp_cuda.cu:41-94

// ---- LM optimiser state shared by VGICP and NDT (lsq_registration_impl.hpp) ----
struct LsqBase {
  int max_iterations = 64;               // :11
  double rotation_epsilon = 2e-3;        // :12
  double transformation_epsilon = 5e-4;  // :13
  int lm_max_iterations = 10;            // :17
  double lm_init_lambda_factor = 1e-9;   // :18
  double lm_lambda = -1.0;               // :19
  bool lm_debug_print = false;
  bool converged = false;
  int nr_iterations = 0;
  int num_linearize = 0, num_error_evals = 0;  // bookkeeping for the algorithmic-bytes model
  double final_hessian[36];
  Iso3 final_transformation = iso_identity();  // as double; callers cast to float like :77
  virtual ~LsqBase() {}
  virtual double linearize(const Iso3& T, double* H, double* b) = 0;
  virtual double compute_error(const Iso3& T) = 0;
  bool is_converged(const Iso3& delta) const;        // :82-91
  bool gauss_newton = false;                         // lsq_optimizer_type_ == GaussNewton (:15 default: LevenbergMarquardt)
  bool step_gn(Iso3& x0, Iso3& delta);               // :108-121
  bool step_lm(Iso3& x0, Iso3& delta);               // :123-168
  void optimize(const Iso3& guess);                  // :53-79 (computeTransformation minus the PCL cloud transform)
};

// ---- FastVGICP (fast_vgicp_impl.hpp, fast_gicp_impl.hpp) ----
struct FastVGICP : LsqBase {
  int num_threads;
  int k_correspondences = 20;                         // fast_gicp_impl.hpp:17
  RegularizationMethod regularization = PLANE;        // :21
  double voxel_resolution = 1.0;                      // fast_vgicp_impl.hpp:22
  NeighborSearchMethod search_method = DIRECT1;       // :23
  double search_radius = 0.0;                         // DIRECT_RADIUS (the CUDA classes' fourth method, fast_vgicp_cuda.cu:77-91) on the fp64 formulas
  // covariance source: 0 = kd-tree k-NN (CPU reference), 1 = RBF kernel (CUDA formula)
  int cov_mode = 0;
  int voxel_mode = 0;                                 // VoxelAccumulationMode ordinal (fast_vgicp_impl.hpp:24 ADDITIVE; 2 = MULTIPLICATIVE)
  double kernel_width = 0.5, kernel_max_dist = 3.0;   // fast_vgicp_cuda_impl.hpp:31
  // when true, regularised covariances / voxel means+covs are rounded to fp32 before use,
  // mirroring the fp32 HBM storage of the HIP engine (diagnostic only).
  bool round_storage_fp32 = false;
  // FastGICP (the base class of FastVGICP in the reference, fast_gicp_impl.hpp:118-240): correspondences are the
  // nearest TARGET POINT within corr_dist_threshold_ instead of voxels; weight 1, target point covariances.
  bool gicp_mode = false;
  double max_correspondence_distance = 3.4028234663852886e38;  // fast_gicp_impl.hpp:18 (float max)

  CloudPtr input, target;
  std::shared_ptr<KdTree> search_source, search_target, pcl_tree;  // pcl_tree = PCL Registration::tree_
  std::vector<M3> source_covs, target_covs;
  std::unique_ptr<VoxelMap> voxelmap;
  std::vector<std::pair<int, int>> voxel_correspondences;
  std::vector<M3> voxel_mahalanobis;
  Iso3 lin_pose = iso_identity();  // pose of the last update_correspondences()
  bool target_cloud_updated = false;

  FastVGICP();
  void setInputTarget(const CloudPtr& c);   // fast_vgicp_impl.hpp:56-63 + fast_gicp_impl.hpp:88-95
  void setInputSource(const CloudPtr& c);   // fast_gicp_impl.hpp:77-85
  void clearSource();                       // :65-68
  void clearTarget();                       // :71-74
  void swapSourceAndTarget();               // fast_vgicp_impl.hpp:46-53
  void align(const Iso3& guess);            // pcl::Registration::align -> fast_vgicp_impl.hpp:66-70 -> fast_gicp_impl.hpp:103-115
  double getFitnessScore() const;           // pcl::Registration::getFitnessScore (max_range = inf)

  void calculate_covariances(const CloudPtr& c, const KdTree& tree, std::vector<M3>& covs);
  void update_correspondences(const Iso3& T);                    // fast_vgicp_impl.hpp:73-116
  double linearize(const Iso3& T, double* H, double* b) override;  // :119-178
  double compute_error(const Iso3& T) override;                    // :181-204
  double cuda_compat_sums(const Iso3& T, double* H, double* b) const;  // compute_derivatives.cu:50-103 in float over the current correspondences
};

// ---- NDT (ndt_cuda.cu, ndt_compute_derivatives.cu, ndt_cuda_impl.hpp), fp64 restatement ----
struct NDT : LsqBase {
  int num_threads;
  double resolution = 1.0;                      // ndt_cuda.cu:15
  NDTDistanceMode distance_mode = D2D;          // :21
  NeighborSearchMethod search_method = DIRECT7; // :22
  double search_radius = 0.0;
  bool round_storage_fp32 = false;              // test leg: voxel means/covs rounded to float as the device stores them
  CloudPtr input, target;
  std::shared_ptr<KdTree> pcl_tree;
  std::unique_ptr<VoxelMap> source_voxelmap, target_voxelmap;
  std::vector<std::pair<int, int>> correspondences;
  Iso3 linearized_x = iso_identity();
  bool target_cloud_updated = false;

  NDT();
  void setInputTarget(const CloudPtr& c);  // ndt_cuda_impl.hpp:63-73 + ndt_cuda.cu:105-113
  void setInputSource(const CloudPtr& c);  // :52-60 + ndt_cuda.cu:95-103
  void clearSource() { input.reset(); }
  void clearTarget() { target.reset(); }
  void swapSourceAndTarget();              // ndt_cuda_impl.hpp:36-39 + ndt_cuda.cu:90-93
  void align(const Iso3& guess);           // :76-79
  double getFitnessScore() const;
  void create_voxelmaps();                 // ndt_cuda.cu:115-140
  double linearize(const Iso3& T, double* H, double* b) override;
  double compute_error(const Iso3& T) override;
  double cost(const Iso3& T, double* H, double* b);  // ndt_compute_derivatives.cu:33-175
};

// mean squared exact-NN distance of (float T)*source to target (PCL getFitnessScore semantics)
double fitness_score(const Cloud& source, const KdTree& target_tree, const Iso3& T);

}  // namespace orc
