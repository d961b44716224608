/*
 * fast_vgicp_hip.h -- C ABI of libfast_vgicp_hip.so, the MI355X (gfx950) engine that drops in where
 * the reference's nvcc-built libfast_vgicp_cuda.so sits (the pimpl classes
 * fast_gicp::cuda::FastVGICPCudaCore and fast_gicp::cuda::NDTCudaCore).
 *
 * Reference files cited below are relative to koide3/fast_gicp @ 2024-10-22:
 *   [VC]  include/fast_gicp/cuda/fast_vgicp_cuda.cuh   (class FastVGICPCudaCore, lines 28-92)
 *   [VCU] src/fast_gicp/cuda/fast_vgicp_cuda.cu
 *   [NC]  include/fast_gicp/cuda/ndt_cuda.cuh          (class NDTCudaCore, lines 28-68)
 *   [NCU] src/fast_gicp/cuda/ndt_cuda.cu
 *
 * Conventions
 *   - Every function returns an int status (FVH_OK == 0); fvh_*_last_error() gives the message.
 *     Nothing throws across the ABI.  (The reference has no error reporting: asserts/abort.)
 *   - The library owns all device memory behind the opaque handle; inputs are copied
 *     (caller keeps its buffers), outputs go to caller-allocated buffers -- same ownership
 *     as the reference's std::vector-by-const-ref / out-param style.
 *   - A handle is used from one host thread at a time; distinct handles may be used
 *     concurrently.  Each handle owns one HIP stream; calls are synchronous unless noted.
 *   - Poses are 4x4 double, COLUMN-MAJOR, i.e. exactly Eigen::Isometry3d::data(); H is 6x6
 *     double column-major (Eigen::Matrix<double,6,6>::data(), it is symmetric), b is 6 doubles.
 *     Twist order is (rot xyz, trans xyz) as in the reference.
 *   - Point clouds are packed float xyz (Eigen::Vector3f layout, 12 B/point).
 *   - 3x3 covariances returned by getters are 9 floats column-major (Eigen::Matrix3f layout).
 *   - Enum values equal the reference's enum class ordinals (gicp_settings.hpp:7-11,
 *     ndt_settings.hpp:6) so a static_cast<int>() in the shim is enough.
 */
#ifndef FAST_VGICP_HIP_H
#define FAST_VGICP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fvh_vgicp fvh_vgicp; /* replaces fast_gicp::cuda::FastVGICPCudaCore */
typedef struct fvh_ndt fvh_ndt;     /* replaces fast_gicp::cuda::NDTCudaCore */

enum fvh_status { FVH_OK = 0, FVH_ERR_INVALID_ARGUMENT = 1, FVH_ERR_BAD_STATE = 2, FVH_ERR_HIP = 3, FVH_ERR_UNSUPPORTED = 4, FVH_ERR_COMM = 5 };

/* fast_gicp::RegularizationMethod (gicp_settings.hpp:7) */
enum fvh_regularization { FVH_REG_NONE = 0, FVH_REG_MIN_EIG = 1, FVH_REG_NORMALIZED_MIN_EIG = 2, FVH_REG_PLANE = 3, FVH_REG_FROBENIUS = 4 };
/* fast_gicp::NeighborSearchMethod (gicp_settings.hpp:9) */
enum fvh_neighbor_search { FVH_DIRECT27 = 0, FVH_DIRECT7 = 1, FVH_DIRECT1 = 2, FVH_DIRECT_RADIUS = 3 };
/* fast_gicp::NDTDistanceMode (ndt_settings.hpp:6) */
enum fvh_ndt_distance_mode { FVH_NDT_P2D = 0, FVH_NDT_D2D = 1 };
/* arithmetic: FP64 matches the CPU FastVGICP (default); FP32 runs the per-correspondence cost math in float like the CUDA path (sums are
 * still accumulated in fp64) on the engine's fp64-centred covariances; CUDA_COMPAT is FastVGICPCuda's arithmetic end to end -- FP32's cost
 * math + the k-NN covariances as covariance_estimation.cu:20-35 / covariance_regularization.cu:15-125 compute them (uncentred float sums
 * in neighbour-list order, Eigen's closed-form float eigen solver). VGICP handles only; RBF covariances and the voxel sums stay fp64. */
enum fvh_precision { FVH_COMPUTE_FP64 = 0, FVH_COMPUTE_FP32 = 1, FVH_COMPUTE_CUDA_COMPAT = 2 };

/* LsqRegistration parameters (lsq_registration_impl.hpp:9-22 defaults) for the device-resident optimiser loop */
typedef struct fvh_lm_params {
  int max_iterations;            /* 64   pcl max_iterations_ */
  double rotation_epsilon;       /* 2e-3 */
  double transformation_epsilon; /* 5e-4 */
  int lm_max_iterations;         /* 10 */
  double lm_init_lambda_factor;  /* 1e-9 */
  int optimizer;                 /* 0 LSQ_OPTIMIZER_TYPE::LevenbergMarquardt (step_lm, default), 1 GaussNewton (step_gn, lsq_registration_impl.hpp:108-121) */
} fvh_lm_params;

typedef struct fvh_lm_result {
  double T[16];        /* final pose x0, column-major double (reference casts it to float) */
  double H[36];        /* final_hessian_ (last accepted, undamped) */
  double final_error;  /* y0 of the last linearisation */
  int converged;       /* converged_ */
  int nr_iterations;   /* nr_iterations_ (index of the last outer iteration) */
  int num_linearize;   /* calls to linearize() */
  int num_error_evals; /* calls to compute_error() */
  int lm_failed;       /* 1 = "lm not converged!!" (lsq_registration_impl.hpp:69-72) */
  int num_launches;    /* kernel launches used by this align */
} fvh_lm_result;

void fvh_default_lm_params(fvh_lm_params* p);
int fvh_device_count(int* count);

/* Engine parameters of a handle (round 6): the routes, thresholds and watchdogs that rounds 1-5 read from the process environment each time
 * they were consulted. They are per-handle state now: a new handle starts from fvh_default_engine_params() -- the built-in defaults with
 * the FVH_* environment variables of INTEGRATION.md applied ONCE per process -- and fvh_*_set_engine_params() changes one handle only.
 * (Process-wide by nature and therefore NOT in here: how concurrent aligns split the device's co-resident workgroup slots, the XCD-local
 * hand-offs and the small-grid layout, which every handle of a process must agree on: FVH_SLOT_MAX_SPLIT, FVH_CONTENDED_SLOT_PCT,
 * FVH_XCD_LOCAL, FVH_SMALL_GRID_LAYOUT.) No reference counterpart. */
typedef struct fvh_engine_params {
  int struct_size;                       /* sizeof(fvh_engine_params) of the caller's header: set by fvh_default_engine_params, checked by the setters */
  /* Morton sort of a cloud */
  int sort_mode;                         /* 0 multi-kernel radix, 1 one workgroup, 2 cooperative kernel while no other handle has a gang kernel in flight, else the radix passes (default), 3 cooperative always */
  int sort_items;                        /* points per wave of the radix passes; 0 = by cloud size */
  int sort_fused_bits;                   /* two-launch passes (32k..256k points): 10 (default) or 9 key bits per pass, 0 = four-launch passes */
  int sort_two_pass_max;                 /* clouds up to this size take two 11-bit four-launch passes (262,144) */
  unsigned long long sort_coop_watchdog_ticks; /* 100 MHz ticks before the cooperative sort gives up and the one-workgroup sort redoes it (2,000,000; 0 = at once: test hook) */
  /* neighbour search */
  int knn_nearest_first_max_points;      /* clouds up to this size walk the boxes nearest first (65,536) */
  int knn_block;                         /* threads per workgroup of the k-NN kernel: 64 (default), 128, 256 */
  /* voxel map */
  int coherent_min_points;               /* clouds of this size and up are walked in Morton order (32,768) */
  int bitmap_min_points;                 /* maps of this size and up get an occupancy bitmap (300,000) */
  unsigned long long bitmap_max_bytes;   /* its budget (32 MiB) */
  /* the LM kernel */
  int persistent;                        /* 1 (default): one launch per align while the problem is latency-bound; 0: one launch per LM transition */
  unsigned long long persist_watchdog_ticks; /* 100 MHz ticks a hand-off may take before the launch aborts and the align is redone per transition (5,000,000; 0: test hook) */
  unsigned long long peer_watchdog_ticks;    /* ... for a peer rank's sums (200,000,000) */
  int lm_everywhere;                     /* 0 never, 1 (default) on grids of at most two workgroups per CU, 2 always: every workgroup runs the LM step itself */
  int cost_prio;                         /* -1 (default) by grid shape, 0 never, 1 always: s_setprio for the second workgroup of a CU */
  int cost_split;                        /* 1 (default): wave roles for NDT launches of at most one workgroup per CU */
  int cost_group_max;                    /* voxel lookups per work item, 1..4 (4) */
  int cost_max_blocks;                   /* grid cap of a cost launch (1,024) */
  long long cost_target_items;           /* work items a small problem is split into (131,072) */
  int zerocopy_result;                   /* 1 (default): the final LM state travels through mapped host memory */
  int host_wait_block;                   /* 0 (default): the host spins on the result word; 1: it sleeps in hipStreamSynchronize */
  unsigned long long result_query_spins; /* spins between two hipStreamQuery calls while waiting (1,024) */
  /* streams and uploads */
  int side_stream;                       /* 1 (default): swap_source_and_target rebuilds the target map on a second stream */
  unsigned long long pinned_upload_max;  /* host clouds up to this many bytes go through the handle's pinned staging buffer (8 MiB) */
  unsigned long long zerocopy_upload_max;/* ... and up to this many are read by the widening kernel straight over PCIe (1 MiB) */
  /* ApproximateVoxelGrid */
  int avg_fused;                         /* 1 (default): four launches up to 262,144 points; 0: round 2's six */
  /* exact 1-NN search (FastGICP correspondences) */
  int nn1_seed;                          /* 1 (default): the id a point found last time seeds the bound of its next search (identical ids); 0: every search from scratch */
} fvh_engine_params;
void fvh_default_engine_params(fvh_engine_params* p);

/* ---------------------------------------------------------------------------------------------
 * FastVGICPCudaCore
 * ------------------------------------------------------------------------------------------- */
/* [VC]:37 ctor ([VCU]:18-30: res 1.0, kernel 0.25/3.0, offsets {0,0,0}) / [VC]:38 dtor */
int fvh_vgicp_create(int device, fvh_vgicp** out);
int fvh_vgicp_destroy(fvh_vgicp* h);
const char* fvh_vgicp_last_error(const fvh_vgicp* h);

int fvh_vgicp_set_resolution(fvh_vgicp* h, double resolution);                               /* [VC]:40 */
int fvh_vgicp_set_kernel_params(fvh_vgicp* h, double kernel_width, double kernel_max_dist);  /* [VC]:41 */
/* DIRECT_RADIUS: offsets up to +-511 voxels per axis (they travel packed, 10 bits each); a larger radius is FVH_ERR_INVALID_ARGUMENT */
int fvh_vgicp_set_neighbor_search_method(fvh_vgicp* h, int method, double radius);           /* [VC]:42, [VCU]:41-94 */
int fvh_vgicp_set_precision(fvh_vgicp* h, int precision);                                    /* new */
int fvh_vgicp_get_engine_params(fvh_vgicp* h, fvh_engine_params* out);                       /* new: see fvh_engine_params */
int fvh_vgicp_set_engine_params(fvh_vgicp* h, const fvh_engine_params* p);
/* fast_gicp::VoxelAccumulationMode (gicp_settings.hpp:10) of the CPU FastVGICP (setVoxelAccumulationMode, fast_vgicp_impl.hpp:41-43;
 * the CUDA core only has the additive voxel): ADDITIVE / ADDITIVE_WEIGHTED -> AdditiveGaussianVoxel (fast_vgicp_voxel.hpp:105-122),
 * MULTIPLICATIVE -> MultiplicativeGaussianVoxel (:79-103: sum of C^-1 and C^-1 p, inverted at finalize). Takes effect at the next map build. */
enum fvh_voxel_accumulation_mode { FVH_VOXEL_ADDITIVE = 0, FVH_VOXEL_ADDITIVE_WEIGHTED = 1, FVH_VOXEL_MULTIPLICATIVE = 2 };
/* `mode` of a map snapshot taken from an NDT handle (fvh_ndt_voxelmap_export): its sums are {sum p, sum p p^T, count}. Never a voxel
 * accumulation mode of a VGICP handle, whose snapshots carry 0 or 2. */
enum { FVH_VOXEL_NDT_SUMS = 3 };
int fvh_vgicp_set_voxel_accumulation_mode(fvh_vgicp* h, int mode);

int fvh_vgicp_swap_source_and_target(fvh_vgicp* h);                                          /* [VC]:44, [VCU]:97-107 */
int fvh_vgicp_set_source_cloud(fvh_vgicp* h, const float* xyz, int n);                       /* [VC]:45 */
int fvh_vgicp_set_target_cloud(fvh_vgicp* h, const float* xyz, int n);                       /* [VC]:46 */
/* same from a HOST array of points `stride_floats` (3 or 4) floats apart -- e.g. &cloud->points[0].x of a pcl::PointCloud<pcl::PointXYZ>
 * (16-byte points): the PointT -> Vector3f repack of fast_vgicp_cuda_impl.hpp:87-90,116-119 disappears */
int fvh_vgicp_set_source_cloud_strided(fvh_vgicp* h, const float* xyz, int n, int stride_floats);
int fvh_vgicp_set_target_cloud_strided(fvh_vgicp* h, const float* xyz, int n, int stride_floats);
/* same, but the cloud is already in device memory (stride_floats = 3 or 4); D2D copy on the handle's stream */
int fvh_vgicp_set_source_cloud_device(fvh_vgicp* h, const float* d_xyz, int n, int stride_floats);
int fvh_vgicp_set_target_cloud_device(fvh_vgicp* h, const float* d_xyz, int n, int stride_floats);

int fvh_vgicp_set_source_neighbors(fvh_vgicp* h, int k, const int* neighbors /* n*k */);     /* [VC]:48 */
int fvh_vgicp_set_target_neighbors(fvh_vgicp* h, int k, const int* neighbors);               /* [VC]:49 */
int fvh_vgicp_find_source_neighbors(fvh_vgicp* h, int k);                                    /* [VC]:50 brute-force k-NN incl. self */
int fvh_vgicp_find_target_neighbors(fvh_vgicp* h, int k);                                    /* [VC]:51 */

int fvh_vgicp_calculate_source_covariances(fvh_vgicp* h, int regularization);                /* [VC]:53 */
int fvh_vgicp_calculate_target_covariances(fvh_vgicp* h, int regularization);                /* [VC]:54 */
int fvh_vgicp_calculate_source_covariances_rbf(fvh_vgicp* h, int regularization);            /* [VC]:56 */
int fvh_vgicp_calculate_target_covariances_rbf(fvh_vgicp* h, int regularization);            /* [VC]:57 */
/* new: inject covariances computed elsewhere (9 doubles per point, symmetric, any major) */
int fvh_vgicp_set_source_covariances(fvh_vgicp* h, const double* covs9);
int fvh_vgicp_set_target_covariances(fvh_vgicp* h, const double* covs9);

int fvh_vgicp_get_num_source_points(const fvh_vgicp* h, int* n);
int fvh_vgicp_get_num_target_points(const fvh_vgicp* h, int* n);
int fvh_vgicp_get_source_neighbors(fvh_vgicp* h, int* k, int* neighbors /* n*k, may be NULL to query k */);
int fvh_vgicp_get_target_neighbors(fvh_vgicp* h, int* k, int* neighbors);
int fvh_vgicp_get_source_covariances(fvh_vgicp* h, float* covs9);                            /* [VC]:59 */
int fvh_vgicp_get_target_covariances(fvh_vgicp* h, float* covs9);                            /* [VC]:60 */
int fvh_vgicp_get_num_voxels(fvh_vgicp* h, int* num_voxels);
int fvh_vgicp_get_voxel_num_points(fvh_vgicp* h, int* num_points);                           /* [VC]:62 */
int fvh_vgicp_get_voxel_means(fvh_vgicp* h, float* means3);                                  /* [VC]:63 */
int fvh_vgicp_get_voxel_covs(fvh_vgicp* h, float* covs9);                                    /* [VC]:64 */
int fvh_vgicp_get_voxel_coords(fvh_vgicp* h, int* coords3);                                  /* new (same order as the three above) */
int fvh_vgicp_get_num_correspondences(fvh_vgicp* h, int* n);
int fvh_vgicp_get_voxel_correspondences(fvh_vgicp* h, int* pairs /* n*2: (source index, voxel index in getter order) */); /* [VC]:65 */

int fvh_vgicp_create_target_voxelmap(fvh_vgicp* h);                                          /* [VC]:67 */
int fvh_vgicp_update_correspondences(fvh_vgicp* h, const double* T16);                       /* [VC]:69 */
/* [VC]:71 -- H36/b6 may both be NULL (error only).  Reuses the correspondences and the
 * linearisation rotation of the last update_correspondences(). */
int fvh_vgicp_compute_error(fvh_vgicp* h, const double* T16, double* H36, double* b6, double* error);

/* new: the whole LsqRegistration::computeTransformation loop (lsq_registration_impl.hpp:53-168) on the device.
 * Normally ONE persistent kernel launch per call (every LM transition is a trip through an in-kernel barrier; the
 * result comes back through mapped pinned memory, result->num_launches == 1); one launch per LM transition when a
 * RCCL communicator is attached, when another handle of the process is aligning at the same moment, for > 4 M voxel
 * lookups per evaluation, or after the barrier watchdog aborted a persistent launch (FVH_PERSISTENT=0 forces it).
 * All routes produce bit-identical results. */
int fvh_vgicp_align(fvh_vgicp* h, const double* guess16, const fvh_lm_params* params, fvh_lm_result* result);
/* new: K independent LM problems (the same clouds, K initial guesses) in one launch. results[k] equals, bit for bit,
 * fvh_vgicp_align(h, guesses16 + 16 k, params) on a handle whose cost_max_blocks is grid_blocks_out (K = 1: plain align, default plan).
 * 1 <= k <= 64; guesses column-major, finite. grid_blocks_out may be NULL.
 * Each hypothesis runs in its own gang of grid_blocks_out workgroups with its own LM state; all K share the prepared source, its
 * covariances and the target voxel map. One persistent launch when the K gangs fit the co-resident workgroup slots together (the gangs
 * shrink to fit, down to 8 workgroups), else one launch per LM transition over all K gangs; an aborted persistent launch is redone on
 * that route with the same plan. Afterwards the handle is where `for k: fvh_vgicp_align(guess k)` leaves it (linearisation pose and
 * correspondences of hypothesis K-1: a later compute_error / align gives the same bits either way). The LM debug trace is not recorded.
 * Refused: multi-GPU handles (FVH_ERR_UNSUPPORTED), an align_async in flight (FVH_ERR_BAD_STATE), k out of range, null pointers and
 * non-finite guesses (FVH_ERR_INVALID_ARGUMENT); the handle stays usable. FastGICP (nearest-point correspondences) has no multi call. */
int fvh_vgicp_align_multi(fvh_vgicp* h, int k, const double* guesses16, const fvh_lm_params* params,
                          fvh_lm_result* results, int* grid_blocks_out);
/* new: a scan stream as a two-stage pipeline (scan-to-scan odometry, src/kitti.cpp:95-128 / src/align.cpp:87-101 with the preparation of
 * scan k+1 hidden under the registration of scan k). The handle owns a SECOND stream and a prepared-source slot:
 *   fvh_vgicp_prepare_source_device  packs a device cloud into the slot and queues, on the second stream, the first `stages` stages of what
 *                                    the sequential loop runs for a new source: 1 = Morton order + exact k-NN (k), 2 = + covariances
 *                                    (rbf != 0: the RBF covariances instead of both; regularization as in
 *                                    fvh_vgicp_calculate_source_covariances), 3 = + the scan's own voxel map at the handle's resolution.
 *                                    Returns when everything is queued.
 *   fvh_vgicp_align_async / _wait    launch the LM kernel on the main stream / collect its result (together: fvh_vgicp_align). Between the
 *                                    two only fvh_vgicp_prepare_source_device may be called on this handle (anything else: FVH_ERR_BAD_STATE).
 *   fvh_vgicp_adopt_prepared_source  the slot becomes the source (stages = 1: the caller then calls fvh_vgicp_calculate_source_covariances);
 *                                    a map prepared with it travels with the cloud, and the next fvh_vgicp_swap_source_and_target makes
 *                                    that map the live one instead of building it ([VCU]:102-104's rebuild, already done).
 * The loop:  align_async; prepare_source_device(next scan); align_wait; swap_source_and_target; adopt_prepared_source.
 * The results are the sequential calls': with k-NN covariances bit for bit; RBF covariances are float sums in the cloud's spatial order, and a
 * cloud prepared beside a running LM kernel is ordered by the radix passes (a finer Morton key than the cooperative sort's, whose 1,024-thread
 * finish kernel fits on no CU that hosts LM workgroups): their last bits differ, poses agree to 1e-9. The bundled 17k pair: stages 2 is
 * best (+37 % registrations/s over the sequential loop), 3 and 1 within 4 % of it.
 * swap_source_and_target() on ANY handle now keeps the old target's map with its cloud: swapping back costs nothing, unless that cloud's
 * covariances changed after the map was built (then it is rebuilt, as the reference would).
 * Not on a multi-GPU handle (FVH_ERR_UNSUPPORTED). */
int fvh_vgicp_align_async(fvh_vgicp* h, const double* guess16, const fvh_lm_params* params);
int fvh_vgicp_align_wait(fvh_vgicp* h, fvh_lm_result* result);
int fvh_vgicp_prepare_source_device(fvh_vgicp* h, const float* d_xyz, int n, int stride_floats, int k, int regularization, int rbf, int stages);
int fvh_vgicp_prepare_source(fvh_vgicp* h, const float* xyz, int n, int stride_floats, int k, int regularization, int rbf, int stages); /* a HOST cloud, consumed before the call returns */
int fvh_vgicp_adopt_prepared_source(fvh_vgicp* h);
/* new: an INCREMENTAL target voxel map (scan-to-map odometry / mapping: align scan k against a local map, add scan k at the pose found,
 * drop what the vehicle left behind). The map keeps its per-voxel running sums, so adding a scan costs work proportional to the scan,
 * not to the map, and no target CLOUD is needed: align, align_async / _wait, align_multi, update_correspondences, compute_error, the
 * voxel getters and get_voxel_correspondences work on it as on a batch map.
 *   map_begin          start (or restart) an empty incremental map at the handle's resolution and voxel accumulation mode. expected_voxels
 *                      sizes the first table (<= 0: 16,384). Replaces whatever target map was live.
 *   map_insert_source  add the CURRENT SOURCE (points + covariances) at pose T (4x4 double column-major, rigid). Afterwards the map is the
 *                      map fvh_vgicp_create_target_voxelmap would build from the cloud of ALL points inserted so far, where an inserted
 *                      point is p' = (float)(T p) and its covariance C' = (float)(R C R^T), both formed in fp64 and rounded once: same voxel
 *                      set, same point counts exactly, means / covariances equal up to the order of the fp64 sums. MULTIPLICATIVE voxels
 *                      accumulate C'^-1 and C'^-1 p' of those rounded values. The source's Morton order is used when it has one.
 *   map_insert_cloud   the same for a cloud that is not the source: device or host points (stride 3 or 4 floats) + 9 doubles per point on
 *                      the host, as fvh_vgicp_set_*_covariances.
 *   map_prune          drop the voxels whose centre ((c + 1) * resolution per axis, fp64) is further than `radius` (Euclidean) from center3
 *                      (NULL: no distance rule), and those no insert has touched during the last max_age inserts (<= 0: no age rule;
 *                      1 keeps exactly what the last insert touched). A surviving voxel keeps its FULL sums. num_removed may be NULL.
 *   map_get_info       any pointer may be NULL. num_points counts the points offered since map_begin (skipped ones included);
 *                      num_dropped is the table-overflow counter and reads 0: capacity is secured BEFORE an insert launches, from a host-side
 *                      upper bound of the voxel count (the table grows by a rehash when needed), so no point is ever dropped and no
 *                      insert redone. Non-finite / out-of-range points are skipped and counted (fvh_vgicp_debug_get_skipped_points,
 *                      cumulative since map_begin).
 * Every insert and prune clears the stored correspondences (call update_correspondences / align again); a prune and a growing insert
 * are the only passes proportional to the map. A large map (fvh_engine_params::bitmap_min_points) keeps a correct occupancy bitmap:
 * new voxels inside its box set their bit, one outside switches it off until the next rehash (a prune, or an insert that grows the table)
 * rebuilds it -- a map that is never pruned and never grows then runs without a bitmap from that insert on (correct, slower on maps that no
 * longer fit the caches). The host keeps an upper bound of the voxel count that grows by the scan size per insert: when it says the table
 * could pass a load factor of 0.5, the insert first reads the real count back (one stream synchronisation; in the steady state of a
 * scan-to-map loop whose scans have more points than the map has voxels: every insert), and a prune reads its counts back as well.
 * While an incremental map is live: fvh_vgicp_create_target_voxelmap replaces it by the batch map of the target cloud (the mode ends; a call
 * refused because there is no target cloud / covariances leaves the incremental map as it was); fvh_vgicp_comm_init / _peer_attach are
 * FVH_ERR_BAD_STATE (every rank would grow a private map: end the mode first);
 * fvh_vgicp_swap_source_and_target / _gicp_swap_source_and_target are FVH_ERR_BAD_STATE (there is no cloud behind the map to become a
 * source); a change of the resolution or between additive and multiplicative voxels is FVH_ERR_BAD_STATE (call map_begin again);
 * fvh_vgicp_set_target_cloud* leaves the map alone (fvh_vgicp_fitness_score still needs a target cloud: fvh_vgicp_target_from_map below makes one of the map). With no incremental map live
 * all of those behave as before.
 * Refused by map_begin / map_insert_* / map_prune, the handle stays usable: multi-GPU handles (communicator, peers or tile attached) and
 * fvh_vgicp_set_target_map_sharding (FVH_ERR_UNSUPPORTED); FVH_COMPUTE_CUDA_COMPAT (FVH_ERR_UNSUPPORTED: its voxel sums are float sums in point order, which an in-place map
 * cannot reproduce); an align_async in flight, insert / prune without map_begin, a source without covariances (FVH_ERR_BAD_STATE); a
 * null or non-finite T (FVH_ERR_INVALID_ARGUMENT). NDT handles: fvh_ndt_map_* below. */
int fvh_vgicp_map_begin(fvh_vgicp* h, int expected_voxels);
int fvh_vgicp_map_insert_source(fvh_vgicp* h, const double* T16);
int fvh_vgicp_map_insert_cloud(fvh_vgicp* h, const float* xyz, int n, int stride_floats, const double* covs9, const double* T16, int on_device);
int fvh_vgicp_map_prune(fvh_vgicp* h, const double* center3, double radius, int max_age, int* num_removed);
int fvh_vgicp_map_get_info(fvh_vgicp* h, int* incremental, int* num_voxels, int* capacity, int* num_inserts, long long* num_points, int* num_dropped);
/* new: FREE-SPACE CARVING. The ray from the sensor to a measured point proves the voxels it crosses empty: a voxel written by a car, a
 * pedestrian or an opening door is removed by the next scan that sees through it, instead of staying until map_prune's distance or age rule
 * also takes the static structure around it. On the device: one 3D grid walk per ray, a sweep, and -- only if something goes -- the rehash
 * map_prune drives. The intended loop is align, clear_rays_source(T), map_insert_source(T).
 *   _source   the rays end at the handle's current source points (no covariances needed), walked in the source's Morton order when it has one.
 *   _cloud    ... at xyz: n points on the host or the device (on_device), stride_floats 3 or 4, as fvh_vgicp_map_insert_cloud takes them.
 *   T16       4x4 double column-major, scan frame -> map frame (R, t); origin3 the sensor origin in the SCAN frame, NULL = (0, 0, 0).
 *   min_range, max_range   metres; rays shorter / longer are skipped.  end_margin: metres in front of the endpoint the walk stops at.
 *   min_misses             a voxel goes when at least this many rays of THIS call crossed it and none ended in it.
 * end_margin and min_misses are the knobs against grazing rays eroding the ground: a ray that runs along a surface crosses the voxels of that
 * surface just before it ends; end_margin (a voxel or two) keeps the walk out of them, min_misses > 1 asks for several witnesses.
 * The contract (res = the map's resolution; voxel c covers grid coordinates [c, c + 1) per axis; the grid coordinate of a metric value x is
 * x / res - 0.5 in fp64, the expression an insert bins with):
 *   origin    o' = (float)(R o + t) per axis: ((r0 x + r1 y) + r2 z) + t in fp64, no product contracted into a sum, rounded once.
 *   endpoint  p'_i = (float)(R p_i + t): the bits an insert of the same point at the same pose bins, so a ray ends in the voxel the insert
 *             would put its point in.
 *   range     d_m = (double)p' - (double)o' per axis; r = sqrt((dx*dx + dy*dy) + dz*dz) in fp64, no product contracted into a sum.
 *   skipped   (not counted in *rays_used) when a coordinate of p_i is non-finite, r == 0, r < min_range, r > max_range, or the cell of o' or
 *             of p' is outside |c| < 2^20 - 4096.
 *   hit       with b the grid coordinate of p': the voxel floor(b) of every used ray is protected for this call if it exists.
 *   walk      (Amanatides-Woo, fp64) a = the grid coordinate of o', d = b - a, c = floor(a); per axis s = sign(d), tDelta = 1.0 / fabs(d),
 *             tMax = ((double)(c + 1) - a) / d for d > 0, (a - (double)c) / (-d) for d < 0, +inf for d == 0; t_end = 1.0 - end_margin / r;
 *             N = |dc_x| + |dc_y| + |dc_z| with dc = floor(b) - floor(a). t_in = 0; repeat: stop unless t_in < t_end; the current cell is
 *             CROSSED; stop if N steps have been taken; take the axis of the smallest tMax (ties: x before y before z): t_in = tMax[axis],
 *             c[axis] += s[axis], tMax[axis] += tDelta[axis]. One axis per step: at most N + 1 cells, never past the endpoint's cell.
 *   miss      every crossed cell that exists in the map gets its per-call counter incremented (an integer: order does not matter).
 *   removal   after all rays a voxel is removed iff misses >= min_misses and it is not protected. Survivors keep their full sums, their ages
 *             and their records, bit for bit.
 * Insert count and num_points are unchanged. When something was removed the table is rewritten by the rehash at the same capacity, the
 * bitmap rebuilt, stored correspondences cleared. When NOTHING was removed the map is not touched: no rehash, an export before and after is
 * byte-equal, stored correspondences are kept. *num_removed and *rays_used may be NULL; the call synchronises once to read its counts, as
 * map_prune does. The miss counters live for one call: nothing is added to the snapshot format (a hit / miss count kept across calls
 * is a different feature).
 * Refusals (the handle and its map stay as they were; host input is validated before anything is queued): no live incremental map, an
 * align_async in flight, _source without a source cloud (FVH_ERR_BAD_STATE); a NULL or non-finite T16, a non-finite origin3, min_range < 0
 * or NaN, max_range not finite or < min_range or > 4096 * res (one lane then walks at most 3 * 4097 = 12,291 cells), end_margin < 0 or
 * not finite, min_misses < 1, n < 0, NULL xyz with n > 0, a stride other than 3 or 4 (FVH_ERR_INVALID_ARGUMENT); multi-GPU handles
 * (communicator, peers, tile, map sharding) and FVH_COMPUTE_CUDA_COMPAT (FVH_ERR_UNSUPPORTED). n == 0: FVH_OK, nothing removed. */
int fvh_vgicp_clear_rays_source(fvh_vgicp* h, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, int* num_removed, int* rays_used);
int fvh_vgicp_clear_rays_cloud(fvh_vgicp* h, const float* xyz, int n, int stride_floats, int on_device, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, int* num_removed, int* rays_used);
/* new: SCORING a posed scan against the target voxel map, per point, on the device. How well does the map explain the scan at pose T: the
 * share of points that fall into occupied voxels (gtsam_points / GLIM: "overlap"), a likelihood (Autoware's NDT matcher: "transform
 * probability", "nearest voxel transformation likelihood"), and per point whether the map explains it or it is novel. The map is the handle's
 * CURRENT target voxel map, batch (create_target_voxelmap) or incremental (map_begin), of any accumulation mode and precision: the call reads
 * the voxel records {num_points, mean, covariance} and nothing else. It is point-to-distribution: source covariances play no part.
 *   _source   scores the handle's current source points (no covariances needed), walked in the source's Morton order when it has one.
 *   _cloud    ... xyz: n points on the host or the device (on_device), stride_floats 3 or 4.
 *   T16       4x4 double column-major, scan frame -> map frame (R, t).
 *   neighbors FVH_DIRECT1, FVH_DIRECT7 or FVH_DIRECT27: the voxels looked up around a point, independent of the handle's own search method.
 *   min_points  voxels with fewer points are not candidates (<= 1: every voxel).  max_m2: a point is EXPLAINED when its best squared
 *   Mahalanobis distance is finite and <= max_m2 (+inf allowed: every finite distance explains).  score_scale: the scores are exp(-0.5 * score_scale * m2).
 *   out       required.  found, best, best_m2: host arrays of n rows in INPUT order, each may be NULL; with all three NULL the call reads back
 *             sizeof(fvh_map_score) bytes and nothing else.
 * The contract (res = the map's resolution):
 *   point     p' = (float)(R p + t), the bits an insert of the same point at the same pose bins (the device expression of the insert and of
 *             clear_rays); c = floor((double)p' / res - 0.5) per axis. SKIPPED when a coordinate of p is non-finite or c is outside
 *             |c| < 2^20 - 4096: found = -1, best = -1, best_m2 = NaN, not counted in n_used.
 *   offsets   DIRECT1: (0,0,0). DIRECT7: (0,0,0), +x, -x, +y, -y, +z, -z. DIRECT27: dx outermost, then dy, then dz, each -1, 0, 1 (so
 *             (0,0,0) is index 13). `best` is an index into that order.
 *   candidate the voxel c + o when it lies inside the key range, exists in the map and its record's num_points >= min_points. A live
 *             occupancy bitmap may answer for absent cells first; the result is the same with and without it.
 *   distance  d = (double)p' - (double)mean per axis; the record's six covariance floats widened to fp64; then in fp64, every product and
 *             sum rounded on its own (no contraction):
 *               a00 = cyy*czz - cyz*cyz, a01 = cxz*cyz - cxy*czz, a02 = cxy*cyz - cxz*cyy,
 *               a11 = cxx*czz - cxz*cxz, a12 = cxy*cxz - cxx*cyz, a22 = cxx*cyy - cxy*cxy,
 *               det = (cxx*a00 + cxy*a01) + cxz*a02,
 *               q = (((dx*dx)*a00 + (dy*dy)*a11) + (dz*dz)*a22) + 2.0*((((dx*dy)*a01) + ((dx*dz)*a02)) + ((dy*dz)*a12)),
 *             m2 = q / det when det > 0 and det, q are finite (a negative quotient becomes 0), else m2 = +inf: a singular record counts as
 *             found and explains nothing.
 *   per point found = the number of candidates; best = the candidate with the smallest m2, the first in offset order on ties, -1 with
 *             found = 0; best_m2 = that m2, +inf with no candidate. score(m2) = exp((-0.5 * score_scale) * m2) by the fp64 device exp, 0 for
 *             m2 = +inf.
 *   sums      per point three fp64 terms at its INPUT index: best_m2 if explained (best_m2 < +inf and best_m2 <= max_m2); score(best_m2) if found > 0; the sum over its candidates,
 *             in offset order, of score(m2); 0 otherwise. Each array is summed in an order that depends on n alone (chunks of 16,384 entries;
 *             inside a chunk thread t of 1,024 takes entries t, t + 1,024, ... in four interleaved partial sums, then a fixed tree; the chunk
 *             sums the same way): two runs give the same bits, _source with or without a Morton order gives the same bits, _cloud of the same
 *             points gives the same bits. The counts are integers. No floating-point atomics.
 * Nothing of the handle is written: the map (an export before and after is byte-equal), stored correspondences, the linearisation pose, the
 * clouds and their Morton order (the call does not sort); an align after the call gives the bits it gave before. The scratch is the call's
 * own, so it is legal between prepare_source* and adopt_prepared_source, as target_from_map is. One exception: a batch map whose hint-sized
 * table had dropped points is rebuilt at the safe size first, as align, compute_error and the voxel getters do. The call synchronises once.
 * Refusals (the handle stays usable; host input is validated before anything is queued): no target voxel map, an align_async in flight,
 * _source without a source cloud (FVH_ERR_BAD_STATE); a NULL or non-finite T16, NULL out, neighbors other than the three above
 * (FVH_DIRECT_RADIUS too), max_m2 NaN or < 0, score_scale not finite or <= 0, n < 0, NULL xyz with n > 0, a stride other than 3 or 4
 * (FVH_ERR_INVALID_ARGUMENT); multi-GPU handles -- communicator, peers, tile, map sharding -- (FVH_ERR_UNSUPPORTED). n == 0: FVH_OK, all zeros. */
typedef struct fvh_map_score {
  int n_points;        /* rows offered */
  int n_used;          /* not skipped */
  int n_in_voxel;      /* used points whose OWN voxel (offset 0,0,0) is a candidate */
  int n_near;          /* used points with at least one candidate among the offsets */
  int n_explained;     /* ... whose best squared Mahalanobis distance is finite and <= max_m2 */
  double sum_best_m2;  /* over explained points */
  double sum_score_max;/* over near points: exp(-0.5 * score_scale * best m2) */
  double sum_score_all;/* over used points: sum over candidates of exp(-0.5 * score_scale * m2) */
} fvh_map_score;
int fvh_vgicp_score_source(fvh_vgicp* h, const double* T16, int neighbors, int min_points, double max_m2, double score_scale, fvh_map_score* out, int* found, int* best, double* best_m2);
int fvh_vgicp_score_cloud(fvh_vgicp* h, const float* xyz, int n, int stride_floats, int on_device, const double* T16, int neighbors, int min_points, double max_m2, double score_scale, fvh_map_score* out, int* found, int* best, double* best_m2);
/* new: RAY CASTING into the target voxel map: the first hit per ray, on the device. Every call above asks a question about a measured point;
 * this one asks the map what a sensor at a pose should see along a ray (OctoMap: castRay; NDT-OM: the maximum-likelihood point along a ray):
 * a predicted scan or depth image of the map, change detection BEFORE carving (the expected range against the measured one: a surface in
 * front of a return is what clear_rays will delete), occlusion and visibility tests, a localisation check that does not use the scan's own
 * points. A walk that stopped at the first occupied CELL would give ranges quantised to the voxel size; here the hit test uses the voxel's
 * Gaussian: inside each occupied cell the ray's point of smallest squared Mahalanobis distance to the Gaussian is found in closed form, and
 * the cell is a hit only if that distance is <= max_m2. The map is the handle's CURRENT target voxel map, batch or incremental, of any
 * accumulation mode and precision: the call reads the voxel records {num_points, mean, covariance} and nothing else.
 *   A ray is the SEGMENT from the sensor origin to an endpoint row, exactly the segments clear_rays_* walks (a caller with directions passes
 *   origin + length * unit direction).
 *   _source   the endpoints are the handle's current source points (no covariances needed), walked in the source's Morton order when it has one.
 *   _cloud    ... xyz: n points on the host or the device (on_device), stride_floats 3 or 4.
 *   T16       4x4 double column-major, scan frame -> map frame (R, t); origin3 the sensor origin in the SCAN frame, NULL = (0, 0, 0).
 *   min_range metres: it does NOT skip a ray, it bounds where a hit may lie (t_lo below).  max_range: metres; longer rays are skipped.
 *   min_points  voxels with fewer points are not candidates (<= 1: every voxel).  max_m2: the hit bound (+inf allowed).
 *   out       required.  hit, cell3 (3 int per row), range, m2: host arrays of n rows in INPUT order, each may be NULL; with all four NULL the
 *             call reads back sizeof(fvh_ray_cast) bytes and nothing else.
 * The contract (res = the map's resolution; everything fp64 unless stated; no product is contracted into a sum anywhere):
 *   origin, endpoint, range   word for word those of clear_rays_*: o' = (float)(R o + t), p' = (float)(R p + t), d_m = (double)p' - (double)o'
 *             per axis, r = sqrt((dx*dx + dy*dy) + dz*dz).
 *   skipped   when a coordinate of p is non-finite, r == 0, r > max_range, or the cell of o' or of p' is outside |c| < 2^20 - 4096.
 *             t_lo = min_range / r.
 *   walk      that of clear_rays_* with end_margin = 0: the same a, b, d, tMax, tDelta, tie order (x before y before z) and N; a cell is
 *             visited only while t_in < 1.0. Every visited cell has a parameter interval: t_in = 0 for the first cell, otherwise the tMax
 *             value the step into the cell took; t_out = min(the smallest tMax on leaving, 1.0), or 1.0 for the cell visited after N steps.
 *             At most N + 1 cells, in walk order; the walk ends at the first hit.
 *   candidate a visited cell that exists in the map, whose record's num_points >= min_points, and with t_out > t_lo. A live occupancy
 *             bitmap may answer for absent cells first; the result is the same with and without it. lo = max(t_in, t_lo).
 *   closest approach   e = (double)o' - (double)mean per axis; the record's six covariance floats widened to fp64; the adjugate terms
 *             a00 .. a22 and det of the score_* contract above; the bilinear form
 *               B(u, v) = (((ux*vx)*a00 + (uy*vy)*a11) + (uz*vz)*a22) + ((((ux*vy + uy*vx)*a01) + ((ux*vz + uz*vx)*a02)) + ((uy*vz + uz*vy)*a12)),
 *             den = B(d_m, d_m), num = B(d_m, e). The record is SINGULAR for this ray if det is not > 0 or not finite, den is not > 0 or not
 *             finite, or num is not finite: then s = lo and m2 = +inf. Otherwise s* = (-num) / den; s = lo if s* < lo, t_out if
 *             s* > t_out, else s*; x = e + s * d_m per axis (the product, then the sum); m2 = the score_* quotient form of x (q / det, a
 *             negative quotient 0, +inf when q is not finite).
 *   hit       the first candidate in walk order with m2 <= max_m2 (+inf <= +inf holds: with max_m2 = +inf the first candidate cell stops
 *             the ray, a singular one at its entry; with a finite bound singular records are passed through).
 *   per ray   hit: hit = 1, cell3 = the hit cell, range = s * r, m2 = that m2.  used, no hit: 0, (0, 0, 0), +inf, +inf.  skipped: -1,
 *             (0, 0, 0), NaN, NaN.
 * The counts are integers (order does not matter); no floating-point atomics. Nothing of the handle is written: the map (an export before and
 * after is byte-equal), stored correspondences, the clouds and their Morton order; an align after the call gives the bits it gave before. The
 * scratch is the call's own, so it is legal between prepare_source* and adopt_prepared_source. One exception, as for score_*: a batch map
 * whose hint-sized table had dropped points is rebuilt at the safe size first. The call synchronises once.
 * Refusals (the handle stays usable; host input is validated before anything is queued): no target voxel map, an align_async in flight,
 * _source without a source cloud (FVH_ERR_BAD_STATE); a NULL or non-finite T16, a non-finite origin3, NULL out, min_range < 0 or NaN,
 * max_range not finite or < min_range or > 4096 * res (one lane then walks at most 3 * 4097 = 12,291 cells), max_m2 NaN or < 0, n < 0, NULL
 * xyz with n > 0, a stride other than 3 or 4 (FVH_ERR_INVALID_ARGUMENT); multi-GPU handles -- communicator, peers, tile, map sharding --
 * (FVH_ERR_UNSUPPORTED). n == 0: FVH_OK, all zeros. */
typedef struct fvh_ray_cast {
  int n_rays;         /* rows offered */
  int n_used;         /* not skipped */
  int n_hit;          /* used rays with a hit */
  int n_hit_at_origin;/* ... whose hit is in the origin's own cell (the sensor sits inside map matter) */
  long long n_cells;  /* cells visited over all used rays, the hit cell included (integer: order does not matter) */
} fvh_ray_cast;
int fvh_vgicp_cast_rays_source(fvh_vgicp* h, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2);
int fvh_vgicp_cast_rays_cloud(fvh_vgicp* h, const float* xyz, int n, int stride_floats, int on_device, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2);
/* Snapshots of the live incremental map: write it out, bring it back, add another map to it.
 * A snapshot is a header -- resolution, mode (0 additive, 2 multiplicative), num_inserts (the map's insert count), num_points, num_voxels --
 * and per voxel coords[3] (int32), sums[10] (fp64: {sum p | sum C^-1 p (3), sum C | sum C^-1 (6), count}, the device's own sums) and an age
 * (inserts since the voxel was last touched; 0 = the last insert touched it). Rows come in ascending packed-key order (z-major, then y,
 * then x), so two snapshots of equal maps are byte-equal.
 *   _export: fills the header fields that are not NULL; coords3 / sums10 / ages (num_voxels rows; all three or none) receive the rows. Call it
 *            with the arrays NULL first to learn num_voxels.
 *   _import: ADDS n rows into the live map (restore = fvh_vgicp_map_begin + _import): a key already present gets sums += incoming (all ten,
 *            the count included; a key listed twice adds twice), a new key is created; the map's insert count becomes max(own, num_inserts),
 *            a voxel's last-touched stamp max(own, new insert count - age), num_points adds. fvh_vgicp_map_prune(max_age) then means on a
 *            restored map what it meant on the original. Capacity is secured before the launch: nothing is dropped. ages may be NULL (all 0).
 *   _merge_from: the same with the rows read in place from `other`'s live map, device to device; `other` is unchanged. A merged voxel has
 *            the smaller of its two ages. Both streams are ordered around the read (a later insert into `other` cannot race it).
 * With unique keys every sum receives exactly one fp64 add: the result is own + incoming to the bit, whatever the order.
 * Refusals (the handle and its map stay as they were; host input is validated before anything is queued): no live incremental map, or an
 * align_async in flight on either handle (FVH_ERR_BAD_STATE); resolution (bit-equal double) or mode different from the live map's, n < 0,
 * NULL arrays with n > 0, |coordinate| >= 2^20 - 4096, a non-finite sum, a count that is not an integer >= 1, an age >= num_inserts,
 * other == h, handles on different devices (FVH_ERR_INVALID_ARGUMENT); multi-GPU handles (communicator / peers / tile / map sharding),
 * FVH_COMPUTE_CUDA_COMPAT, more than 2^28 voxels (FVH_ERR_UNSUPPORTED). */
int fvh_vgicp_voxelmap_export(fvh_vgicp* h, int* num_voxels, double* resolution, int* mode, int* num_inserts, long long* num_points, int* coords3, double* sums10, unsigned* ages);
int fvh_vgicp_voxelmap_import(fvh_vgicp* h, int n, const int* coords3, const double* sums10, const unsigned* ages, double resolution, int mode, int num_inserts, long long num_points);
int fvh_vgicp_voxelmap_merge_from(fvh_vgicp* h, fvh_vgicp* other);
/* new: a map built in ANOTHER frame added into this one (submaps fused after pose-graph optimisation, a second session registered against
 * the first), and the live map re-anchored in place (a vehicle-centred map that moves, a loop-closure correction) -- on the device, one pass.
 * T16: 4x4 double, column-major, mapping `other`'s frame into h's; finite and rigid by the rule fvh_voxelgrid_deskew applies to a knot
 * pose (last row (0,0,0,1) to 1e-9, |R^T R - I| <= 1e-6 entrywise, det R > 0).
 *   posed_merge_from: every row {key, s[0..9], age} of `other`'s live map is transformed in fp64 (R, t from T16; n = s[9]; the six stored
 *            entries of a symmetric result are its upper triangle xx xy xz yy yz zz):
 *              additive (snapshot mode 0)        sp' = R sp + n t;   SC' = R SC R^T;                                          n' = n
 *              multiplicative (mode 2)           A'  = R A R^T;      b'  = R b + A' t;                                        n' = n
 *              NDT sums (mode 3), u = R sp       sp' = u + n t;      S'  = R S R^T + u t^T + t u^T + n t t^T;                 n' = n
 *            and added into the voxel of ITS OWN float32 mean: m' = the mean the voxel record arithmetic gives the transformed sums alone
 *            (additive / NDT: (float)(sp' * (1 / n)); multiplicative: (float)(A'^-1 b')), coord = floor((double)m' / resolution - 0.5) per
 *            axis, exactly as an inserted point is binned. The voxel is created if absent; several rows may land in one voxel and their
 *            sums add; stamp = max(own, new insert count - age) as _merge_from. A row whose coord leaves |c| < 2^20 - 4096 is skipped:
 *            counted in *rows_skipped (may be NULL; non-NULL costs one int read back and a stream synchronisation) and its point count added
 *            to the skipped-point counter (fvh_vgicp_debug_get_skipped_points). Bookkeeping as _merge_from: insert count max(own, other's),
 *            num_points += other's (skipped rows included), capacity secured before the launch (num_dropped stays 0), stored
 *            correspondences cleared, the occupancy bitmap follows the insert rule, both streams ordered around the read, `other` unchanged.
 *   transform_map: re-anchors h's live map by T16 in place; the result is what fvh_vgicp_map_begin on a fresh handle followed by
 *            posed_merge_from(fresh, h, T16) would hold. Insert count, num_points, every row's age, resolution and mode stay; the table is
 *            rewritten into its other buffer set (a pass proportional to the map, like a rehash) and the bitmap rebuilt; stored
 *            correspondences are cleared. A target cloud made earlier by fvh_vgicp_target_from_map is a snapshot and stays as it was.
 * This re-bins voxel GAUSSIANS, not points: a voxel of `other` goes where its mean goes. The result is therefore not the map of the
 * re-inserted points, voxels may fuse (never split), and merge(T) followed by merge(T^-1) is not the identity. Conserved exactly in the
 * algebra above: counts, first moments (sum p' = R sum p + n t) and covariance sums. Numerically each output sum is within a few dozen
 * 2^-53 of the same formulas evaluated with |R|, |t|, |sums| (tests/posedmerge_ref.py). For NDT the covariance recomputed from S' is
 * analytically R C R^T, but S' holds n |m'|^2-sized terms that cancel in it: its absolute fp64 error grows with n |m'|^2 2^-53, as for
 * any NDT voxel far from the origin.
 * Refusals (the handle, its map and `other` stay as they were; host input is validated before anything is queued): NULL other or T16, a
 * non-finite or non-rigid T16, other == h (use transform_map), resolution (bit-equal double) or mode different, handles on different
 * devices (FVH_ERR_INVALID_ARGUMENT); no live incremental map on either handle, an align_async in flight on either handle
 * (FVH_ERR_BAD_STATE); multi-GPU handles, FVH_COMPUTE_CUDA_COMPAT, more than 2^28 voxels (FVH_ERR_UNSUPPORTED). */
int fvh_vgicp_posed_merge_from(fvh_vgicp* h, fvh_vgicp* other, const double* T16, int* rows_skipped);
int fvh_vgicp_transform_map(fvh_vgicp* h, const double* T16, int* rows_skipped);
/* new: the live incremental map as the handle's TARGET CLOUD -- what fvh_vgicp_fitness_score, fvh_vgicp_gicp_* (FastGICP), find_target_neighbors
 * and debug_get_spatial_order(which = 1) need and a map does not have. Made on the device (select, radix sort by key, gather), nothing
 * crosses PCIe but one 32-byte readback.
 *   target_from_map    the target cloud becomes ONE POINT PER VOXEL of the live map that holds at least min_points points (<= 1: every
 *                      voxel): the point is the voxel's float mean, bit for bit what fvh_vgicp_get_voxel_means returns, and its covariance
 *                      -- stored as the target covariances: fvh_vgicp_get_target_covariances returns it -- the voxel's record covariance,
 *                      bit for bit what fvh_vgicp_get_voxel_covs returns. Rows come in ascending packed-key order (z-major, then y, then x:
 *                      the row order of fvh_vgicp_voxelmap_export; with min_points <= 1 index i IS row i of an export), so two handles that
 *                      hold equal maps hold bit-identical target clouds and the target indices of fvh_vgicp_gicp_get_correspondences mean
 *                      the same on both. *num_points_out (may be NULL) receives the number of points; the call reads that count back either
 *                      way (the size of a cloud is host state): one readback, one stream synchronisation. If no voxel qualifies the
 *                      count is 0 and the handle has NO target cloud (fitness_score: FVH_ERR_BAD_STATE, as without one).
 *   get_target_points  packed xyz (fvh_vgicp_get_num_target_points rows) of the current target cloud in its ORIGINAL order, however it was
 *                      set; FVH_ERR_BAD_STATE without one.
 * A SNAPSHOT: a later insert, prune, import or merge leaves the target cloud as it was; call target_from_map again to refresh it. The map
 * is only read and stays live: align, update_correspondences, compute_error after the call run on the map and give the bits they gave
 * before; stored voxel correspondences are kept (stored nearest-point ones index the old cloud and are dropped). Whatever the target
 * cloud held before is replaced as by fvh_vgicp_set_target_cloud: points, covariances, neighbour lists, Morton order and tiles.
 * Refusals (the handle and its target cloud stay as they were): no live incremental map, an align_async in flight (FVH_ERR_BAD_STATE).
 * Legal between prepare_source* and adopt_prepared_source: the call uses scratch of its own, not the preparation's. */
int fvh_vgicp_target_from_map(fvh_vgicp* h, int min_points, int* num_points_out);
int fvh_vgicp_get_target_points(fvh_vgicp* h, float* xyz3);
/* setDebugPrint(true) on the device LM: with the trace on, an align records one row per trial step -- {inner iteration i, y0,
 * yi, rho, lambda, |d|}, the columns LsqRegistration prints (lsq_registration_impl.hpp:143-149) -- fetched afterwards
 * (rows6 may be NULL to query the count). */
int fvh_vgicp_set_lm_trace(fvh_vgicp* h, int on);
int fvh_vgicp_get_lm_trace(fvh_vgicp* h, int* num_rows, double* rows6);
/* new: pcl::Registration::getFitnessScore(max_range) -- mean squared exact-NN distance of
 * (float)T * source to the target cloud (exact tile-culled 1-NN on device, fixed-order fp64 sum: bit-reproducible). */
int fvh_vgicp_fitness_score(fvh_vgicp* h, const double* T16, double max_range, double* score);

/* ---- FastGICP on the device: nearest-target-point correspondences instead of voxels, on the same handle.
 * Reference: fast_gicp::FastGICP (CPU/OpenMP only), include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:
 *   update_correspondences :118-156 (query = trans.cast<float>() * p, exact 1-NN in the target, kept when the squared
 *   distance < corr_dist_threshold_^2; mahalanobis = (C_B + T C_A T^T)^-1), linearize :159-213, compute_error :216-240,
 *   setMaxCorrespondenceDistance = pcl::Registration (default float max, :18).
 * Needs both clouds and both covariance sets (calculate_*_covariances or set_*_covariances); no voxel map. ---- */
int fvh_vgicp_gicp_set_max_correspondence_distance(fvh_vgicp* h, double max_distance);
int fvh_vgicp_gicp_swap_source_and_target(fvh_vgicp* h);                                    /* fast_gicp_impl.hpp:56-62: swaps clouds, neighbours, covariances; no voxel map */
int fvh_vgicp_gicp_update_correspondences(fvh_vgicp* h, const double* T16);
int fvh_vgicp_gicp_compute_error(fvh_vgicp* h, const double* T16, double* H36, double* b6, double* error);
/* the whole FastGICP LM loop on the device: per LM transition one nearest-point search + one cost launch, no host round trip
 * (the search reads the pose of the next linearisation from the LM state on the device); same result struct as fvh_vgicp_align */
int fvh_vgicp_gicp_align(fvh_vgicp* h, const double* guess16, const fvh_lm_params* params, fvh_lm_result* result);
int fvh_vgicp_gicp_get_correspondences(fvh_vgicp* h, int* target_index_per_source_point /* num_source_points ints, -1 = none */);

/* new: per-kernel-class HIP-event timing on the handle's stream (for bench.py's roofline leg) */
int fvh_vgicp_profile_enable(fvh_vgicp* h, int on /* 0 off; 1 every kernel class; 2 the "cost" class only: two events per registration, the result still travels through mapped memory */);
int fvh_vgicp_profile_reset(fvh_vgicp* h);
/* kernel_class in {"cost", "knn", "cov", "rbf", "voxelmap", "fitness"}; sums over launches since reset */
int fvh_vgicp_profile_get(fvh_vgicp* h, const char* kernel_class, double* total_ms, int* launches);
int fvh_vgicp_synchronize(fvh_vgicp* h);
/* testing hooks: the bucket table is sized from the previous build's voxel count (4x, pow2); a wrong
 * hint must only cost a rebuild at the safe size (2 x N_t), never points. */
int fvh_vgicp_debug_set_voxel_hint(fvh_vgicp* h, int num_voxels);
int fvh_vgicp_debug_get_table_capacity(fvh_vgicp* h, int* capacity);
int fvh_vgicp_debug_get_skipped_points(fvh_vgicp* h, int* n);  /* target points of the current voxel map that belong to no voxel: non-finite or |coord| >= 2^20 voxels (they are skipped, never fatal) */
int fvh_vgicp_debug_get_persist_aborts(fvh_vgicp* h, int* n);  /* persistent-LM launches whose barrier watchdog fired (each was redone with one launch per LM transition) */
int fvh_vgicp_debug_get_persist_grid(fvh_vgicp* h, int* blocks, int* capacity);  /* workgroups of the last persistent-LM launch / co-resident workgroup capacity of the device for that kernel */
int fvh_debug_slot_pool(int device, int* reserved, int* active, int* recent);    /* the process-wide pool that splits those workgroup slots between concurrent aligns: all zero when nothing is in flight */
/* test hook: the device LM step (kernels_cost.hpp: dev_lm_step_wave -- LDL^T solve, se3_exp, the accept / reject / convergence machine of
 * lsq_registration_impl.hpp:53-168) replayed ALONE on sums the caller scripts. No cost kernel runs: on a stream of its own the call
 * initialises one LM state from guess16 (column-major, finite) and *params, then for step s = 0 .. n_steps - 1 copies sums[32 s .. 32 s + 31]
 * into the state where a cost evaluation would have left them, launches the one-wave update kernel the RCCL route runs between two
 * evaluations (the Gauss-Newton instantiation when params->optimizer != 0) and writes the state into rows[FVH_LM_REPLAY_ROW * s ...].
 * A row of sums: [0] error, [1..6] b, [7..12] H rot-rot (xx xy xz yy yz zz), [13..21] H rot-trans (3x3 row-major), [22..27] H trans-trans
 * (xx xy xz yy yz zz) of the linearisation this evaluation computed, [28] the trial error of a fused trial evaluation (a phase-6 trial, error
 * only, carries it at [0]), [29..31] zero.
 * A row of the result, all doubles:
 *   [0] phase (0 linearize, 1 trial, 2 done, 6 final trial) [1] outer_iter [2] inner_iter [3] converged [4] lm_failed
 *   [5] num_linearize [6] num_error_evals [7] nr_iterations [8] corr_cur [9] delta_converged
 *   [10] lambda [11] nu [12] y0 [13..18] d (the step proposed last)
 *   [19..30] x0, [31..42] xi, [43..54] x_lin: each the 9 rotation entries row-major, then the 3 translation entries
 *   [55..90] H (6x6, as the state holds it: row-major, symmetric) [91..96] b [97..132] final_H (6x6)
 * The replay stops once the state is done: *steps_run = steps taken (the last one is the step that ended the loop), rows beyond it are
 * left untouched. max_iterations <= 0: the state is done before any step -- *steps_run = 0 and rows[0 .. FVH_LM_REPLAY_ROW) holds the
 * initial state. Everything is freed before the call returns. FVH_ERR_INVALID_ARGUMENT: a null pointer, a non-finite guess, n_steps
 * outside 1..256 (checked before the device is touched). */
#define FVH_LM_REPLAY_ROW 133
int fvh_debug_lm_replay(int device, const double* guess16, const fvh_lm_params* params, int n_steps, const double* sums /* n_steps x 32 */,
                        double* rows /* n_steps x FVH_LM_REPLAY_ROW */, int* steps_run);
/* test hook: the symmetric 3x3 eigen solver and the covariance regulariser (dev_math.hpp: sym_eig3, regularize_cov -- what the k-NN and RBF
 * covariance kernels, the NDT voxel finalisation and the incremental NDT record run on every matrix) ALONE, in fp64 in and out: one thread per
 * matrix calls the two functions themselves, on a stream of its own. sym6: n x 6 {xx, xy, xz, yy, yz, zz}. w3: n x 3 eigenvalues, ascending.
 * V9: n x 9, row-major, eigenvectors in the COLUMNS (column j belongs to w3[j]). reg6: n x 6, regularize_cov(method) before any fp32 rounding
 * (method: the RegularizationMethod ordinal, 0 NONE .. 4 FROBENIUS). Everything is freed before the call returns.
 * FVH_ERR_INVALID_ARGUMENT: a null pointer, n < 1, a method outside 0..4, a non-finite entry (checked before the device is touched). The
 * solver's domain is finite matrices with 1e-100 <= |S|max <= 1e100 (or S = 0): DESIGN.md, "The eigen solver on its own". */
int fvh_debug_regularize(int device, int n, const double* sym6, int method, double* w3, double* V9, double* reg6);
/* persistent LM kernel, XCD-local hand-offs (kernels_cost.hpp): *wanted = 1 while the process still asks for them, *placement_aborts =
 * launches that ended because the dispatcher had not placed the workgroups of a group on one XCD (3 of those switch the flavour off) */
int fvh_debug_xcd_local(int* wanted, int* placement_aborts);
/* test hook: how many Morton sorts this process has queued on each route -- {cooperative kernel, one workgroup, two-launch radix passes,
 * four-launch radix passes}. (The cooperative kernel is a gang kernel: it is not used while ANOTHER registration handle has one in flight.) */
int fvh_debug_sort_routes(int* counts4);

/* new: multi-GPU over RCCL (one process per GPU). With a communicator attached a VGICP handle shards INTERNALLY, like the peer path below:
 * every rank makes the same calls on the same FULL clouds; neighbour search and covariance estimation run on the rank's spatial tile (a
 * range of the cloud's Morton order) and the 32 B / point covariances are all-gathered (ncclAllGather); every cost evaluation walks the
 * rank's tile of the source and the 32-double normal-equation block (err, b, H, trial error) is all-reduced (ncclAllReduce) on the
 * handle's stream; the LM step then runs redundantly on every rank. The target voxel map is replicated. (NDT handles: either the caller
 * hands each rank its shard of the source and only the all-reduce is the library's, or -- fvh_ndt_set_source_tile -- every rank holds the
 * full source and the engine walks the rank's spatial tile.) */
int fvh_comm_unique_id(void* id128 /* 128 bytes out */);
int fvh_vgicp_comm_init(fvh_vgicp* h, const void* id128, int nranks, int rank);
int fvh_vgicp_comm_destroy(fvh_vgicp* h);

/* new: multi-GPU without RCCL -- peer-mapped exchange regions (one process per GPU on one node; also handles of one process).
 * north_star: "large scans shard by spatial tile across up to 8 GPUs ... all-reduce of the 6x6/6x1 normal equations per
 * iteration".  With peers attached, every rank makes the SAME sequence of calls on the SAME full clouds and the engine shards
 * internally by spatial tile (= a range of the cloud's Morton order):
 *   find_*_neighbors / calculate_*_covariances[_rbf]: each rank computes its tile (the whole sorted cloud is the candidate set:
 *     an exact, implicit halo), then the tiles are all-gathered through the peers' staging areas -> every rank holds exactly
 *     the covariances one GPU would have computed (voxel map: built from them on every rank, replicated);
 *   update_correspondences / compute_error / align: each rank walks its tile of the source; the 32-double block {err, b, H} is
 *     exchanged through the peers' mailboxes INSIDE the cost kernel (every rank writes its block into every peer's mailbox over
 *     xGMI and sums in rank order -> bit-identical sums, the LM step runs redundantly, no broadcast): a sharded align is still
 *     ONE persistent launch per rank.  Measured mailbox round trip (two processes, one MI355X): 1.4 us.
 * peer_export: allocates the region (fine-grained device memory; staging for clouds of up to max_points) and returns its
 *   hipIpcMemHandle_t as 64 opaque bytes (+ the raw device pointer for peers living in the same process).
 * peer_attach: handles of all ranks in rank order (the own entry is ignored); process_local_ptrs[p] != 0 marks a peer of THIS
 *   process (its pointer is used directly, IPC cannot map one's own allocation); ranks_on_this_device: how many of the ranks
 *   share this GPU (their persistent grids share its co-resident workgroup slots).
 * A rank that does not arrive within the watchdog (2 s, FVH_PEER_WATCHDOG_TICKS) fails the call with FVH_ERR_COMM on every rank. */
int fvh_vgicp_peer_export(fvh_vgicp* h, int max_points, void* ipc_handle64 /* out */, unsigned long long* process_local_ptr /* out, may be NULL */);
int fvh_vgicp_peer_attach(fvh_vgicp* h, int nranks, int rank, int ranks_on_this_device, const void* ipc_handles /* nranks x 64 B, may be NULL if all peers are local */,
                          const unsigned long long* process_local_ptrs /* nranks entries or NULL */);
int fvh_vgicp_peer_detach(fvh_vgicp* h);
/* peer_attach refuses (FVH_ERR_COMM) a peer region on a device this one cannot reach (hipDeviceCanAccessPeer).
 * peer_selfcheck: COLLECTIVE -- every rank stores a nonce into every attached region and waits until every rank's nonce has arrived
 *   in its own (the path the in-kernel mailboxes take, over xGMI between devices); FVH_ERR_COMM + the bit mask of the ranks whose
 *   store never came after timeout_seconds (<= 0: 5 s). Call it once after attaching, before the first sharded registration. */
int fvh_vgicp_peer_selfcheck(fvh_vgicp* h, double timeout_seconds, int* missing_rank_mask /* out, may be NULL */);
/* Multi-GPU, either exchange (peers attached or a communicator): shard the TARGET voxel map too ("sharded by the same tiles +
 * halo"). With `on`, fvh_vgicp_align builds this rank's map from the target points around T_guess * (its spatial tile of the source) only:
 * the tile's bounding box in voxel coordinates, widened by the reach of the neighbour offsets (1 voxel for DIRECT7 / 27, ceil(r) for
 * DIRECT_RADIUS) + `margin_voxels` for the motion of the pose during the align. A voxel inside the box receives all its points: its record
 * is the replicated map's. If a source element leaves the inner box during the LM loop (the pose moved further than the margin allows)
 * the rank redoes that align on the full map. The map is rebuilt per align (it depends on the guess): meant for maps that should not be
 * replicated, not for speed. The host-driven calls (update_correspondences / compute_error / the voxel getters) use the replicated map:
 * after a sharded align they rebuild it (and the shard's correspondences die with it). */
int fvh_vgicp_set_target_map_sharding(fvh_vgicp* h, int on, int margin_voxels);
int fvh_vgicp_debug_get_map_shard(fvh_vgicp* h, int* live_map_is_a_shard, int* aligns_redone_on_the_full_map);
/* voxel count of the live map as the last align left it (a shard stays a shard). The voxel GETTERS (fvh_vgicp_get_num_voxels, get_voxel_*),
 * update_correspondences and compute_error always work on the WHOLE map: after a sharded align they rebuild it first. */
int fvh_vgicp_debug_get_live_map_voxels(fvh_vgicp* h, int* num_voxels);
/* test hook: the spatial (Morton) order of a cloud -- order[j] = original index of the j-th point of the sorted cloud (n ints) -- and the
 * boxes of its 64-point tiles (8 floats per tile: min xyz 0, max xyz 0). which: 0 source, 1 target. Sorts the cloud if it is not sorted yet.
 * No reference counterpart (the order is this engine's own device for culling the exact searches and for the multi-GPU tiles). */
int fvh_vgicp_debug_get_spatial_order(fvh_vgicp* h, int which, int* order, float* tile_boxes);

/* ---------------------------------------------------------------------------------------------
 * NDTCudaCore
 * ------------------------------------------------------------------------------------------- */
int fvh_ndt_create(int device, fvh_ndt** out);                                               /* [NC]:34-35, [NCU]:13-23 (D2D, DIRECT7, res 1.0) */
int fvh_ndt_destroy(fvh_ndt* h);
const char* fvh_ndt_last_error(const fvh_ndt* h);
int fvh_ndt_set_distance_mode(fvh_ndt* h, int mode);                                         /* [NC]:37 */
int fvh_ndt_set_resolution(fvh_ndt* h, double resolution);                                   /* [NC]:38 */
int fvh_ndt_set_neighbor_search_method(fvh_ndt* h, int method, double radius);               /* [NC]:39 */
int fvh_ndt_set_precision(fvh_ndt* h, int precision);
int fvh_ndt_get_engine_params(fvh_ndt* h, fvh_engine_params* out);
int fvh_ndt_set_engine_params(fvh_ndt* h, const fvh_engine_params* p);
int fvh_ndt_swap_source_and_target(fvh_ndt* h);                                              /* [NC]:41, [NCU]:90-93 */
int fvh_ndt_set_source_cloud(fvh_ndt* h, const float* xyz, int n);                           /* [NC]:42 (invalidates the source voxel map) */
int fvh_ndt_set_target_cloud(fvh_ndt* h, const float* xyz, int n);                           /* [NC]:43 */
int fvh_ndt_set_source_cloud_strided(fvh_ndt* h, const float* xyz, int n, int stride_floats);
int fvh_ndt_set_target_cloud_strided(fvh_ndt* h, const float* xyz, int n, int stride_floats);
int fvh_ndt_set_source_cloud_device(fvh_ndt* h, const float* d_xyz, int n, int stride_floats);
int fvh_ndt_set_target_cloud_device(fvh_ndt* h, const float* d_xyz, int n, int stride_floats);
int fvh_ndt_create_voxelmaps(fvh_ndt* h);                                                    /* [NC]:45 (lazy; source skipped in P2D) */
int fvh_ndt_create_target_voxelmap(fvh_ndt* h);                                              /* [NC]:46 */
int fvh_ndt_create_source_voxelmap(fvh_ndt* h);                                              /* [NC]:47 */
int fvh_ndt_update_correspondences(fvh_ndt* h, const double* T16);                           /* [NC]:49 */
int fvh_ndt_compute_error(fvh_ndt* h, const double* T16, double* H36, double* b6, double* error); /* [NC]:50 */
int fvh_ndt_align(fvh_ndt* h, const double* guess16, const fvh_lm_params* params, fvh_lm_result* result);
/* new: fvh_vgicp_align_multi for NDT (P2D and D2D), with the same contract against fvh_ndt_align. Also refused (FVH_ERR_UNSUPPORTED):
 * tiled handles (fvh_ndt_set_source_tile). */
int fvh_ndt_align_multi(fvh_ndt* h, int k, const double* guesses16, const fvh_lm_params* params,
                        fvh_lm_result* results, int* grid_blocks_out);
/* new: a frame stream as a two-stage pipeline (src/kitti.cpp:95-128 with the preparation of frame k+1 hidden under the registration of
 * frame k). The handle owns a SECOND stream and a prepared-source slot:
 *   fvh_ndt_align_async          launches the LM kernel on the main stream and returns; fvh_ndt_align_wait collects its result
 *                                (together they are fvh_ndt_align, bit for bit). Between the two, only fvh_ndt_prepare_source_device
 *                                (and a voxel-grid filter sharing the prepare stream) may be called on this handle.
 *   fvh_ndt_prepare_source_device widens a device cloud into the slot and (D2D) builds its voxel map there, all on the second stream;
 *                                returns when everything is queued.
 *   fvh_ndt_adopt_prepared_source the slot becomes the source (what set_source_cloud + the lazy map build of the next align would have
 *                                made: same kernels, same data, bit-identical maps); the main stream is ordered after the preparation.
 * The loop:  adopt; align_async; [filter next frame on the prepare stream; prepare_source_device]; align_wait; swap_source_and_target. */
int fvh_ndt_align_async(fvh_ndt* h, const double* guess16, const fvh_lm_params* params);
int fvh_ndt_align_wait(fvh_ndt* h, fvh_lm_result* result);
int fvh_ndt_prepare_source_device(fvh_ndt* h, const float* d_xyz, int n, int stride_floats);
int fvh_ndt_prepare_source(fvh_ndt* h, const float* xyz, int n, int stride_floats); /* the same for a HOST cloud, consumed before the call returns */
int fvh_ndt_adopt_prepared_source(fvh_ndt* h);
/* new: an INCREMENTAL NDT target map (scan-to-map localisation), the NDT counterpart of fvh_vgicp_map_* / fvh_vgicp_voxelmap_* above with
 * the same semantics call by call; what differs:
 *   - An NDT voxel is {sum p', sum p' p'^T, count} of the inserted points p' = (float)(T p) (formed in fp64, rounded once; the products are
 *     fp64 products of the float values): points only, no covariances -- fvh_ndt_map_insert_cloud takes none. After every insert the map is
 *     the map fvh_ndt_set_target_cloud(all p') + fvh_ndt_create_target_voxelmap would build: same voxel set, same counts exactly, means and
 *     (MIN_EIG-regularised) covariances recomputed from the sums, equal up to the order of the fp64 sums.
 *   - The map is the handle's TARGET map: fvh_ndt_get_voxels(h, 1, ...), update_correspondences, compute_error, align, align_multi,
 *     align_async / _wait and the prepare_source* pipeline read it unchanged, in both distance modes (D2D still builds its source map from
 *     the source cloud per frame), and none of them asks for a target cloud while it is live.
 *   - Snapshots carry mode = FVH_VOXEL_NDT_SUMS (3); file format and version are those of the VGICP snapshots. fvh_ndt_voxelmap_import
 *     refuses mode 0 / 1 / 2 and fvh_vgicp_voxelmap_import refuses mode 3 (FVH_ERR_INVALID_ARGUMENT): sums of different kinds never add.
 *   - While it is live: fvh_ndt_set_resolution to another value, fvh_ndt_swap_source_and_target, fvh_ndt_comm_init / _set_source_tile with
 *     nranks > 1 are FVH_ERR_BAD_STATE; FVH_COMPUTE_CUDA_COMPAT is FVH_ERR_UNSUPPORTED (set before or after map_begin); map_begin and the
 *     other map calls on a tiled / multi-GPU handle are FVH_ERR_UNSUPPORTED; fvh_ndt_fitness_score still needs a target cloud.
 *     fvh_ndt_set_target_cloud* leaves the map alone but marks the cloud as newer: the next fvh_ndt_create_target_voxelmap /
 *     _create_voxelmaps -- fvh_ndt_align and _align_multi make that call themselves -- builds the batch map of that cloud and the mode ends
 *     (a target cloud set BEFORE map_begin stays beside the map, e.g. for fitness_score). Every refusal leaves the handle usable. */
int fvh_ndt_map_begin(fvh_ndt* h, int expected_voxels);
int fvh_ndt_map_insert_source(fvh_ndt* h, const double* T16);
int fvh_ndt_map_insert_cloud(fvh_ndt* h, const float* xyz, int n, int stride_floats, const double* T16, int on_device);
int fvh_ndt_map_prune(fvh_ndt* h, const double* center3, double radius, int max_age, int* num_removed);
int fvh_ndt_map_get_info(fvh_ndt* h, int* incremental, int* num_voxels, int* capacity, int* num_inserts, long long* num_points, int* num_dropped);
/* free-space carving, as fvh_vgicp_clear_rays_source / _cloud above, argument for argument and under the same contract */
int fvh_ndt_clear_rays_source(fvh_ndt* h, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, int* num_removed, int* rays_used);
int fvh_ndt_clear_rays_cloud(fvh_ndt* h, const float* xyz, int n, int stride_floats, int on_device, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, int* num_removed, int* rays_used);
/* a posed scan scored against the target voxel map, as fvh_vgicp_score_source / _cloud above, argument for argument and under the same contract */
int fvh_ndt_score_source(fvh_ndt* h, const double* T16, int neighbors, int min_points, double max_m2, double score_scale, fvh_map_score* out, int* found, int* best, double* best_m2);
int fvh_ndt_score_cloud(fvh_ndt* h, const float* xyz, int n, int stride_floats, int on_device, const double* T16, int neighbors, int min_points, double max_m2, double score_scale, fvh_map_score* out, int* found, int* best, double* best_m2);
/* rays cast into the target voxel map, as fvh_vgicp_cast_rays_source / _cloud above, argument for argument and under the same contract */
int fvh_ndt_cast_rays_source(fvh_ndt* h, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2);
int fvh_ndt_cast_rays_cloud(fvh_ndt* h, const float* xyz, int n, int stride_floats, int on_device, const double* T16, const double* origin3, double min_range, double max_range, int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2);
int fvh_ndt_voxelmap_export(fvh_ndt* h, int* num_voxels, double* resolution, int* mode, int* num_inserts, long long* num_points, int* coords3, double* sums10, unsigned* ages);
int fvh_ndt_voxelmap_import(fvh_ndt* h, int n, const int* coords3, const double* sums10, const unsigned* ages, double resolution, int mode, int num_inserts, long long num_points);
int fvh_ndt_voxelmap_merge_from(fvh_ndt* h, fvh_ndt* other);
/* as fvh_vgicp_posed_merge_from / fvh_vgicp_transform_map, argument for argument, with the NDT row of their table of sums */
int fvh_ndt_posed_merge_from(fvh_ndt* h, fvh_ndt* other, const double* T16, int* rows_skipped);
int fvh_ndt_transform_map(fvh_ndt* h, const double* T16, int* rows_skipped);
/* new: the live incremental NDT map as the handle's target cloud, as fvh_vgicp_target_from_map / _get_target_points above: one point per
 * voxel with >= min_points points (the float mean fvh_ndt_get_voxels(h, 1, ...) returns, bit for bit), rows in ascending packed-key order,
 * a snapshot. POINTS ONLY (an NDT handle keeps no target covariances). The map stays the target map and stays live: the call does NOT mark
 * the cloud as newer than the map -- that is fvh_ndt_set_target_cloud*'s rule; a cloud such a call left behind is replaced, so nothing is
 * newer afterwards -- and fvh_ndt_align after it runs on the incremental map, bit for bit as before; stored correspondences are kept.
 * FVH_ERR_BAD_STATE without a live incremental map or with an align_async in flight. */
int fvh_ndt_target_from_map(fvh_ndt* h, int min_points, int* num_points_out);
int fvh_ndt_get_num_source_points(const fvh_ndt* h, int* n); /* points of the current source cloud (the rows fvh_ndt_score_source writes): 0 without one */
int fvh_ndt_get_num_target_points(const fvh_ndt* h, int* n); /* rows of fvh_ndt_get_target_points: 0 without a target cloud */
int fvh_ndt_get_target_points(fvh_ndt* h, float* xyz3);
/* new (round 6): the output of the filter's last ApproximateVoxelGrid call becomes the cloud WITHOUT a copy -- the filter's emit kernel wrote it as
 * float4 too, and that buffer is swapped with the cloud's (what fvh_voxelgrid_device_points + fvh_ndt_set_source_cloud_device /
 * _prepare_source_device do, minus the widening kernel and its launch: 8 of a LiDAR frame's 141 us). An output can be taken once; the filter's
 * packed xyz (fvh_voxelgrid_get_points / _device_points) stays valid. The streams of the two handles are ordered if they differ. */
struct fvh_voxelgrid;
int fvh_ndt_set_source_cloud_from_voxelgrid(fvh_ndt* h, struct fvh_voxelgrid* filter);
int fvh_ndt_set_target_cloud_from_voxelgrid(fvh_ndt* h, struct fvh_voxelgrid* filter);
int fvh_ndt_prepare_source_from_voxelgrid(fvh_ndt* h, struct fvh_voxelgrid* filter);
int fvh_ndt_fitness_score(fvh_ndt* h, const double* T16, double max_range, double* score);
/* testing hook (as fvh_vgicp_debug_set_voxel_hint): table size hint of the NEXT build of the source (which = 0) / target (1) voxel map */
int fvh_ndt_debug_set_voxel_hint(fvh_ndt* h, int which, int num_voxels);
/* testing hook (as fvh_vgicp_debug_get_table_capacity): buckets of the current source (which = 0) / target (1) voxel table */
int fvh_ndt_debug_get_table_capacity(fvh_ndt* h, int which, int* capacity);
int fvh_ndt_debug_get_skipped_points(fvh_ndt* h, int* n);  /* as fvh_vgicp_debug_get_skipped_points, of the target map: points (and the points of posed-merge rows) that belong to no voxel */
int fvh_ndt_set_lm_trace(fvh_ndt* h, int on);
int fvh_ndt_get_lm_trace(fvh_ndt* h, int* num_rows, double* rows6);
int fvh_ndt_get_num_voxels(fvh_ndt* h, int which /* 0 source, 1 target */, int* num_voxels);
int fvh_ndt_get_voxels(fvh_ndt* h, int which, int* coords3, int* num_points, float* means3, float* covs9);
int fvh_ndt_get_num_correspondences(fvh_ndt* h, int* n);
/* debug getter of the list behind [NC]:67 (`correspondences`, ndt_cuda.cu:142-161), offset-major, invalid pairs removed:
 * (source element, target voxel) -- the source element is a point index (P2D) or an index into fvh_ndt_get_voxels(h, 0, ...)
 * (D2D), the target voxel an index into fvh_ndt_get_voxels(h, 1, ...). 2 * fvh_ndt_get_num_correspondences ints. */
int fvh_ndt_get_voxel_correspondences(fvh_ndt* h, int* pairs);
int fvh_ndt_profile_enable(fvh_ndt* h, int on);                                              /* HIP-event timing per kernel class, as fvh_vgicp_profile_* */
int fvh_ndt_profile_reset(fvh_ndt* h);
int fvh_ndt_profile_get(fvh_ndt* h, const char* kernel_class, double* total_ms, int* launches);
int fvh_ndt_synchronize(fvh_ndt* h);
int fvh_ndt_comm_init(fvh_ndt* h, const void* id128, int nranks, int rank);
/* new: multi-GPU NDT by spatial tile. The handle keeps the FULL clouds (target map replicated) and evaluates tile `rank` of `nranks` of the
 * source: P2D -- that chunk of the source points' Morton order (as a sharded VGICP handle); D2D -- that chunk of the source map's voxels
 * ranked by voxel key (a canonical order: the compact list [NCU]:142-161 walks is ordered by atomics and differs between two builds).
 * fvh_ndt_update_correspondences / fvh_ndt_compute_error then return the tile's PARTIAL err / H / b, to be added over the ranks by the
 * caller; with a communicator of the same nranks attached fvh_ndt_align all-reduces them on the device (without one it refuses).
 * nranks = 1 switches the tile off. The correspondence getters and fvh_ndt_align_async are not available on a tiled handle. */
int fvh_ndt_set_source_tile(fvh_ndt* h, int rank, int nranks);
int fvh_ndt_comm_destroy(fvh_ndt* h);

/* ---------------------------------------------------------------------------------------------------
 * Voxel-grid downsampling on device -- the filter every caller of the reference runs on the raw scan
 * right before the registration path: pcl::ApproximateVoxelGrid in src/align.cpp:136-147, src/kitti.cpp:80-82,117-119
 * and pygicp's downsample()/align_points() (src/python/main.cpp:46-62,80-92); pcl::VoxelGrid in
 * src/test/gicp_test.cpp:55-65.  Output points AND their order are bit-identical to those filters on PointXYZ
 * (fp32 sums in input order).  Non-finite coordinates are rejected (FVH_ERR_INVALID_ARGUMENT).
 * The output stays on the device (packed xyz, 3 floats per point) until the next filter call, so it can be handed
 * straight to fvh_*_set_*_cloud_device(ptr, n, 3).
 * --------------------------------------------------------------------------------------------------- */
typedef struct fvh_voxelgrid fvh_voxelgrid;
enum fvh_voxelgrid_method { FVH_VOXELGRID_EXACT = 0 /* pcl::VoxelGrid */, FVH_VOXELGRID_APPROXIMATE = 1 /* pcl::ApproximateVoxelGrid */ };
int fvh_voxelgrid_create(int device, fvh_voxelgrid** out);
int fvh_voxelgrid_get_engine_params(fvh_voxelgrid* h, fvh_engine_params* out);
int fvh_voxelgrid_set_engine_params(fvh_voxelgrid* h, const fvh_engine_params* p);
int fvh_voxelgrid_destroy(fvh_voxelgrid* h);
const char* fvh_voxelgrid_last_error(const fvh_voxelgrid* h);
int fvh_voxelgrid_filter(fvh_voxelgrid* h, int method, const float* xyz, int n, float leaf, int* out_n);                       /* setLeafSize(l,l,l); setInputCloud; filter */
int fvh_voxelgrid_filter_strided(fvh_voxelgrid* h, int method, const float* xyz, int n, int stride_floats /* 3, or 4 for xyzi (KITTI .bin, kitti.cpp:48-60) */, float leaf, int* out_n);
int fvh_voxelgrid_filter_device(fvh_voxelgrid* h, int method, const float* d_xyz, int n, int stride_floats, float leaf, int* out_n);
/* Device-resident pipeline (no PCL counterpart; kitti.cpp:95-128 with every stage on the GPU): run the filter on the registration
 * handle's stream (null: back to its own) -- its output is then ordered before whatever that handle queues next -- and let
 * _async return as soon as the output COUNT is known, while the last kernel of the filter still runs: the caller hands
 * fvh_voxelgrid_device_points() to fvh_*_set_*_cloud_device() of THAT handle. Without a shared stream _async is the synchronous call.
 * The registration handle must outlive the sharing (un-share or destroy the filter first). */
int fvh_voxelgrid_share_stream_with_ndt(fvh_voxelgrid* h, fvh_ndt* registration);
int fvh_voxelgrid_share_stream_with_vgicp(fvh_voxelgrid* h, fvh_vgicp* registration);
/* same, on the registration handle's SECOND stream (the one fvh_ndt_prepare_source_device works on): the filter of the next frame runs
 * beside the LM kernel of the current one, its output is ordered before the preparation that consumes it */
int fvh_voxelgrid_share_prepare_stream_with_ndt(fvh_voxelgrid* h, fvh_ndt* registration);
int fvh_voxelgrid_share_prepare_stream_with_vgicp(fvh_voxelgrid* h, fvh_vgicp* registration); /* ... the one fvh_vgicp_prepare_source_device works on */
int fvh_voxelgrid_filter_device_async(fvh_voxelgrid* h, int method, const float* d_xyz, int n, int stride_floats, float leaf, int* out_n);
int fvh_voxelgrid_get_points(fvh_voxelgrid* h, float* out_xyz /* host or device, 3*out_n floats */);
int fvh_voxelgrid_device_points(fvh_voxelgrid* h, const float** d_xyz, int* n);
int fvh_voxelgrid_profile_enable(fvh_voxelgrid* h, int on);
int fvh_voxelgrid_profile_reset(fvh_voxelgrid* h);
int fvh_voxelgrid_profile_get(fvh_voxelgrid* h, double* total_ms, int* launches);
int fvh_voxelgrid_profile_get_class(fvh_voxelgrid* h, const char* kernel_class, double* total_ms, int* launches); /* any class of the filter's engine: "downsample", "sort", "knn", "outlier_count", "outlier_score", "compact", "deskew", "cluster", "plane" */

/* ---- range crop, statistical and radius outlier removal (no counterpart in the reference's cores: the stages a LiDAR front end runs
 * around the voxel filter -- the origin / range filter of src/align.cpp:127-133, pcl::StatisticalOutlierRemoval,
 * pcl::RadiusOutlierRemoval -- on the filter handle, so a device-resident loop needs no host pass over the scan) ----
 * Forms as for fvh_voxelgrid_filter: host xyz, host rows of stride_floats (3 or 4), device pointer. Output: the kept points IN INPUT
 * ORDER, as bit copies of the input xyz, in the handle's output state -- fvh_voxelgrid_get_points, _device_points and
 * fvh_ndt_{set_source,set_target,prepare_source}_cloud_from_voxelgrid work on it as on a voxel filter's. Side outputs, kept on the device
 * until the next call on the handle: the ascending input indices of the kept points (fvh_voxelgrid_get_kept_indices: out_n ints) and one
 * score per INPUT point with the threshold it was held against (fvh_voxelgrid_get_scores: n floats; either pointer may be NULL). Both
 * getters answer FVH_ERR_BAD_STATE when the last call on the handle was not one of these filters.
 * Chaining: the input may be the handle's own fvh_voxelgrid_device_points() pointer (voxel filter -> outlier removal -> registration
 * on one handle); the input is copied before the output is written. n == 0: out_n = 0, FVH_OK. Argument errors: FVH_ERR_INVALID_ARGUMENT.
 *
 * The definitions below are the contract. They follow PCL's published algorithms; PCL's own boundary behaviour (ties at the radius,
 * its kd-tree's choice among equidistant neighbours, float vs double accumulation) was not available to compare against, and no bit
 * parity with PCL is claimed. d2(i, j) is fp32 (dx*dx + dy*dy) + dz*dz without contraction: what the exact k-NN of this library ranks by.
 *  crop_range   s = (x*x + y*y) + z*z in fp32 without contraction; keep iff x, y, z are finite and min_sq_norm <= (double)s <= max_sq_norm
 *               (max_sq_norm may be +inf). The one stage that DROPS non-finite points silently (pcl::removeNaNFromPointCloud + the
 *               range test): its output is valid input for every other filter. (1e-3, +inf) is the reference's origin filter.
 *               Score: s. Threshold reported: max_sq_norm.
 *  statistical  1 <= mean_k <= 63, n > mean_k, stddev_mul finite. d_i = (float)(sum of (double)sqrtf(d2(i, j)) / mean_k) over the
 *               mean_k + 1 nearest points of the cloud in (d2, index) order -- the nearest is the point itself or a duplicate, at
 *               distance 0 (PCL: search mean_k + 1, skip the first). mu = sum d_i / n, var = max(0, (sum d_i^2 - (sum d_i)^2 / n) / (n - 1)),
 *               t = mu + stddev_mul * sqrt(var) in fp64, summed in a fixed order (two runs give the same bits). Keep iff (double)d_i <= t.
 *               Score: d_i. Threshold: t.
 *  radius       radius finite and > 0, min_neighbors >= 1. r2 = (float)radius * (float)radius, at most 1e37. Keep iff
 *               #{ j != i (by index) : d2(i, j) <= r2 } >= min_neighbors; duplicates of a point count as its neighbours.
 *               Score: min(count, min_neighbors) as a float (the kernel stops counting once the answer is known). Threshold: min_neighbors.
 * The two outlier filters refuse a cloud with a non-finite coordinate as the voxel filters do (out_n = 0, FVH_ERR_INVALID_ARGUMENT). */
int fvh_voxelgrid_crop_range(fvh_voxelgrid* h, const float* xyz, int n, double min_sq_norm, double max_sq_norm, int* out_n);
int fvh_voxelgrid_crop_range_strided(fvh_voxelgrid* h, const float* xyz, int n, int stride_floats, double min_sq_norm, double max_sq_norm, int* out_n);
int fvh_voxelgrid_crop_range_device(fvh_voxelgrid* h, const float* d_xyz, int n, int stride_floats, double min_sq_norm, double max_sq_norm, int* out_n);
int fvh_voxelgrid_remove_statistical_outliers(fvh_voxelgrid* h, const float* xyz, int n, int mean_k, double stddev_mul, int* out_n);
int fvh_voxelgrid_remove_statistical_outliers_strided(fvh_voxelgrid* h, const float* xyz, int n, int stride_floats, int mean_k, double stddev_mul, int* out_n);
int fvh_voxelgrid_remove_statistical_outliers_device(fvh_voxelgrid* h, const float* d_xyz, int n, int stride_floats, int mean_k, double stddev_mul, int* out_n);
int fvh_voxelgrid_remove_radius_outliers(fvh_voxelgrid* h, const float* xyz, int n, double radius, int min_neighbors, int* out_n);
int fvh_voxelgrid_remove_radius_outliers_strided(fvh_voxelgrid* h, const float* xyz, int n, int stride_floats, double radius, int min_neighbors, int* out_n);
int fvh_voxelgrid_remove_radius_outliers_device(fvh_voxelgrid* h, const float* d_xyz, int n, int stride_floats, double radius, int min_neighbors, int* out_n);
int fvh_voxelgrid_get_kept_indices(fvh_voxelgrid* h, int* idx /* out_n ints, host */);
int fvh_voxelgrid_get_scores(fvh_voxelgrid* h, float* scores /* n floats (the INPUT size), host, may be NULL */, double* threshold /* may be NULL */);

/* ---- Euclidean cluster extraction (no counterpart in the reference's cores: pcl::EuclideanClusterExtraction, the stage that groups the
 * points a map does not explain -- fvh_*_score_cloud's "novel" points, or a cropped scan -- into objects, on the filter handle) ----
 * Forms as for the outlier filters: host xyz, host rows of stride_floats (3 or 4), device pointer.
 * Distances and edges. d2(i, j) is the fp32 (dx*dx + dy*dy) + dz*dz without contraction of the radius filter and the k-NN; it is symmetric
 * in i, j to the bit. r2 = (float)tolerance * (float)tolerance, at most 1e37. Edge i ~ j iff i != j (by index) and d2(i, j) <= r2: exact
 * duplicates are connected.
 * Components and size filter. The components are the connected components of that graph. A component of size s is KEPT iff
 * min_cluster_size <= s and (max_cluster_size <= 0 or s <= max_cluster_size).
 * Labels. Kept components are numbered 0 .. num_clusters - 1 in ascending order of their smallest input index; labels[i] is that number,
 * or -1 when i is in no kept component; sizes[c] is the size of cluster c. This DIFFERS from PCL, which sorts its clusters by size at the
 * end and returns index lists; as for the outlier filters, PCL's boundary behaviour (a kd-tree radius search in its own arithmetic) was not
 * available to compare against and no parity with it is claimed beyond the published algorithm. Everything returned is an integer or a
 * bit copy: the result does not depend on the order in which the device visits the edges, and two runs give the same output.
 * Output state. The points of kept components IN INPUT ORDER, as bit copies, in the handle's ordinary output state as after an outlier
 * filter: fvh_voxelgrid_get_points, _device_points and fvh_ndt_{set_source,set_target,prepare_source}_cloud_from_voxelgrid work on it,
 * fvh_voxelgrid_get_kept_indices gives their input indices, fvh_voxelgrid_get_scores gives the (float) size of each INPUT point's component
 * with threshold min_cluster_size. out_n is the kept point count. fvh_voxelgrid_get_cluster_labels copies labels (n ints, INPUT order) and
 * sizes (num_clusters ints) to host or device memory (either may be NULL); it answers FVH_ERR_BAD_STATE when the last call on the handle
 * was not a clustering call. The input may be the handle's own fvh_voxelgrid_device_points() (crop -> cluster chains on one handle): it is
 * copied before the output is written.
 * Refused with FVH_ERR_INVALID_ARGUMENT, out_n = num_clusters = 0, the handle stays usable: tolerance not finite or <= 0;
 * min_cluster_size < 1; 0 < max_cluster_size < min_cluster_size; n < 0, or NULL xyz with n > 0; stride other than 3 or 4; NULL out_n or
 * NULL num_clusters; a non-finite coordinate (detected on the device and reported at the end of the chain, as the outlier filters do:
 * crop_range is the stage that drops such points). n == 0: FVH_OK with zeros.
 * The call runs on the stream the handle currently works on and synchronises it once, with one readback of its control words.
 * Profile classes: "sort", "cluster" (the union-find sweep), "compact" (everything after it). */
int fvh_voxelgrid_cluster_euclidean(fvh_voxelgrid* h, const float* xyz, int n, double tolerance, int min_cluster_size, int max_cluster_size, int* num_clusters, int* out_n);
int fvh_voxelgrid_cluster_euclidean_strided(fvh_voxelgrid* h, const float* xyz, int n, int stride_floats, double tolerance, int min_cluster_size, int max_cluster_size, int* num_clusters, int* out_n);
int fvh_voxelgrid_cluster_euclidean_device(fvh_voxelgrid* h, const float* d_xyz, int n, int stride_floats, double tolerance, int min_cluster_size, int max_cluster_size, int* num_clusters, int* out_n);
int fvh_voxelgrid_get_cluster_labels(fvh_voxelgrid* h, int* labels /* n ints, INPUT order, host or device; may be NULL */, int* sizes /* num_clusters ints; may be NULL */);

/* ---- plane segmentation by RANSAC (no counterpart in the reference's cores: pcl::SACSegmentation with SACMODEL_PLANE /
 * SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC, the ground removal that sits between the filters and the clustering) ----
 * Forms as for the outlier filters: host xyz, host rows of stride_floats (3 or 4), device pointer.
 * Hypotheses. All arithmetic is uint32 with wrap-around. mix32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16.
 * s0 = mix32(lo32(seed) ^ mix32(hi32(seed) ^ 0x9e3779b9)). Hypothesis h (0 <= h < H = max_iterations, 1 <= H <= 16384) samples the INPUT
 * indices i_j = ((uint64)mix32(s0 + 0x9e3779b9 * (3h + j + 1)) * n) >> 32 for j = 0, 1, 2. No resampling and no early exit: the outcome is
 * a function of (cloud, parameters, seed) only. This DIFFERS from PCL, which draws from a stateful generator, redraws degenerate samples
 * and stops adaptively; as for the outlier and cluster calls, no parity with PCL's boundary behaviour is claimed.
 * A hypothesis's plane. Everything in fp64 without contraction, associations as written, coordinates widened to double first:
 * e1 = p[i1] - p[i0], e2 = p[i2] - p[i0], (a, b, c) = e1 x e2 with each component as x*y - z*w, nn = (a*a + b*b) + c*c. The hypothesis is
 * INVALID if two of its indices are equal or nn == 0; with axis non-NULL also unless dot*dot >= (c2*nn)*aa, dot = (a*ax + b*ay) + c*az,
 * aa = (ax*ax + ay*ay) + az*az, c2 = cos(eps_angle)^2 (the host's cos): the normal is within eps_angle of +-axis. No finite float32 input
 * overflows these expressions (the largest intermediate is below 1e235).
 * Score. count_h = #{ i : s_i*s_i <= t2*nn }, u = p[i] - p[i0], s_i = (a*ux + b*uy) + c*uz, t2 = distance_threshold^2: no division and no
 * square root. The winner is the valid hypothesis with the largest count, ties to the smallest h. With no valid hypothesis (n < 3, a
 * collinear or all-duplicate cloud, an axis nothing satisfies) the call returns FVH_OK with num_inliers = 0, coefficients 0, winner -1 and
 * every point an outlier: a streaming loop does not die on one bad frame.
 * Refit (FVH_PLANE_REFINE; skipped when the winner has fewer than 3 inliers). Count, first and second moments of p - q over the winner's
 * inliers, q = p[i0], in fp64 and in a FIXED order (two runs give the same bits); mean mu and covariance C = S2/m - mu mu^T; v = the unit
 * eigenvector of C's smallest eigenvalue (cyclic Jacobi, on the device); the plane is (v, d = -v.(q + mu)). The axis test is not repeated.
 * Returned coefficients (a, b, c, d): unit normal, sign such that d >= 0 (the normal faces the sensor origin; d == 0: the first non-zero
 * component is positive). Without a refit they are the winner's plane normalised on the host (one square root, three divisions,
 * d = -((a*qx + b*qy) + c*qz) on the normalised normal); the labelling IS the winner's count test and num_inliers == count_winner. With a
 * refit the labelling uses the RETURNED doubles: i is an inlier iff s*s <= t2*((a*a + b*b) + c*c), s = ((a*x + b*y) + c*z) + d, and
 * num_inliers counts that labelling.
 * Output state. The kept points are the inliers (FVH_PLANE_KEEP_OUTLIERS: everything else), IN INPUT ORDER, as bit copies, in the handle's
 * ordinary output state as after an outlier filter: fvh_voxelgrid_get_points, _device_points, fvh_ndt_*_from_voxelgrid and
 * fvh_voxelgrid_get_kept_indices work on it; out_n is their count. fvh_voxelgrid_get_scores gives each INPUT point's distance to the
 * WINNER's plane, (float)(|s_i| / sqrt(nn)) (+inf when there is no model), with threshold distance_threshold. The input may be the handle's
 * own fvh_voxelgrid_device_points(): it is copied before the output is written. fvh_voxelgrid_get_cluster_labels answers
 * FVH_ERR_BAD_STATE afterwards. fvh_voxelgrid_get_plane_model returns the coefficients, the winner's three indices, info = {winner,
 * number of valid hypotheses, count_winner, num_inliers} and all H counts (-1 for an invalid hypothesis; host or device memory); each
 * output may be NULL; it answers FVH_ERR_BAD_STATE when the last call on the handle was not a successful plane segmentation.
 * Refused with FVH_ERR_INVALID_ARGUMENT, zero outputs, the handle stays usable: distance_threshold not finite or <= 0; max_iterations
 * outside [1, 16384]; with an axis, eps_angle not in [0, pi/2] or an axis that is not finite or is zero; unknown flag bits; n < 0, or NULL
 * xyz with n > 0; stride other than 3 or 4; NULL coefficients, num_inliers or out_n; a non-finite coordinate (detected on the device and
 * reported at the end of the chain, as the cluster call does). n == 0: FVH_OK with zeros (winner -1, every count -1).
 * The call runs on the stream the handle currently works on and synchronises it once, with one readback of its control words.
 * Profile classes: "plane" (hypotheses, sweep, winner, refit), "compact" (everything after it). */
enum fvh_plane_flags { FVH_PLANE_KEEP_OUTLIERS = 1, FVH_PLANE_REFINE = 2 };
int fvh_voxelgrid_segment_plane(fvh_voxelgrid* h, const float* xyz, int n, double distance_threshold, int max_iterations, unsigned long long seed, const double* axis /* 3 doubles, host; NULL: no constraint */, double eps_angle, int flags, double* coefficients /* 4 */, int* num_inliers, int* out_n);
int fvh_voxelgrid_segment_plane_strided(fvh_voxelgrid* h, const float* xyz, int n, int stride_floats, double distance_threshold, int max_iterations, unsigned long long seed, const double* axis, double eps_angle, int flags, double* coefficients, int* num_inliers, int* out_n);
int fvh_voxelgrid_segment_plane_device(fvh_voxelgrid* h, const float* d_xyz, int n, int stride_floats, double distance_threshold, int max_iterations, unsigned long long seed, const double* axis, double eps_angle, int flags, double* coefficients, int* num_inliers, int* out_n);
int fvh_voxelgrid_get_plane_model(fvh_voxelgrid* h, double* coefficients /* 4 */, int* sample /* 3 */, int* info /* 4 */, int* counts /* max_iterations ints, host or device */);

/* ---- motion compensation ("deskew") of one sweep (no counterpart in the reference: the KITTI odometry scans it runs on are untwisted by
 * the dataset; a live driver delivers points taken over ~0.1 s of vehicle motion) ----
 * Input: n points (float32 xyz), one float32 time per point t_i = times[i * time_stride] (a separate array: time_stride 1; xyzt rows:
 * times = xyz + 3, time_stride 4), K knots (2 <= K <= 64) with times tau[0] < ... < tau[K-1] (fp64, finite) and poses T[0..K-1]
 * (knot_poses: K consecutive 4x4 double COLUMN-MAJOR matrices, sensor-at-that-instant -> one fixed frame), and a reference time t_ref
 * (finite fp64). A knot pose must be finite, as fvh_*_map_insert_source asks of its pose, and -- a logarithm is taken of it -- a rigid
 * motion: last row (0, 0, 0, 1) to 1e-9, |R^T R - I| <= 1e-6 entrywise, det R > 0.
 * Trajectory: xi_j = log(T[j]^-1 * T[j+1]) (SE(3) logarithm, rotation part omega_j, translation part v_j; rotation-first exponential
 * exp(omega, v) = {exp(omega), V(omega) v}), computed once on the host in fp64. For a time x: j(x) = the largest j with tau[j] <= x,
 * clamped to [0, K-2]; s = (x - tau[j]) / (tau[j+1] - tau[j]); T(x) = T[j] * exp(s * xi_j). s outside [0, 1] on the end segments
 * EXTRAPOLATES at that segment's constant twist (drivers overshoot the sweep by a few points).
 * Output: p'_i = float32( T(t_ref)^-1 * T((double)t_i) * (double)p_i ), everything before the final cast in fp64; out_n = n, input order.
 * The output is the handle's output state exactly as after a crop (packed xyz and {x, y, z, 0}): fvh_voxelgrid_get_points,
 * _device_points, fvh_ndt_{set_source,set_target,prepare_source}_cloud_from_voxelgrid and a following crop_range_device / filter_device on
 * the handle's own output pointer work on it unchanged. fvh_voxelgrid_get_kept_indices / _get_scores answer FVH_ERR_BAD_STATE after it.
 * The input xyz may be the handle's own fvh_voxelgrid_device_points() (it is copied before the output is written).
 * A point whose time or any coordinate is not finite comes out as three NaNs; it is not refused: crop_range is the stage that drops
 * non-finite points, and deskew -> crop_range is the intended chain (deskew FIRST: crop and voxel filter change the indexing of the times).
 * Refused with FVH_ERR_INVALID_ARGUMENT and out_n = 0: K outside [2, 64]; knot times not finite or not strictly increasing; a non-rigid
 * knot pose; a segment whose relative rotation angle exceeds pi - 1e-6 (the logarithm is not unique there); non-finite t_ref; null
 * pointers with n > 0 (null knot arrays at any n); stride not 3 or 4; time_stride < 1. n == 0: out_n = 0, FVH_OK.
 * _device: d_xyz and d_times are device memory; the knot arrays are always host memory. All three forms run on the stream the handle
 * currently works on (sharing as for the other filters) and synchronise it before returning. Profile class: "deskew". */
int fvh_voxelgrid_deskew(fvh_voxelgrid* h, const float* xyz, int n, const float* times, int time_stride, const double* knot_times, const double* knot_poses, int K, double t_ref, int* out_n);
int fvh_voxelgrid_deskew_strided(fvh_voxelgrid* h, const float* xyz, int n, int stride_floats, const float* times, int time_stride, const double* knot_times, const double* knot_poses, int K, double t_ref, int* out_n);
int fvh_voxelgrid_deskew_device(fvh_voxelgrid* h, const float* d_xyz, int n, int stride_floats, const float* d_times, int time_stride, const double* knot_times, const double* knot_poses, int K, double t_ref, int* out_n);

#ifdef __cplusplus
}
#endif
#endif /* FAST_VGICP_HIP_H */
