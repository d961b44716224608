// Call trace of the host C++ classes (include/fast_gicp_amd/registration.hpp) without a GPU: every fvh_* function the header uses is a
// fake that prints its name and arguments and returns canned results, and main() drives FastVGICPCuda, FastGICP, FastVGICP and NDTCuda
// through their public methods. The output -- which C calls are made, in which order, with which arguments and labels, and what the
// getters hold afterwards -- is compared byte for byte with tests/golden/registration_trace.txt (tests/test_registration_trace_cpu.py).
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <type_traits>
#include <vector>

#include "fast_gicp_amd/registration.hpp"

struct fvh_vgicp { int n_source = 0, n_target = 0; };
struct fvh_ndt { int unused = 0; };
struct fvh_voxelgrid { int unused = 0; };

namespace {
const char* g_fail = nullptr;  // the fake of this name returns 3 once ...
int g_fail_skip = 0;           // ... after this many calls of it that succeed
int g_trace_rows = 2;          // what get_lm_trace reports

void vec(const char* label, const double* v, int n) {
  std::printf(" %s=", label);
  if (!v) { std::printf("null"); return; }
  for (int i = 0; i < n; i++) std::printf(i ? " %.9g" : "[%.9g", v[i]);
  std::printf("]");
}
void params(const fvh_lm_params* p) {
  if (!p) { std::printf(" params=null"); return; }
  std::printf(" params={%d %.9g %.9g %d %.9g %d}", p->max_iterations, p->rotation_epsilon, p->transformation_epsilon, p->lm_max_iterations, p->lm_init_lambda_factor, p->optimizer);
}
int end(const char* fn) {
  std::printf("\n");
  if (g_fail && !std::strcmp(g_fail, fn) && g_fail_skip-- == 0) {
    g_fail = nullptr;
    std::printf("  (%s returns 3)\n", fn);
    return 3;
  }
  return 0;
}
#define BEGIN std::printf("%s", __func__)
#define END return end(__func__)

void cloud(const float* xyz, int n, int stride) {
  std::printf(" n=%d stride=%d", n, stride);
  if (!xyz) std::printf(" xyz=null");
  else for (int i = 0; i < n; i++) std::printf(" (%.9g %.9g %.9g)", xyz[i * stride], xyz[i * stride + 1], xyz[i * stride + 2]);
}
int fake_cloud(const char* fn, const float* xyz, int n, int stride) {
  std::printf("%s", fn);
  cloud(xyz, n, stride);
  return end(fn);
}
int fake_neighbors(const char* fn, int n, int k, const int* nb) {
  std::printf("%s k=%d", fn, k);
  if (!nb) std::printf(" neighbors=null");
  else for (int i = 0; i < n * k; i++) std::printf(i % k ? " %d" : " | %d", nb[i]);
  return end(fn);
}
int fake_pose(const char* fn, const double* T16) {
  std::printf("%s", fn);
  vec("T", T16, 16);
  return end(fn);
}
// err = 1 + |t - (0.5, 0, 0)|^2 with its gradient in b and a non-symmetric H: the host LM loop has something to walk on
int fake_compute_error(const char* fn, const double* T, double* H, double* b, double* err) {
  std::printf("%s", fn);
  vec("T", T, 16);
  std::printf(" H=%s b=%s error=%s", H ? "set" : "null", b ? "set" : "null", err ? "set" : "null");
  const double d[3] = {T[12] - 0.5, T[13], T[14]};
  if (err) *err = 1.0 + d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  if (H) for (int c = 0; c < 6; c++) for (int r = 0; r < 6; r++) H[c * 6 + r] = r == c ? 2.0 + 0.125 * r : 0.001 * (c * 6 + r);
  if (b) for (int i = 0; i < 6; i++) b[i] = i < 3 ? 0.01 * (i + 1) : 2.0 * d[i - 3];
  return end(fn);
}
void canned_result(fvh_lm_result* r, int i) {
  std::memset(r, 0, sizeof(*r));
  const double c = 0.9800665778412416, s = 0.19866933079506122;  // a rotation of 0.2 rad about z, column-major
  const double T[16] = {c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, 1.0 + i, 2.0, 3.0, 1};
  std::memcpy(r->T, T, sizeof(T));
  for (int j = 0; j < 36; j++) r->H[j] = j + 0.5 + 100.0 * i;
  r->final_error = 0.125 + i;
  r->converged = i % 2 == 0;
  r->nr_iterations = 7 + i;
  r->num_linearize = 8;
  r->num_error_evals = 9;
  r->lm_failed = 1;
  r->num_launches = 1;
}
int fake_align(const char* fn, const double* g, const fvh_lm_params* p, fvh_lm_result* r) {
  std::printf("%s", fn);
  vec("guess", g, 16);
  params(p);
  std::printf(" result=%s", r ? "set" : "null");
  if (r) canned_result(r, 0);
  return end(fn);
}
int fake_align_multi(const char* fn, int k, const double* g, const fvh_lm_params* p, fvh_lm_result* r, int* grid) {
  std::printf("%s k=%d", fn, k);
  vec("guesses", g, 16 * k);
  params(p);
  std::printf(" results=%s grid_blocks=%s", r ? "set" : "null", grid ? "set" : "null");
  for (int i = 0; r && i < k; i++) canned_result(r + i, i);
  if (grid) *grid = 24;
  return end(fn);
}
int fake_align_async(const char* fn, const double* g, const fvh_lm_params* p) {
  std::printf("%s", fn);
  vec("guess", g, 16);
  params(p);
  return end(fn);
}
int fake_align_wait(const char* fn, fvh_lm_result* r) {
  std::printf("%s result=%s", fn, r ? "set" : "null");
  if (r) { canned_result(r, 1); r->lm_failed = 0; }
  return end(fn);
}
int fake_fitness(const char* fn, const double* T, double max_range, double* score) {
  std::printf("%s", fn);
  vec("T", T, 16);
  std::printf(" max_range=%.9g score=%s", max_range, score ? "set" : "null");
  if (score) *score = 10.0 - T[12];
  return end(fn);
}
int fake_get_trace(const char* fn, int* n, double* rows) {
  std::printf("%s num_rows=%s rows=%s", fn, n ? "set" : "null", rows ? "set" : "null");
  if (n) *n = g_trace_rows;
  for (int i = 0; rows && i < 6 * g_trace_rows; i++) rows[i] = i % 6 == 0 ? i / 6 : (i % 6 == 3 ? (i < 6 ? 0.5 : -0.25) : 0.1 * i);
  return end(fn);
}
int fake_int(const char* fn, int a) { std::printf("%s %d", fn, a); return end(fn); }
int fake_void(const char* fn) { std::printf("%s", fn); return end(fn); }
}  // namespace

extern "C" {
int fvh_vgicp_create(int device, fvh_vgicp** out) { BEGIN; std::printf(" device=%d", device); *out = new fvh_vgicp; END; }
int fvh_vgicp_destroy(fvh_vgicp* h) { delete h; return fake_void(__func__); }
const char* fvh_vgicp_last_error(const fvh_vgicp*) { return "the vgicp handle's text"; }
int fvh_vgicp_set_resolution(fvh_vgicp*, double r) { BEGIN; std::printf(" %.9g", r); END; }
int fvh_vgicp_set_kernel_params(fvh_vgicp*, double w, double d) { BEGIN; std::printf(" %.9g %.9g", w, d); END; }
int fvh_vgicp_set_neighbor_search_method(fvh_vgicp*, int m, double r) { BEGIN; std::printf(" %d %.9g", m, r); END; }
int fvh_vgicp_set_precision(fvh_vgicp*, int p) { return fake_int(__func__, p); }
int fvh_vgicp_set_voxel_accumulation_mode(fvh_vgicp*, int m) { return fake_int(__func__, m); }
int fvh_vgicp_swap_source_and_target(fvh_vgicp* h) { std::swap(h->n_source, h->n_target); return fake_void(__func__); }
int fvh_vgicp_set_source_cloud_strided(fvh_vgicp* h, const float* xyz, int n, int stride) { h->n_source = n; return fake_cloud(__func__, xyz, n, stride); }
int fvh_vgicp_set_target_cloud_strided(fvh_vgicp* h, const float* xyz, int n, int stride) { h->n_target = n; return fake_cloud(__func__, xyz, n, stride); }
int fvh_vgicp_set_source_neighbors(fvh_vgicp* h, int k, const int* nb) { return fake_neighbors(__func__, h->n_source, k, nb); }
int fvh_vgicp_set_target_neighbors(fvh_vgicp* h, int k, const int* nb) { return fake_neighbors(__func__, h->n_target, k, nb); }
int fvh_vgicp_find_source_neighbors(fvh_vgicp*, int k) { return fake_int(__func__, k); }
int fvh_vgicp_find_target_neighbors(fvh_vgicp*, int k) { return fake_int(__func__, k); }
int fvh_vgicp_calculate_source_covariances(fvh_vgicp*, int reg) { return fake_int(__func__, reg); }
int fvh_vgicp_calculate_target_covariances(fvh_vgicp*, int reg) { return fake_int(__func__, reg); }
int fvh_vgicp_calculate_source_covariances_rbf(fvh_vgicp*, int reg) { return fake_int(__func__, reg); }
int fvh_vgicp_calculate_target_covariances_rbf(fvh_vgicp*, int reg) { return fake_int(__func__, reg); }
int fvh_vgicp_set_source_covariances(fvh_vgicp* h, const double* c) { BEGIN; vec("covs9", c, c ? 9 * h->n_source : 0); END; }
int fvh_vgicp_set_target_covariances(fvh_vgicp* h, const double* c) { BEGIN; vec("covs9", c, c ? 9 * h->n_target : 0); END; }
int fvh_vgicp_get_source_covariances(fvh_vgicp* h, float* c) { BEGIN; for (int i = 0; i < 9 * h->n_source; i++) c[i] = 0.5f * i; END; }
int fvh_vgicp_get_target_covariances(fvh_vgicp* h, float* c) { BEGIN; for (int i = 0; i < 9 * h->n_target; i++) c[i] = 0.25f * i; END; }
int fvh_vgicp_create_target_voxelmap(fvh_vgicp*) { return fake_void(__func__); }
int fvh_vgicp_update_correspondences(fvh_vgicp*, const double* T) { return fake_pose(__func__, T); }
int fvh_vgicp_compute_error(fvh_vgicp*, const double* T, double* H, double* b, double* e) { return fake_compute_error(__func__, T, H, b, e); }
int fvh_vgicp_align(fvh_vgicp*, const double* g, const fvh_lm_params* p, fvh_lm_result* r) { return fake_align(__func__, g, p, r); }
int fvh_vgicp_align_multi(fvh_vgicp*, int k, const double* g, const fvh_lm_params* p, fvh_lm_result* r, int* grid) { return fake_align_multi(__func__, k, g, p, r, grid); }
int fvh_vgicp_align_async(fvh_vgicp*, const double* g, const fvh_lm_params* p) { return fake_align_async(__func__, g, p); }
int fvh_vgicp_align_wait(fvh_vgicp*, fvh_lm_result* r) { return fake_align_wait(__func__, r); }
int fvh_vgicp_prepare_source_device(fvh_vgicp*, const float* d, int n, int stride, int k, int reg, int rbf, int stages) {
  BEGIN; std::printf(" d_xyz=%s n=%d stride=%d k=%d reg=%d rbf=%d stages=%d", d ? "set" : "null", n, stride, k, reg, rbf, stages); END;
}
int fvh_vgicp_prepare_source(fvh_vgicp*, const float* xyz, int n, int stride, int k, int reg, int rbf, int stages) {
  BEGIN; std::printf(" k=%d reg=%d rbf=%d stages=%d", k, reg, rbf, stages); cloud(xyz, n, stride); END;
}
int fvh_vgicp_adopt_prepared_source(fvh_vgicp*) { return fake_void(__func__); }
int fvh_vgicp_map_begin(fvh_vgicp*, int expected) { return fake_int(__func__, expected); }
int fvh_vgicp_map_insert_source(fvh_vgicp*, const double* T) { return fake_pose(__func__, T); }
int fvh_vgicp_map_prune(fvh_vgicp*, const double* c, double radius, int max_age, int* removed) {
  BEGIN; vec("center", c, 3); std::printf(" radius=%.9g max_age=%d removed=%s", radius, max_age, removed ? "set" : "null"); if (removed) *removed = 4; END;
}
int fvh_vgicp_voxelmap_export(fvh_vgicp*, int* n, double* res, int* mode, int* inserts, long long* points, int* coords, double* sums, unsigned* ages) {
  BEGIN; std::printf(" coords=%s sums=%s ages=%s", coords ? "set" : "null", sums ? "set" : "null", ages ? "set" : "null");
  *n = 2; *res = 0.5; *mode = 2; *inserts = 3; *points = 11;
  for (int i = 0; coords && i < 6; i++) coords[i] = i - 2;
  for (int i = 0; sums && i < 20; i++) sums[i] = 0.5 * i;
  for (int i = 0; ages && i < 2; i++) ages[i] = 1u + i;
  END;
}
int fvh_vgicp_voxelmap_import(fvh_vgicp*, int n, const int* coords, const double* sums, const unsigned* ages, double res, int mode, int inserts, long long points) {
  BEGIN; std::printf(" n=%d resolution=%.9g mode=%d num_inserts=%d num_points=%lld coords=", n, res, mode, inserts, points);
  for (int i = 0; coords && i < 3 * n; i++) std::printf("%d,", coords[i]);
  vec("sums", sums, sums ? 10 * n : 0);
  std::printf(" ages=");
  for (int i = 0; ages && i < n; i++) std::printf("%u,", ages[i]);
  END;
}
int fvh_vgicp_voxelmap_merge_from(fvh_vgicp*, fvh_vgicp* other) { BEGIN; std::printf(" other=%s", other ? "set" : "null"); END; }
int fvh_vgicp_set_lm_trace(fvh_vgicp*, int on) { return fake_int(__func__, on); }
int fvh_vgicp_get_lm_trace(fvh_vgicp*, int* n, double* rows) { return fake_get_trace(__func__, n, rows); }
int fvh_vgicp_fitness_score(fvh_vgicp*, const double* T, double r, double* s) { return fake_fitness(__func__, T, r, s); }
int fvh_vgicp_gicp_set_max_correspondence_distance(fvh_vgicp*, double d) { BEGIN; std::printf(" %.9g", d); END; }
int fvh_vgicp_gicp_swap_source_and_target(fvh_vgicp* h) { std::swap(h->n_source, h->n_target); return fake_void(__func__); }
int fvh_vgicp_gicp_update_correspondences(fvh_vgicp*, const double* T) { return fake_pose(__func__, T); }
int fvh_vgicp_gicp_compute_error(fvh_vgicp*, const double* T, double* H, double* b, double* e) { return fake_compute_error(__func__, T, H, b, e); }
int fvh_vgicp_gicp_align(fvh_vgicp*, const double* g, const fvh_lm_params* p, fvh_lm_result* r) { return fake_align(__func__, g, p, r); }

int fvh_ndt_create(int device, fvh_ndt** out) { BEGIN; std::printf(" device=%d", device); *out = new fvh_ndt; END; }
int fvh_ndt_destroy(fvh_ndt* h) { delete h; return fake_void(__func__); }
const char* fvh_ndt_last_error(const fvh_ndt*) { return "the ndt handle's text"; }
int fvh_ndt_set_distance_mode(fvh_ndt*, int m) { return fake_int(__func__, m); }
int fvh_ndt_set_resolution(fvh_ndt*, double r) { BEGIN; std::printf(" %.9g", r); END; }
int fvh_ndt_set_neighbor_search_method(fvh_ndt*, int m, double r) { BEGIN; std::printf(" %d %.9g", m, r); END; }
int fvh_ndt_swap_source_and_target(fvh_ndt*) { return fake_void(__func__); }
int fvh_ndt_set_source_cloud_strided(fvh_ndt*, const float* xyz, int n, int stride) { return fake_cloud(__func__, xyz, n, stride); }
int fvh_ndt_set_target_cloud_strided(fvh_ndt*, const float* xyz, int n, int stride) { return fake_cloud(__func__, xyz, n, stride); }
int fvh_ndt_create_voxelmaps(fvh_ndt*) { return fake_void(__func__); }
int fvh_ndt_update_correspondences(fvh_ndt*, const double* T) { return fake_pose(__func__, T); }
int fvh_ndt_compute_error(fvh_ndt*, const double* T, double* H, double* b, double* e) { return fake_compute_error(__func__, T, H, b, e); }
int fvh_ndt_align(fvh_ndt*, const double* g, const fvh_lm_params* p, fvh_lm_result* r) { return fake_align(__func__, g, p, r); }
int fvh_ndt_align_multi(fvh_ndt*, int k, const double* g, const fvh_lm_params* p, fvh_lm_result* r, int* grid) { return fake_align_multi(__func__, k, g, p, r, grid); }
int fvh_ndt_align_async(fvh_ndt*, const double* g, const fvh_lm_params* p) { return fake_align_async(__func__, g, p); }
int fvh_ndt_align_wait(fvh_ndt*, fvh_lm_result* r) { return fake_align_wait(__func__, r); }
int fvh_ndt_prepare_source_device(fvh_ndt*, const float* d, int n, int stride) { BEGIN; std::printf(" d_xyz=%s n=%d stride=%d", d ? "set" : "null", n, stride); END; }
int fvh_ndt_prepare_source(fvh_ndt*, const float* xyz, int n, int stride) { return fake_cloud(__func__, xyz, n, stride); }
int fvh_ndt_adopt_prepared_source(fvh_ndt*) { return fake_void(__func__); }
int fvh_ndt_prepare_source_from_voxelgrid(fvh_ndt*, fvh_voxelgrid* f) { BEGIN; std::printf(" filter=%s", f ? "set" : "null"); END; }
int fvh_ndt_fitness_score(fvh_ndt*, const double* T, double r, double* s) { return fake_fitness(__func__, T, r, s); }
int fvh_ndt_set_lm_trace(fvh_ndt*, int on) { return fake_int(__func__, on); }
int fvh_ndt_get_lm_trace(fvh_ndt*, int* n, double* rows) { return fake_get_trace(__func__, n, rows); }
}

using namespace fast_gicp;
using P = PointXYZ;
using Cloud = PointCloud<P>;
using VGICPCuda = FastVGICPCuda<P, P>;
using GICP = FastGICP<P, P>;
using VGICP = FastVGICP<P, P>;
using NDT = NDTCuda<P, P>;
struct PointXYZIR { float x, y, z, intensity, ring; };  // 20 bytes: goes through the repack of detail::XyzView

namespace {
template <typename PointT = P>
std::shared_ptr<PointCloud<PointT>> make_cloud(int n, float offset) {
  auto c = std::make_shared<PointCloud<PointT>>();
  c->resize((size_t)n);
  for (int i = 0; i < n; i++) {
    auto& p = c->points[(size_t)i];
    p.x = offset + 0.5f * (float)i; p.y = 0.25f * (float)((i * 3) % 5); p.z = (float)(i % 2) - 0.125f * (float)i;
  }
  return c;
}
Matrix4f guess(float tx) {  // a rotation of 0.1 rad about x and a translation
  Matrix4f G = Matrix4f::Identity();
  G(1, 1) = 0.99500417f; G(1, 2) = -0.09983342f; G(2, 1) = 0.09983342f; G(2, 2) = 0.99500417f;
  G(0, 3) = tx; G(1, 3) = -0.25f; G(2, 3) = 0.125f;
  return G;
}
void step(const char* what) { std::printf("== %s\n", what); }
/// runs f; an exception becomes a line of the trace
void attempt(const std::function<void()>& f) {
  try { f(); } catch (const std::exception& e) { std::printf("  exception: %s\n", e.what()); }
}
template <typename R>
void getters(R& reg, const Cloud& out) {
  std::printf("  hasConverged=%d getNumIterations=%d\n  H=", (int)reg.hasConverged(), reg.getNumIterations());
  for (double v : reg.getFinalHessian()) std::printf(" %.9g", v);
  std::printf("\n  T=");
  for (float v : reg.getFinalTransformation().m) std::printf(" %.9g", v);
  if (out.empty()) std::printf("\n  out: empty\n");
  else std::printf("\n  out: %zu points, first (%.9g %.9g %.9g)\n", out.size(), out.points[0].x, out.points[0].y, out.points[0].z);
}
template <typename R>
void inputs(R& reg, const Cloud::ConstPtr& source, const Cloud::ConstPtr& target) {
  std::printf("  input is %s, target is %s\n", reg.getInputSource() == source ? "source" : reg.getInputSource() == target ? "target" : reg.getInputSource() ? "other" : "null",
              reg.getInputTarget() == target ? "target" : reg.getInputTarget() == source ? "source" : reg.getInputTarget() ? "other" : "null");
}

template <typename R>
constexpr bool kHasAsync = std::is_same<R, VGICPCuda>::value || std::is_same<R, NDT>::value;

/// steps 2-7, 9 and 10 of the test plan on a registration object with both clouds set
template <typename R>
void drive(R& reg, const Cloud::ConstPtr& source, const Cloud::ConstPtr& target) {
  Cloud out;
  step("the same pointers again");
  reg.setInputTarget(target);
  reg.setInputSource(source);
  inputs(reg, source, target);

  step("align, debug print off");
  attempt([&] { reg.align(out, guess(0.5f)); });
  getters(reg, out);
  step("align, debug print on");
  reg.setDebugPrint(true);
  attempt([&] { reg.align(out, guess(0.75f)); });
  getters(reg, out);
  step("align, debug print on, an empty trace");
  g_trace_rows = 0;
  attempt([&] { reg.align(out, guess(0.75f)); });
  g_trace_rows = 2;
  reg.setDebugPrint(false);
  step("align, default guess, GaussNewton");
  reg.setLSQType(LSQ_OPTIMIZER_TYPE::GaussNewton);
  attempt([&] { reg.align(out); });
  getters(reg, out);
  step("align on the host loop, two iterations, GaussNewton");
  reg.setUseDeviceLM(false);
  reg.setMaximumIterations(2);
  attempt([&] { reg.align(out, guess(0.5f)); });
  getters(reg, out);
  step("align on the host loop, two iterations, LevenbergMarquardt, debug print on");
  reg.setLSQType(LSQ_OPTIMIZER_TYPE::LevenbergMarquardt);
  reg.setDebugPrint(true);
  attempt([&] { reg.align(out, guess(0.5f)); });
  getters(reg, out);
  reg.setDebugPrint(false);
  reg.setUseDeviceLM(true);
  reg.setMaximumIterations(64);
  step("align with other parameters");
  reg.setRotationEpsilon(1e-3); reg.setTransformationEpsilon(2e-4); reg.setMaximumIterations(33); reg.setInitialLambdaFactor(1e-6);
  attempt([&] { reg.align(out, guess(0.5f)); });

  step("evaluateCost");
  Matrix6d H;
  Vector6d b;
  H.fill(-1.0); b.fill(-1.0);
  attempt([&] { std::printf("  cost=%.9g\n", reg.evaluateCost(guess(0.25f), &H, &b)); });
  std::printf("  H=");
  for (double v : H) std::printf(" %.9g", v);
  std::printf("\n  b=");
  for (double v : b) std::printf(" %.9g", v);
  std::printf("\n");
  attempt([&] { std::printf("  cost=%.9g\n", reg.evaluateCost(guess(0.25f))); });
  attempt([&] { std::printf("  cost=%.9g\n", reg.evaluateCost(guess(0.25f), &H)); });

  step("getFitnessScore");
  attempt([&] { std::printf("  score=%.9g\n", reg.getFitnessScore(2.0)); });
  attempt([&] { std::printf("  score=%.9g\n", reg.getFitnessScore()); });

  step("alignMulti");
  const std::vector<Matrix4f> guesses{guess(0.5f), guess(-1.5f)};
  attempt([&] {
    const std::vector<MultiAlignResult> rs = reg.alignMulti(guesses);
    for (const MultiAlignResult& r : rs) {
      std::printf("  final_error=%.9g converged=%d nr_iterations=%d\n  T=", r.final_error, (int)r.converged, r.nr_iterations);
      for (double v : r.T.m) std::printf(" %.9g", v);
      std::printf("\n  H=");
      for (double v : r.H) std::printf(" %.9g", v);
      std::printf("\n");
    }
  });
  std::printf("  getMultiGridBlocks=%d\n", reg.getMultiGridBlocks());
  getters(reg, out);
  step("alignBest");
  attempt([&] { std::printf("  best=%d\n", reg.alignBest(guesses, 3.0, out)); });
  getters(reg, out);
  attempt([&] { reg.alignBest({}, 3.0, out); });

  step("swapSourceAndTarget");
  attempt([&] { reg.swapSourceAndTarget(); });
  inputs(reg, source, target);
  attempt([&] { reg.swapSourceAndTarget(); });
  inputs(reg, source, target);

  if constexpr (kHasAsync<R>) {
    step("alignAsync / alignWait");
    attempt([&] { reg.alignAsync(guess(0.5f)); });
    attempt([&] {
      const Matrix4f& T = reg.alignWait();
      std::printf("  alignWait returns getFinalTransformation(): %d\n", (int)(&T == &reg.getFinalTransformation()));
    });
    getters(reg, out);
    reg.setLSQType(LSQ_OPTIMIZER_TYPE::GaussNewton);
    attempt([&] { reg.alignAsync(); });
    reg.setLSQType(LSQ_OPTIMIZER_TYPE::LevenbergMarquardt);
    step("prepareNextSource / adoptPreparedSource");
    const Cloud::ConstPtr next = make_cloud(3, 7.f);
    attempt([&] { reg.prepareNextSource(next); });
    inputs(reg, source, target);
    attempt([&] { reg.adoptPreparedSource(); });
    std::printf("  input is the prepared cloud: %d\n", (int)(reg.getInputSource() == next));
    const float device_points[3] = {0, 0, 0};
    attempt([&] { reg.prepareNextSourceDevice(device_points, 1, 3); });
    attempt([&] { reg.adoptPreparedSource(); });
    std::printf("  input is null: %d\n", (int)(reg.getInputSource() == nullptr));
    attempt([&] { reg.setInputSource(source); });
  }

  step("one failing call per C function");
  struct Failure { const char* fn; int skip; std::function<void()> run; };
  std::vector<Failure> failures;
  const bool ndt = std::is_same<R, NDT>::value, gicp = std::is_same<R, GICP>::value;
  const char* compute_error = ndt ? "fvh_ndt_compute_error" : gicp ? "fvh_vgicp_gicp_compute_error" : "fvh_vgicp_compute_error";
  const Cloud::ConstPtr other_source = make_cloud(2, 3.f), other_target = make_cloud(2, 4.f);
  failures.push_back({ndt ? "fvh_ndt_set_source_cloud_strided" : "fvh_vgicp_set_source_cloud_strided", 0, [&] { reg.setInputSource(other_source); }});
  failures.push_back({ndt ? "fvh_ndt_set_target_cloud_strided" : "fvh_vgicp_set_target_cloud_strided", 0, [&] { reg.setInputTarget(other_target); }});
  failures.push_back({ndt ? "fvh_ndt_update_correspondences" : gicp ? "fvh_vgicp_gicp_update_correspondences" : "fvh_vgicp_update_correspondences", 0, [&] { reg.evaluateCost(guess(0.f)); }});
  failures.push_back({compute_error, 0, [&] { reg.evaluateCost(guess(0.f)); }});
  failures.push_back({compute_error, 1, [&] { reg.setUseDeviceLM(false); reg.align(out, guess(0.f)); }});  // the trial step's compute_error()
  failures.push_back({ndt ? "fvh_ndt_align" : gicp ? "fvh_vgicp_gicp_align" : "fvh_vgicp_align", 0, [&] { reg.align(out, guess(0.f)); }});
  failures.push_back({ndt ? "fvh_ndt_align_multi" : "fvh_vgicp_align_multi", 0, [&] { reg.alignMulti(guesses); }});
  failures.push_back({ndt ? "fvh_ndt_fitness_score" : "fvh_vgicp_fitness_score", 0, [&] { reg.getFitnessScore(2.0); }});
  failures.push_back({ndt ? "fvh_ndt_fitness_score" : "fvh_vgicp_fitness_score", 1, [&] { reg.alignBest(guesses, 2.0, out); }});
  failures.push_back({ndt ? "fvh_ndt_set_lm_trace" : "fvh_vgicp_set_lm_trace", 0, [&] { reg.align(out, guess(0.f)); }});
  failures.push_back({ndt ? "fvh_ndt_get_lm_trace" : "fvh_vgicp_get_lm_trace", 0, [&] { reg.setDebugPrint(true); reg.align(out, guess(0.f)); }});
  failures.push_back({ndt ? "fvh_ndt_get_lm_trace" : "fvh_vgicp_get_lm_trace", 1, [&] { reg.setDebugPrint(true); reg.align(out, guess(0.f)); }});
  if constexpr (kHasAsync<R>) {
    failures.push_back({ndt ? "fvh_ndt_align_async" : "fvh_vgicp_align_async", 0, [&] { reg.alignAsync(guess(0.f)); }});
    failures.push_back({ndt ? "fvh_ndt_align_wait" : "fvh_vgicp_align_wait", 0, [&] { reg.alignWait(); }});
  }
  if (ndt) failures.push_back({"fvh_ndt_create_voxelmaps", 0, [&] { reg.align(out, guess(0.f)); }});
  if (ndt) failures.push_back({"fvh_ndt_create_voxelmaps", 0, [&] { reg.alignMulti(guesses); }});
  for (Failure& f : failures) {
    std::printf("-- %s, call %d\n", f.fn, f.skip + 1);
    g_fail = f.fn;
    g_fail_skip = f.skip;
    attempt(f.run);
    g_fail = nullptr;
    reg.setDebugPrint(false);
    reg.setUseDeviceLM(true);
    inputs(reg, source, target);
    getters(reg, out);
    attempt([&] { reg.setInputSource(source); reg.setInputTarget(target); });
  }

  step("clearSource / clearTarget");
  reg.clearTarget();
  attempt([&] { reg.align(out); });
  attempt([&] { reg.alignMulti(guesses); });
  reg.clearSource();
  inputs(reg, source, target);
  attempt([&] { reg.align(out); });
}
}  // namespace

int main() {
  std::setvbuf(stdout, nullptr, _IONBF, 0);
  dup2(1, 2);  // "lm not converged!!" goes to stderr: into the same stream, in order
  const Cloud::ConstPtr source = make_cloud(5, 0.f), target = make_cloud(5, 1.f);

  std::printf("#### FastVGICPCuda\n");
  for (NearestNeighborMethod method : {NearestNeighborMethod::CPU_PARALLEL_KDTREE, NearestNeighborMethod::GPU_BRUTEFORCE, NearestNeighborMethod::GPU_RBF_KERNEL})
    for (bool host_tree : {false, true}) {
      std::printf("== setInputTarget / setInputSource, nearest neighbour method %d, host kd-tree %d\n", (int)method, (int)host_tree);
      VGICPCuda reg;
      reg.setNearestNeighborSearchMethod(method);
      reg.setHostKdTree(host_tree);
      std::printf("  getHostKdTree=%d\n", (int)reg.getHostKdTree());
      reg.setInputTarget(target); reg.setInputSource(source);
      reg.setInputTarget(target); reg.setInputSource(source);
    }
  {
    step("24 points: the default method is served by the device search");
    VGICPCuda reg;
    reg.setHostKdTree(false);
    const Cloud::ConstPtr big = make_cloud(24, 0.f);
    reg.setInputTarget(big); reg.setInputSource(big);
    step("a point type that is not packed xyz");
    FastVGICPCuda<PointXYZIR, PointXYZIR> wide;
    wide.setHostKdTree(false);
    const auto cloud = make_cloud<PointXYZIR>(3, 2.f);
    wide.setInputTarget(cloud); wide.setInputSource(cloud);
    wide.prepareNextSource(cloud, 1);
    wide.adoptPreparedSource();
  }
  {
    VGICPCuda reg;
    reg.setHostKdTree(false);
    step("setters");
    reg.setCorrespondenceRandomness(7); reg.setResolution(0.5); reg.setKernelWidth(0.25); reg.setKernelWidth(0.25, 2.0);
    reg.setRegularizationMethod(RegularizationMethod::FROBENIUS); reg.setNeighborSearchMethod(NeighborSearchMethod::DIRECT_RADIUS, 1.5);
    reg.setComputePrecision(FVH_COMPUTE_FP32); reg.setVoxelAccumulationMode(VoxelAccumulationMode::MULTIPLICATIVE);
    reg.setInputTarget(target); reg.setInputSource(source);
    reg.setVoxelAccumulationMode(VoxelAccumulationMode::ADDITIVE);
    drive(reg, source, target);

    step("incremental target");
    Cloud out;
    reg.setInputSource(source);
    attempt([&] { reg.beginIncrementalTarget(); });
    std::printf("  hasIncrementalTarget=%d\n", (int)reg.hasIncrementalTarget());
    inputs(reg, source, target);
    attempt([&] { reg.insertSourceIntoTarget(guess(0.125f)); });
    attempt([&] { reg.align(out, guess(0.5f)); });
    attempt([&] { reg.insertSourceIntoTarget(); });
    const double center[3] = {1.0, 2.0, 3.0};
    attempt([&] { std::printf("  removed=%d\n", reg.pruneTarget(center, 12.5, 3)); });
    attempt([&] { std::printf("  removed=%d\n", reg.pruneTarget(nullptr, 0.0)); });
    attempt([&] { reg.alignMulti({guess(0.5f)}); });
    TargetMapSnapshot snap;
    attempt([&] { snap = reg.exportTargetMap(); });
    std::printf("  snapshot: %d voxels, resolution %.9g, mode %d, %d inserts, %lld points, coords[5]=%d sums[19]=%.9g ages[1]=%u\n", snap.num_voxels(), snap.resolution, snap.mode,
                snap.num_inserts, snap.num_points, snap.coords[5], snap.sums[19], snap.ages[1]);
    attempt([&] { reg.importTargetMap(snap); });
    attempt([&] { reg.importTargetMap(TargetMapSnapshot()); });
    {
      VGICPCuda other;
      attempt([&] { reg.mergeTargetFrom(other); });
    }
    g_fail = "fvh_vgicp_swap_source_and_target";
    g_fail_skip = 0;
    attempt([&] { reg.swapSourceAndTarget(); });
    g_fail = nullptr;
    inputs(reg, source, target);
    attempt([&] { reg.setInputTarget(target); });
    std::printf("  hasIncrementalTarget=%d\n", (int)reg.hasIncrementalTarget());
    attempt([&] { reg.beginIncrementalTarget(100); });
    reg.clearSource();
    attempt([&] { reg.insertSourceIntoTarget(); });
    attempt([&] { reg.align(out); });
  }

  std::printf("#### FastGICP\n");
  for (int k : {3, 8, 0}) {
    std::printf("== setInputTarget / setInputSource, k = %d\n", k);
    GICP reg;
    reg.setCorrespondenceRandomness(k);
    attempt([&] { reg.setInputTarget(target); reg.setInputSource(source); });
    attempt([&] { reg.setInputTarget(target); reg.setInputSource(source); });
  }
  {
    GICP reg;
    step("setters");
    reg.setNumThreads(4); reg.setCorrespondenceRandomness(3); reg.setRegularizationMethod(RegularizationMethod::MIN_EIG); reg.setMaxCorrespondenceDistance(1.5);
    reg.setInputTarget(target); reg.setInputSource(source);
    step("covariances");
    attempt([&] { reg.setSourceCovariances(GICP::Covariances(4)); });
    attempt([&] { reg.setSourceCovariances(reg.getSourceCovariances()); });
    attempt([&] { reg.setTargetCovariances(reg.getTargetCovariances()); });
    drive(reg, source, target);
  }

  std::printf("#### FastVGICP\n");
  for (int k : {3, 8}) {
    std::printf("== setInputTarget / setInputSource, k = %d\n", k);
    VGICP reg;
    reg.setCorrespondenceRandomness(k);
    reg.setInputTarget(target); reg.setInputSource(source);
    reg.setInputTarget(target); reg.setInputSource(source);
  }
  {
    VGICP reg;
    step("setters");
    reg.setCorrespondenceRandomness(3); reg.setResolution(0.5); reg.setNeighborSearchMethod(NeighborSearchMethod::DIRECT7);
    attempt([&] { reg.setNeighborSearchMethod(NeighborSearchMethod::DIRECT_RADIUS); });
    reg.setVoxelAccumulationMode(VoxelAccumulationMode::ADDITIVE_WEIGHTED); reg.setMaxCorrespondenceDistance(1.5);
    reg.setInputTarget(target); reg.setInputSource(source);
    reg.setResolution(2.0); reg.setVoxelAccumulationMode(VoxelAccumulationMode::ADDITIVE);
    attempt([&] { reg.setTargetCovariances(reg.getTargetCovariances()); });
    drive(reg, source, target);
  }

  std::printf("#### NDTCuda\n");
  {
    NDT reg;
    step("setters");
    reg.setDistanceMode(NDTDistanceMode::P2D); reg.setResolution(0.5); reg.setNeighborSearchMethod(NeighborSearchMethod::DIRECT_RADIUS, 2.5);
    step("setInputTarget / setInputSource");
    reg.setInputTarget(target); reg.setInputSource(source);
    drive(reg, source, target);
    fvh_voxelgrid filter;
    attempt([&] { reg.prepareNextSourceFromFilter(&filter); });
    step("a point type that is not packed xyz");
    NDTCuda<PointXYZIR, PointXYZIR> wide;
    const auto cloud = make_cloud<PointXYZIR>(3, 2.f);
    wide.setInputTarget(cloud); wide.setInputSource(make_cloud<PointXYZIR>(2, 5.f));
    wide.prepareNextSource(cloud);
  }
  return 0;
}
