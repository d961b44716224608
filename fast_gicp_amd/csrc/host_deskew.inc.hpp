// Motion compensation of a sweep on the voxel-grid filter's handle (kernels_deskew.hpp; the contract is in include/fast_vgicp_hip.h).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_outlier.inc.hpp)
//
// The host does everything that happens once per call, in fp64: the rigidity test of the knot poses, the SE(3) logarithm of every
// segment, T(t_ref), and A_j = T(t_ref)^-1 * T[j]. The segment records travel through a pinned buffer of the handle (64 records:
// more than the engine's own pinned block holds) into a small device buffer, by one hipMemcpyAsync in front of the kernel.
// A stage of host_filter_stage.inc.hpp that keeps every point: begin, the cloud checks, the upload and the publication are that layer's.

struct DeskewDev {
  DevBuf segs, times;       // nseg DeskewSeg records; the times of a HOST call, packed
  void* host_segs = nullptr;  // pinned, (DESKEW_MAX_KNOTS - 1) records
  std::vector<float> host_times;
  void release() {
    segs.release(); times.release();
    if (host_segs) { (void)hipHostFree(host_segs); host_segs = nullptr; }
  }
};

// rigid motion on the host: x -> r x + t, r row-major
struct DeskewPose { double r[9], t[3]; };

inline DeskewPose deskew_mul(const DeskewPose& a, const DeskewPose& b) {
  DeskewPose c;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.r[i * 3 + j] = a.r[i * 3] * b.r[j] + a.r[i * 3 + 1] * b.r[3 + j] + a.r[i * 3 + 2] * b.r[6 + j];
    c.t[i] = a.r[i * 3] * b.t[0] + a.r[i * 3 + 1] * b.t[1] + a.r[i * 3 + 2] * b.t[2] + a.t[i];
  }
  return c;
}
inline DeskewPose deskew_inv(const DeskewPose& a) {  // (r^T, -r^T t)
  DeskewPose c;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.r[i * 3 + j] = a.r[j * 3 + i];
    c.t[i] = -(a.r[i] * a.t[0] + a.r[3 + i] * a.t[1] + a.r[6 + i] * a.t[2]);
  }
  return c;
}

// Finite like fvh_*_map_insert_source asks of its pose, and -- because a logarithm is taken of it -- a rotation: last row (0, 0, 0, 1),
// |R^T R - I| <= 1e-6 entrywise, det R > 0.
inline bool deskew_rigid(const double* T) {
  for (int i = 0; i < 16; i++) if (!std::isfinite(T[i])) return false;
  if (std::fabs(T[3]) > 1e-9 || std::fabs(T[7]) > 1e-9 || std::fabs(T[11]) > 1e-9 || std::fabs(T[15] - 1.0) > 1e-9) return false;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double g = T[i * 4] * T[j * 4] + T[i * 4 + 1] * T[j * 4 + 1] + T[i * 4 + 2] * T[j * 4 + 2];  // columns i and j
      if (std::fabs(g - (i == j ? 1.0 : 0.0)) > 1e-6) return false;
    }
  const double det = T[0] * (T[5] * T[10] - T[9] * T[6]) - T[4] * (T[1] * T[10] - T[9] * T[2]) + T[8] * (T[1] * T[6] - T[5] * T[2]);
  return det > 0.0;
}

// SE(3) logarithm, rotation first: xi = (w, v) with exp(xi) = m. The rotation goes through the unit quaternion (largest-component
// extraction), w = 2 atan2(|q_v|, q_w) q_v / |q_v|: well conditioned up to pi. v = V^-1 t, V^-1 = I - K / 2 + d K^2,
// d = (1 - (th / 2) cot(th / 2)) / th^2 (1/12 below 1e-5 rad). Returns the rotation angle.
inline double deskew_se3_log(const DeskewPose& m, double* w, double* v) {
  const double* r = m.r;
  const double tr = r[0] + r[4] + r[8];
  double q[4];  // w, x, y, z
  if (tr > 0.0) {
    const double s = std::sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (r[7] - r[5]) / s; q[2] = (r[2] - r[6]) / s; q[3] = (r[3] - r[1]) / s;
  } else if (r[0] > r[4] && r[0] > r[8]) {
    const double s = std::sqrt(1.0 + r[0] - r[4] - r[8]) * 2.0;
    q[0] = (r[7] - r[5]) / s; q[1] = 0.25 * s; q[2] = (r[1] + r[3]) / s; q[3] = (r[2] + r[6]) / s;
  } else if (r[4] > r[8]) {
    const double s = std::sqrt(1.0 + r[4] - r[0] - r[8]) * 2.0;
    q[0] = (r[2] - r[6]) / s; q[1] = (r[1] + r[3]) / s; q[2] = 0.25 * s; q[3] = (r[5] + r[7]) / s;
  } else {
    const double s = std::sqrt(1.0 + r[8] - r[0] - r[4]) * 2.0;
    q[0] = (r[3] - r[1]) / s; q[1] = (r[2] + r[6]) / s; q[2] = (r[5] + r[7]) / s; q[3] = 0.25 * s;
  }
  if (q[0] < 0.0) for (int i = 0; i < 4; i++) q[i] = -q[i];
  const double nv = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double th = 2.0 * std::atan2(nv, q[0]);
  const double f = nv < 1e-12 ? 2.0 / q[0] : th / nv;
  for (int i = 0; i < 3; i++) w[i] = f * q[1 + i];
  const double d = th < 1e-5 ? 1.0 / 12.0 : (1.0 - 0.5 * th * std::cos(0.5 * th) / std::sin(0.5 * th)) / (th * th);
  const double* t = m.t;
  const double k1[3] = {w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0]};
  const double k2[3] = {w[1] * k1[2] - w[2] * k1[1], w[2] * k1[0] - w[0] * k1[2], w[0] * k1[1] - w[1] * k1[0]};
  for (int i = 0; i < 3; i++) v[i] = t[i] - 0.5 * k1[i] + d * k2[i];
  return th;
}

// exp(s * (w, v)) as a pose, by the formulas of deskew_se3_exp_apply (kernels_deskew.hpp)
inline DeskewPose deskew_se3_exp(const double* w_, const double* v_, double s) {
  const double w[3] = {s * w_[0], s * w_[1], s * w_[2]}, u[3] = {s * v_[0], s * v_[1], s * v_[2]};
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  double a = 1.0, b = 0.5, c = 1.0 / 6.0;
  if (th >= 1e-10) {
    const double sh = std::sin(0.5 * th), ch = std::cos(0.5 * th), sn = 2.0 * sh * ch;
    a = sn / th;
    b = 2.0 * sh * sh / th2;
    c = (th - sn) / (th2 * th);
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double K2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) K2[i * 3 + j] = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
  DeskewPose e;
  for (int i = 0; i < 3; i++) {
    e.t[i] = 0.0;
    for (int j = 0; j < 3; j++) {
      const double id = i == j ? 1.0 : 0.0;
      e.r[i * 3 + j] = id + a * K[i * 3 + j] + b * K2[i * 3 + j];
      e.t[i] += (id + b * K[i * 3 + j] + c * K2[i * 3 + j]) * u[j];
    }
  }
  return e;
}

// the largest j with tau[j] <= x, clamped to [0, K - 2]
inline int deskew_segment(const double* tau, int K, double x) {
  int j = 0;
  while (j < K - 2 && tau[j + 1] <= x) j++;
  return j;
}

int deskew(Engine* e, DownsampleDev& d, OutlierDev& o, DeskewDev& k, const float* xyz, int n, int stride, bool on_device, const float* times, int time_stride,
           const double* knot_times, const double* knot_poses, int K, double t_ref, int* out_n) {
  stage_begin(e, d, o);
  if (!out_n) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: null out_n");
  *out_n = 0;
  int rc = stage_check_cloud(e, "deskew", xyz && times, n, stride, "points or times");
  if (rc) return rc;
  if (time_stride < 1) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: time_stride must be >= 1");
  if (K < 2 || K > DESKEW_MAX_KNOTS) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: the number of knots must be in [2, 64]");
  if (!knot_times || !knot_poses) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: null knots");
  if (!std::isfinite(t_ref)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: t_ref must be finite");
  for (int j = 0; j < K; j++) {
    if (!std::isfinite(knot_times[j]) || (j > 0 && !(knot_times[j] > knot_times[j - 1]))) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: the knot times must be finite and strictly increasing");
    if (!deskew_rigid(knot_poses + 16 * j)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: knot pose " + std::to_string(j) + " is not a rigid motion");
  }
  const int nseg = K - 1;
  DeskewPose T[DESKEW_MAX_KNOTS];
  double w[DESKEW_MAX_KNOTS][3], v[DESKEW_MAX_KNOTS][3];
  for (int j = 0; j < K; j++) {
    const PoseD p = pose_from_colmajor16(knot_poses + 16 * j);
    std::memcpy(T[j].r, p.r, sizeof(p.r));
    std::memcpy(T[j].t, p.t, sizeof(p.t));
  }
  for (int j = 0; j < nseg; j++) {
    const double th = deskew_se3_log(deskew_mul(deskew_inv(T[j]), T[j + 1]), w[j], v[j]);
    if (!(th <= 3.14159265358979323846 - 1e-6)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "deskew: segment " + std::to_string(j) + " turns by more than pi - 1e-6: its logarithm is not unique");
  }
  if (n == 0) return stage_publish(e, d, o, LAST_DESKEW, 0, out_n);
  if (!k.host_segs) HIP_OR_FAIL(e, hipHostMalloc(&k.host_segs, sizeof(DeskewSeg) * (DESKEW_MAX_KNOTS - 1), hipHostMallocDefault));
  {
    const int jr = deskew_segment(knot_times, K, t_ref);
    const double sr = (t_ref - knot_times[jr]) / (knot_times[jr + 1] - knot_times[jr]);
    const DeskewPose ref_inv = deskew_inv(deskew_mul(T[jr], deskew_se3_exp(w[jr], v[jr], sr)));
    DeskewSeg* hs = static_cast<DeskewSeg*>(k.host_segs);
    for (int j = 0; j < nseg; j++) {
      const DeskewPose A = deskew_mul(ref_inv, T[j]);
      for (int i = 0; i < 3; i++) {
        for (int c = 0; c < 3; c++) hs[j].a[i * 4 + c] = A.r[i * 3 + c];
        hs[j].a[i * 4 + 3] = A.t[i];
        hs[j].w[i] = w[j][i];
        hs[j].v[i] = v[j][i];
      }
      hs[j].tau = knot_times[j];
      hs[j].inv_dt = 1.0 / (knot_times[j + 1] - knot_times[j]);
    }
  }
  if ((rc = stage_upload(e, d, xyz, n, stride, on_device))) return rc;
  const float* d_times = times;
  int d_time_stride = time_stride;
  if (!on_device) {
    k.host_times.resize((size_t)n);
    for (int i = 0; i < n; i++) k.host_times[i] = times[(size_t)i * time_stride];
    HIP_OR_FAIL(e, k.times.ensure(sizeof(float) * (size_t)n));
    HIP_OR_FAIL(e, hipMemcpyAsync(k.times.p, k.host_times.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    d_times = k.times.as<float>();
    d_time_stride = 1;
  }
  HIP_OR_FAIL(e, k.segs.ensure(sizeof(DeskewSeg) * (DESKEW_MAX_KNOTS - 1)));
  HIP_OR_FAIL(e, hipMemcpyAsync(k.segs.p, k.host_segs, sizeof(DeskewSeg) * (size_t)nseg, hipMemcpyHostToDevice, e->stream));
  {
    ProfScope ps(e, "deskew");
    deskew_points_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, d_times, d_time_stride, k.segs.as<double>(), nseg, d.out.as<float>(), d.out4.as<float4>());
  }
  HIP_OR_FAIL(e, hipGetLastError());
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return stage_publish(e, d, o, LAST_DESKEW, n, out_n);
}
