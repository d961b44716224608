// RANSAC plane segmentation on the voxel-grid filter's handle (kernels_plane.hpp; the contract is in include/fast_vgicp_hip.h).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_cluster.inc.hpp)
//
// The call writes the handle's output state and the side outputs of an outlier filter (OutlierDev: keep flags, scanned positions, scores,
// kept indices), so get_points, device_points, fvh_ndt_*_from_voxelgrid, get_kept_indices and get_scores work on the result unchanged;
// the hypotheses, their counts and the model are its own (PlaneDev). The input may be the handle's own output: it is widened into
// d.cloud FIRST. No Morton sort: the samples are input indices and the sweep is dense. One stream, one synchronisation, one readback
// (PlaneCtl): winner, refit and the final labelling all happen on the device.

struct PlaneDev {
  DevBuf hyp, counts, part;  // PlaneHyp and count per hypothesis; the refit's partial sums
  bool valid = false;        // the last call on the handle was segment_plane (and succeeded)
  int H = 0;
  double coef[4] = {0, 0, 0, 0};
  int sample[3] = {0, 0, 0};
  int info[4] = {-1, 0, 0, 0};  // winner, valid hypotheses, count_winner, num_inliers
  void release() { hyp.release(); counts.release(); part.release(); }
};

int segment_plane(Engine* e, DownsampleDev& d, OutlierDev& o, PlaneDev& pl, const float* xyz, int n, int stride, bool on_device, double threshold, int max_iterations,
                  unsigned long long seed, const double* axis, double eps_angle, int flags_in, double* coefficients, int* num_inliers, int* out_n) {
#pragma clang fp contract(off)
  if (e->stream_owner) e->stream_owner->quiet = false;  // work on a borrowed stream (see downsample())
  o.valid = false;
  o.cluster = false;
  pl.valid = false;
  d.out_n = 0;
  d.out4_valid = false;
  if (out_n) *out_n = 0;
  if (num_inliers) *num_inliers = 0;
  if (coefficients) for (int k = 0; k < 4; k++) coefficients[k] = 0.0;
  if (!out_n || !num_inliers || !coefficients) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: null coefficients / num_inliers / out_n");
  if (n < 0 || (n > 0 && !xyz)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: null points");
  if (stride != 3 && stride != 4) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: stride must be 3 or 4 floats");
  if (!std::isfinite(threshold) || !(threshold > 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: distance_threshold must be finite and > 0");
  if (max_iterations < 1 || max_iterations > PLANE_MAX_HYP) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: max_iterations must be in [1, 16384]");
  if (flags_in & ~(FVH_PLANE_KEEP_OUTLIERS | FVH_PLANE_REFINE)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: unknown flag bits");
  double ax = 0.0, ay = 0.0, az = 0.0, aa = 0.0, c2 = 0.0;
  if (axis) {
    ax = axis[0]; ay = axis[1]; az = axis[2];
    if (!std::isfinite(ax) || !std::isfinite(ay) || !std::isfinite(az)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: the axis must be finite");
    aa = (ax * ax + ay * ay) + az * az;
    if (!(aa > 0.0) || !std::isfinite(aa)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: the axis must not be zero");
    if (!(eps_angle >= 0.0 && eps_angle <= 1.5707963267948966)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: eps_angle must be in [0, pi/2]");
    const double ce = std::cos(eps_angle);
    c2 = ce * ce;
  }
  const int H = max_iterations;
  const bool refine = (flags_in & FVH_PLANE_REFINE) != 0;
  const double t2 = threshold * threshold;
  o.n_in = n;
  o.threshold = threshold;
  pl.H = H;
  for (int k = 0; k < 4; k++) pl.coef[k] = 0.0;
  pl.sample[0] = pl.sample[1] = pl.sample[2] = 0;
  pl.info[0] = -1; pl.info[1] = pl.info[2] = pl.info[3] = 0;
  HIP_OR_FAIL(e, pl.counts.ensure(sizeof(int) * (size_t)H));
  if (n == 0) {
    HIP_OR_FAIL(e, hipMemsetAsync(pl.counts.p, 0xff, sizeof(int) * (size_t)H, e->stream));  // every hypothesis invalid: -1
    o.valid = true;
    pl.valid = true;
    return FVH_OK;
  }
  int rc = upload_cloud(e, d.cloud, xyz, n, stride, on_device, false);  // before anything below writes d.out / d.out4: xyz may alias them
  if (rc) return rc;
  const size_t words = sizeof(int) * (size_t)n;
  const int rblocks = (n + PLANE_REFIT_ITEMS - 1) / PLANE_REFIT_ITEMS;
  HIP_OR_FAIL(e, o.flags.ensure(words));
  HIP_OR_FAIL(e, o.pos.ensure(words));
  HIP_OR_FAIL(e, o.score.ensure(words));
  HIP_OR_FAIL(e, o.kept.ensure(words));
  HIP_OR_FAIL(e, o.ctl.ensure(sizeof(PlaneCtl)));
  HIP_OR_FAIL(e, pl.hyp.ensure(sizeof(PlaneHyp) * (size_t)H));
  if (refine) HIP_OR_FAIL(e, pl.part.ensure(sizeof(double) * PLANE_MOMENTS * (size_t)rblocks));
  HIP_OR_FAIL(e, d.out.ensure(sizeof(float) * 3 * (size_t)n));   // (never a reallocation when xyz is this buffer: its n points fit)
  HIP_OR_FAIL(e, d.out4.ensure(sizeof(float4) * (size_t)n));
  HIP_OR_FAIL(e, hipMemsetAsync(o.ctl.p, 0, sizeof(PlaneCtl), e->stream));
  PlaneCtl* ctl = o.ctl.as<PlaneCtl>();
  unsigned* flags = o.flags.as<unsigned>();
  const float4* pts = d.cloud.pts.as<float4>();
  const int blocks = (n + 255) / 256;
  outlier_finite_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, &ctl->o);
  HIP_OR_FAIL(e, hipGetLastError());
  {
    ProfScope ps(e, "plane");
    plane_hypo_kernel<<<(H + 255) / 256, 256, 0, e->stream>>>(pts, n, H, plane_seed_word(seed), axis ? 1 : 0, ax, ay, az, aa, c2, pl.hyp.as<PlaneHyp>(), pl.counts.as<int>());
    const dim3 grid((unsigned)((n + PLANE_SLAB - 1) / PLANE_SLAB), (unsigned)((H + 255) / 256));
    plane_sweep_kernel<<<grid, 256, 0, e->stream>>>(pts, n, H, t2, pl.hyp.as<PlaneHyp>(), pl.counts.as<int>());
    plane_winner_kernel<<<1, 64, 0, e->stream>>>(H, pl.hyp.as<PlaneHyp>(), pl.counts.as<int>(), ctl);
    if (refine) {
      plane_refit_partial_kernel<<<rblocks, 256, 0, e->stream>>>(pts, n, t2, ctl, pl.part.as<double>());
      plane_refit_final_kernel<<<1, 64, 0, e->stream>>>(rblocks, pl.part.as<double>(), ctl);
    }
  }
  HIP_OR_FAIL(e, hipGetLastError());
  {
    ProfScope ps(e, "compact");
    plane_flag_kernel<<<blocks, 256, 0, e->stream>>>(pts, n, t2, (flags_in & FVH_PLANE_KEEP_OUTLIERS) ? 1 : 0, ctl, flags, o.score.as<float>());
    HIP_OR_FAIL(e, hipGetLastError());
    const unsigned* total_dev = nullptr;
    if ((rc = device_scan(e, d.bsums, flags, n, o.pos.as<unsigned>(), &total_dev))) return rc;
    outlier_compact_kernel<<<blocks, 256, 0, e->stream>>>(pts, n, flags, o.pos.as<unsigned>(), total_dev, d.out.as<float>(), d.out4.as<float4>(), o.kept.as<int>(), &ctl->o);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  PlaneCtl* h = reinterpret_cast<PlaneCtl*>(e->pinned);
  HIP_OR_FAIL(e, hipMemcpyAsync(h, ctl, sizeof(PlaneCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  if (h->o.bad) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: non-finite coordinates in the input");
  d.out_n = (int)h->o.count;
  d.out4_valid = d.out_n > 0;
  d.out_stream = e->stream;
  d.out_complete = true;
  const int inliers = (flags_in & FVH_PLANE_KEEP_OUTLIERS) ? n - d.out_n : d.out_n;
  if (h->winner >= 0) {
    const PlaneHyp& w = h->win;
    if (h->refit) {
      for (int k = 0; k < 4; k++) pl.coef[k] = h->coef[k];
    } else {  // the winner's plane, normalised: one square root, three divisions
      const double norm = std::sqrt(w.nn);
      pl.coef[0] = w.a / norm; pl.coef[1] = w.b / norm; pl.coef[2] = w.c / norm;
      pl.coef[3] = -((pl.coef[0] * w.qx + pl.coef[1] * w.qy) + pl.coef[2] * w.qz);
      plane_fix_sign(pl.coef);
    }
    pl.sample[0] = w.i0; pl.sample[1] = w.i1; pl.sample[2] = w.i2;
  }
  pl.info[0] = h->winner; pl.info[1] = h->nvalid; pl.info[2] = h->count_w; pl.info[3] = inliers;
  o.valid = true;
  pl.valid = true;
  for (int k = 0; k < 4; k++) coefficients[k] = pl.coef[k];
  *num_inliers = inliers;
  *out_n = d.out_n;
  return FVH_OK;
}

int plane_get_model(Engine* e, OutlierDev& o, PlaneDev& pl, double* coefficients, int* sample, int* info, int* counts) {
  if (!o.valid || !pl.valid) return e->fail(FVH_ERR_BAD_STATE, "get_plane_model: the last call on this handle was not segment_plane");
  if (coefficients) for (int k = 0; k < 4; k++) coefficients[k] = pl.coef[k];
  if (sample) for (int k = 0; k < 3; k++) sample[k] = pl.sample[k];
  if (info) for (int k = 0; k < 4; k++) info[k] = pl.info[k];
  if (counts && pl.H > 0) {
    HIP_OR_FAIL(e, hipMemcpyAsync(counts, pl.counts.p, sizeof(int) * (size_t)pl.H, hipMemcpyDefault, e->stream));
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  }
  return FVH_OK;
}
