// RANSAC plane segmentation on the voxel-grid filter's handle (kernels_plane.hpp; the contract is in include/fast_vgicp_hip.h).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_cluster.inc.hpp)
//
// A mask stage of host_filter_stage.inc.hpp: get_kept_indices and get_scores work on its result as after an outlier filter; the
// hypotheses, their counts and the model are its own (PlaneDev). No Morton sort: the samples are input indices and the sweep is dense.
// One stream, one synchronisation, one readback (PlaneCtl): winner, refit and the final labelling all happen on the device.

struct PlaneDev {
  DevBuf hyp, counts, part;  // PlaneHyp and count per hypothesis; the refit's partial sums
  int H = 0;
  double coef[4] = {0, 0, 0, 0};
  int sample[3] = {0, 0, 0};
  int info[4] = {-1, 0, 0, 0};  // winner, valid hypotheses, count_winner, num_inliers
  void release() { hyp.release(); counts.release(); part.release(); }
};

int segment_plane(Engine* e, DownsampleDev& d, OutlierDev& o, PlaneDev& pl, const float* xyz, int n, int stride, bool on_device, double threshold, int max_iterations,
                  unsigned long long seed, const double* axis, double eps_angle, int flags_in, double* coefficients, int* num_inliers, int* out_n) {
#pragma clang fp contract(off)
  stage_begin(e, d, o);
  if (out_n) *out_n = 0;
  if (num_inliers) *num_inliers = 0;
  if (coefficients) for (int k = 0; k < 4; k++) coefficients[k] = 0.0;
  if (!out_n || !num_inliers || !coefficients) return e->fail(FVH_ERR_INVALID_ARGUMENT, "segment_plane: null coefficients / num_inliers / out_n");
  int rc = stage_check_cloud(e, "segment_plane", xyz != nullptr, n, stride);
  if (rc) return rc;
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
    return stage_publish(e, d, o, LAST_PLANE, 0, out_n);
  }
  const int rblocks = (n + PLANE_REFIT_ITEMS - 1) / PLANE_REFIT_ITEMS;
  HIP_OR_FAIL(e, pl.hyp.ensure(sizeof(PlaneHyp) * (size_t)H));
  if (refine) HIP_OR_FAIL(e, pl.part.ensure(sizeof(double) * PLANE_MOMENTS * (size_t)rblocks));
  if ((rc = mask_stage_setup(e, d, o, xyz, n, stride, on_device, sizeof(PlaneCtl)))) return rc;
  PlaneCtl* ctl = o.ctl.as<PlaneCtl>();
  unsigned* flags = o.flags.as<unsigned>();
  const float4* pts = d.cloud.pts.as<float4>();
  const int blocks = (n + 255) / 256;
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
    if ((rc = mask_stage_compact(e, d, o, n))) return rc;
  }
  if ((rc = mask_stage_finish(e, d, o, sizeof(PlaneCtl), "segment_plane", LAST_PLANE, out_n))) return rc;
  const PlaneCtl* h = reinterpret_cast<const PlaneCtl*>(e->pinned);
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
  for (int k = 0; k < 4; k++) coefficients[k] = pl.coef[k];
  *num_inliers = inliers;
  return FVH_OK;
}

int plane_get_model(Engine* e, OutlierDev& o, PlaneDev& pl, double* coefficients, int* sample, int* info, int* counts) {
  if (o.last != LAST_PLANE) return e->fail(FVH_ERR_BAD_STATE, "get_plane_model: the last call on this handle was not segment_plane");
  if (coefficients) for (int k = 0; k < 4; k++) coefficients[k] = pl.coef[k];
  if (sample) for (int k = 0; k < 3; k++) sample[k] = pl.sample[k];
  if (info) for (int k = 0; k < 4; k++) info[k] = pl.info[k];
  if (counts && pl.H > 0) {
    HIP_OR_FAIL(e, hipMemcpyAsync(counts, pl.counts.p, sizeof(int) * (size_t)pl.H, hipMemcpyDefault, e->stream));
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  }
  return FVH_OK;
}
