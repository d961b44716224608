// Range crop, statistical and radius outlier removal on the voxel-grid filter's handle (kernels_outlier.hpp).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_filter_stage.inc.hpp)
//
// Three mask stages of host_filter_stage.inc.hpp (which holds OutlierDev, the output-state contract and the chaining rule).

enum OutlierKind { OUTLIER_CROP = 0, OUTLIER_STATISTICAL = 1, OUTLIER_RADIUS = 2 };

// p0 / p1 / k: crop {min_sq_norm, max_sq_norm, -}, statistical {stddev_mul, -, mean_k}, radius {radius, -, min_neighbors}
int outlier_filter(Engine* e, DownsampleDev& d, OutlierDev& o, int kind, const float* xyz, int n, int stride, bool on_device, double p0, double p1, int k, int* out_n) {
  stage_begin(e, d, o);
  if (!out_n) return e->fail(FVH_ERR_INVALID_ARGUMENT, "outlier filter: null out_n");
  *out_n = 0;
  int rc = stage_check_cloud(e, "outlier filter", xyz != nullptr, n, stride);
  if (rc) return rc;
  if (kind == OUTLIER_CROP) {
    if (std::isnan(p0) || std::isnan(p1)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "crop_range: the bounds must not be NaN");
  } else if (kind == OUTLIER_STATISTICAL) {
    if (k < 1 || k > 63) return e->fail(FVH_ERR_INVALID_ARGUMENT, "remove_statistical_outliers: mean_k must be in [1, 63]");
    if (!std::isfinite(p0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "remove_statistical_outliers: stddev_mul must be finite");
    if (n > 0 && n <= k) return e->fail(FVH_ERR_INVALID_ARGUMENT, "remove_statistical_outliers: the cloud must hold more than mean_k points");
  } else {
    if (!std::isfinite(p0) || !(p0 > 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "remove_radius_outliers: radius must be finite and > 0");
    if (k < 1) return e->fail(FVH_ERR_INVALID_ARGUMENT, "remove_radius_outliers: min_neighbors must be >= 1");
  }
  o.n_in = n;
  o.threshold = kind == OUTLIER_CROP ? p1 : (kind == OUTLIER_RADIUS ? (double)k : std::nan(""));
  if (n == 0) return stage_publish(e, d, o, LAST_OUTLIER, 0, out_n);
  if ((rc = mask_stage_setup(e, d, o, xyz, n, stride, on_device, sizeof(OutlierCtl), kind != OUTLIER_CROP))) return rc;
  OutlierCtl* ctl = o.ctl.as<OutlierCtl>();
  unsigned* flags = o.flags.as<unsigned>();
  float* score = o.score.as<float>();
  const int blocks = (n + 255) / 256;
  if (kind == OUTLIER_CROP) {
    ProfScope ps(e, "compact");
    crop_flag_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, p0, p1, flags, score);
  } else if (kind == OUTLIER_RADIUS) {
    if ((rc = ensure_sorted(e, d.cloud))) return rc;
    const float r = (float)p0;
    const float r2 = fminf(r * r, 1e37f);  // below the 2.7e37 of a slot past the end of the cloud (calc_cov_rbf clamps md_sq the same way)
    ProfScope ps(e, "outlier_count");
    outlier_radius_count_kernel<<<(n + 3) / 4, 256, 0, e->stream>>>(d.cloud.sorted.as<float4>(), d.cloud.bbox.as<float4>(), d.cloud.bbox2.as<float4>(), n, r2, k, flags, score);
  } else {
    const int k1 = k + 1;  // "search mean_k + 1, skip the first"
    if ((rc = find_neighbors(e, d.cloud, k1))) return rc;
    {
      ProfScope ps(e, "outlier_score");
      const int lblocks = (int)(((long long)n * OUTLIER_LANES + 255) / 256);
      if (k1 <= 24) outlier_mean_dist_kernel<6><<<lblocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, k1, d.cloud.nbr.as<int>(), score);
      else outlier_mean_dist_kernel<16><<<lblocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, k1, d.cloud.nbr.as<int>(), score);
      outlier_stats_kernel<<<1, 1024, 0, e->stream>>>(score, n, p0, ctl);
    }
    HIP_OR_FAIL(e, hipGetLastError());
    ProfScope ps(e, "compact");
    outlier_flag_kernel<<<blocks, 256, 0, e->stream>>>(score, n, ctl, flags);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  {
    ProfScope ps(e, "compact");
    if ((rc = mask_stage_compact(e, d, o, n))) return rc;
  }
  if ((rc = mask_stage_finish(e, d, o, sizeof(OutlierCtl), "outlier filter", LAST_OUTLIER, out_n))) return rc;
  if (kind == OUTLIER_STATISTICAL) o.threshold = reinterpret_cast<const OutlierCtl*>(e->pinned)->threshold;
  return FVH_OK;
}

int outlier_get_kept(Engine* e, DownsampleDev& d, OutlierDev& o, int* idx) {
  if (!o.has_kept()) return e->fail(FVH_ERR_BAD_STATE, "get_kept_indices: the last call on this handle was not crop_range / remove_statistical_outliers / remove_radius_outliers / cluster_euclidean");
  if (d.out_n == 0) return FVH_OK;
  if (!idx) return e->fail(FVH_ERR_INVALID_ARGUMENT, "get_kept_indices: null output");
  HIP_OR_FAIL(e, hipMemcpyAsync(idx, o.kept.p, sizeof(int) * (size_t)d.out_n, hipMemcpyDefault, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return FVH_OK;
}

int outlier_get_scores(Engine* e, OutlierDev& o, float* scores, double* threshold) {
  if (!o.has_kept()) return e->fail(FVH_ERR_BAD_STATE, "get_scores: the last call on this handle was not crop_range / remove_statistical_outliers / remove_radius_outliers / cluster_euclidean");
  if (threshold) *threshold = o.threshold;
  if (scores && o.n_in > 0) {
    HIP_OR_FAIL(e, hipMemcpyAsync(scores, o.score.p, sizeof(float) * (size_t)o.n_in, hipMemcpyDefault, e->stream));
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  }
  return FVH_OK;
}
