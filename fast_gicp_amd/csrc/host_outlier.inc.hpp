// Range crop, statistical and radius outlier removal on the voxel-grid filter's handle (kernels_outlier.hpp).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_downsample.inc.hpp)
//
// The three filters write the handle's output state (DownsampleDev::out / out4 / out_n) like a voxel filter does, so get_points,
// device_points and fvh_ndt_*_from_voxelgrid work on the result unchanged. The input may be that very output (chaining on one handle):
// it is widened into d.cloud FIRST (upload_cloud), and everything that writes out / out4 is queued behind that kernel on the same stream.

struct OutlierDev {
  DevBuf flags, pos, score, kept, ctl;  // keep flag and scanned position per input point, its score, kept indices, OutlierCtl
  bool valid = false;                   // the last call on the handle was one of the three filters below or cluster_euclidean (and succeeded)
  bool cluster = false;                 // ... and it was cluster_euclidean (host_cluster.inc.hpp): labels and cluster sizes exist too
  int n_in = 0;
  double threshold = 0.0;
  void release() { flags.release(); pos.release(); score.release(); kept.release(); ctl.release(); }
};

enum OutlierKind { OUTLIER_CROP = 0, OUTLIER_STATISTICAL = 1, OUTLIER_RADIUS = 2 };

// p0 / p1 / k: crop {min_sq_norm, max_sq_norm, -}, statistical {stddev_mul, -, mean_k}, radius {radius, -, min_neighbors}
int outlier_filter(Engine* e, DownsampleDev& d, OutlierDev& o, int kind, const float* xyz, int n, int stride, bool on_device, double p0, double p1, int k, int* out_n) {
  if (e->stream_owner) e->stream_owner->quiet = false;  // work on a borrowed stream (see downsample())
  o.valid = false;
  o.cluster = false;
  d.out_n = 0;
  d.out4_valid = false;
  if (!out_n) return e->fail(FVH_ERR_INVALID_ARGUMENT, "outlier filter: null out_n");
  *out_n = 0;
  if (n < 0 || (n > 0 && !xyz)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "outlier filter: null points");
  if (stride != 3 && stride != 4) return e->fail(FVH_ERR_INVALID_ARGUMENT, "outlier filter: stride must be 3 or 4 floats");
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
  if (n == 0) { o.valid = true; return FVH_OK; }
  int rc = upload_cloud(e, d.cloud, xyz, n, stride, on_device, false);  // before anything below writes d.out / d.out4: xyz may alias them
  if (rc) return rc;
  HIP_OR_FAIL(e, o.flags.ensure(sizeof(unsigned) * (size_t)n));
  HIP_OR_FAIL(e, o.pos.ensure(sizeof(unsigned) * (size_t)n));
  HIP_OR_FAIL(e, o.score.ensure(sizeof(float) * (size_t)n));
  HIP_OR_FAIL(e, o.kept.ensure(sizeof(int) * (size_t)n));
  HIP_OR_FAIL(e, o.ctl.ensure(sizeof(OutlierCtl)));
  HIP_OR_FAIL(e, d.out.ensure(sizeof(float) * 3 * (size_t)n));   // (never a reallocation when xyz is this buffer: its n points fit)
  HIP_OR_FAIL(e, d.out4.ensure(sizeof(float4) * (size_t)n));
  HIP_OR_FAIL(e, hipMemsetAsync(o.ctl.p, 0, sizeof(OutlierCtl), e->stream));
  OutlierCtl* ctl = o.ctl.as<OutlierCtl>();
  unsigned* flags = o.flags.as<unsigned>();
  float* score = o.score.as<float>();
  const int blocks = (n + 255) / 256;
  if (kind == OUTLIER_CROP) {
    ProfScope ps(e, "compact");
    crop_flag_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, p0, p1, flags, score);
  } else {
    outlier_finite_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, ctl);
    HIP_OR_FAIL(e, hipGetLastError());
    if (kind == OUTLIER_RADIUS) {
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
  }
  HIP_OR_FAIL(e, hipGetLastError());
  {
    ProfScope ps(e, "compact");
    const unsigned* total_dev = nullptr;
    if ((rc = device_scan(e, d.bsums, flags, n, o.pos.as<unsigned>(), &total_dev))) return rc;
    outlier_compact_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, flags, o.pos.as<unsigned>(), total_dev, d.out.as<float>(), d.out4.as<float4>(), o.kept.as<int>(), ctl);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  OutlierCtl* h = reinterpret_cast<OutlierCtl*>(e->pinned);
  HIP_OR_FAIL(e, hipMemcpyAsync(h, ctl, sizeof(OutlierCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  if (h->bad) return e->fail(FVH_ERR_INVALID_ARGUMENT, "outlier filter: non-finite coordinates in the input");
  if (kind == OUTLIER_STATISTICAL) o.threshold = h->threshold;
  d.out_n = (int)h->count;
  d.out4_valid = d.out_n > 0;
  d.out_stream = e->stream;
  d.out_complete = true;
  o.valid = true;
  *out_n = d.out_n;
  return FVH_OK;
}

int outlier_get_kept(Engine* e, DownsampleDev& d, OutlierDev& o, int* idx) {
  if (!o.valid) return e->fail(FVH_ERR_BAD_STATE, "get_kept_indices: the last call on this handle was not crop_range / remove_statistical_outliers / remove_radius_outliers / cluster_euclidean");
  if (d.out_n == 0) return FVH_OK;
  if (!idx) return e->fail(FVH_ERR_INVALID_ARGUMENT, "get_kept_indices: null output");
  HIP_OR_FAIL(e, hipMemcpyAsync(idx, o.kept.p, sizeof(int) * (size_t)d.out_n, hipMemcpyDefault, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return FVH_OK;
}

int outlier_get_scores(Engine* e, OutlierDev& o, float* scores, double* threshold) {
  if (!o.valid) return e->fail(FVH_ERR_BAD_STATE, "get_scores: the last call on this handle was not crop_range / remove_statistical_outliers / remove_radius_outliers / cluster_euclidean");
  if (threshold) *threshold = o.threshold;
  if (scores && o.n_in > 0) {
    HIP_OR_FAIL(e, hipMemcpyAsync(scores, o.score.p, sizeof(float) * (size_t)o.n_in, hipMemcpyDefault, e->stream));
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  }
  return FVH_OK;
}
