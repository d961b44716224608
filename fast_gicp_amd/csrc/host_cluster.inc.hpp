// Euclidean cluster extraction on the voxel-grid filter's handle (kernels_cluster.hpp; the contract is in include/fast_vgicp_hip.h).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_outlier.inc.hpp)
//
// The call writes the handle's output state and the side outputs of an outlier filter (OutlierDev: keep flags, scanned positions, scores,
// kept indices), so get_points, device_points, fvh_ndt_*_from_voxelgrid, get_kept_indices and get_scores work on the result unchanged;
// labels and cluster sizes are its own (ClusterDev). The input may be the handle's own output: it is widened into d.cloud FIRST.
// One stream, one synchronisation, one readback (ClusterCtl).

struct ClusterDev {
  DevBuf parent, root_in, csize, cmin;  // union-find over sorted positions; per input point its root; per root the size and smallest input index
  DevBuf lead, lpos, labels, sizes;     // leader flags and their scan; the label per input point; the size per cluster
  int num_clusters = 0;
  void release() { parent.release(); root_in.release(); csize.release(); cmin.release(); lead.release(); lpos.release(); labels.release(); sizes.release(); }
};

int cluster_euclidean(Engine* e, DownsampleDev& d, OutlierDev& o, ClusterDev& c, const float* xyz, int n, int stride, bool on_device, double tolerance, int min_size, int max_size,
                      int* num_clusters, int* out_n) {
  if (e->stream_owner) e->stream_owner->quiet = false;  // work on a borrowed stream (see downsample())
  o.valid = false;
  o.cluster = false;
  c.num_clusters = 0;
  d.out_n = 0;
  d.out4_valid = false;
  if (out_n) *out_n = 0;
  if (num_clusters) *num_clusters = 0;
  if (!out_n || !num_clusters) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: null out_n / num_clusters");
  if (n < 0 || (n > 0 && !xyz)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: null points");
  if (stride != 3 && stride != 4) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: stride must be 3 or 4 floats");
  if (!std::isfinite(tolerance) || !(tolerance > 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: tolerance must be finite and > 0");
  if (min_size < 1) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: min_cluster_size must be >= 1");
  if (max_size > 0 && max_size < min_size) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: max_cluster_size must be <= 0 (no upper bound) or >= min_cluster_size");
  o.n_in = n;
  o.threshold = (double)min_size;
  if (n == 0) { o.valid = true; o.cluster = true; return FVH_OK; }
  int rc = upload_cloud(e, d.cloud, xyz, n, stride, on_device, false);  // before anything below writes d.out / d.out4: xyz may alias them
  if (rc) return rc;
  const size_t words = sizeof(int) * (size_t)n;
  HIP_OR_FAIL(e, o.flags.ensure(words));
  HIP_OR_FAIL(e, o.pos.ensure(words));
  HIP_OR_FAIL(e, o.score.ensure(words));
  HIP_OR_FAIL(e, o.kept.ensure(words));
  HIP_OR_FAIL(e, o.ctl.ensure(sizeof(ClusterCtl)));
  for (DevBuf* b : {&c.parent, &c.root_in, &c.csize, &c.cmin, &c.lead, &c.lpos, &c.labels, &c.sizes}) HIP_OR_FAIL(e, b->ensure(words));
  HIP_OR_FAIL(e, d.out.ensure(sizeof(float) * 3 * (size_t)n));   // (never a reallocation when xyz is this buffer: its n points fit)
  HIP_OR_FAIL(e, d.out4.ensure(sizeof(float4) * (size_t)n));
  HIP_OR_FAIL(e, hipMemsetAsync(o.ctl.p, 0, sizeof(ClusterCtl), e->stream));
  ClusterCtl* ctl = o.ctl.as<ClusterCtl>();
  unsigned* flags = o.flags.as<unsigned>();
  const int blocks = (n + 255) / 256;
  outlier_finite_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, &ctl->o);
  HIP_OR_FAIL(e, hipGetLastError());
  if ((rc = ensure_sorted(e, d.cloud))) return rc;
  const float r = (float)tolerance;
  const float r2 = fminf(r * r, 1e37f);  // below the 2.7e37 of a slot past the end of the cloud, as for the radius filter
  {
    ProfScope ps(e, "cluster");
    cluster_init_kernel<<<blocks, 256, 0, e->stream>>>(n, c.parent.as<int>(), c.csize.as<int>(), c.cmin.as<int>());
    cluster_link_kernel<<<(n + 3) / 4, 256, 0, e->stream>>>(d.cloud.sorted.as<float4>(), d.cloud.bbox.as<float4>(), d.cloud.bbox2.as<float4>(), n, r2, c.parent.as<int>());
  }
  HIP_OR_FAIL(e, hipGetLastError());
  {
    ProfScope ps(e, "compact");
    cluster_flatten_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.sorted.as<float4>(), n, c.parent.as<int>(), c.root_in.as<int>(), c.csize.as<int>(), c.cmin.as<int>());
    cluster_flag_kernel<<<blocks, 256, 0, e->stream>>>(n, c.root_in.as<int>(), c.csize.as<int>(), c.cmin.as<int>(), min_size, max_size, flags, c.lead.as<unsigned>(), o.score.as<float>());
    HIP_OR_FAIL(e, hipGetLastError());
    const unsigned* total_dev = nullptr;  // (both scans leave their total in the same word of d.bsums: the label kernel reads the first before the second is queued)
    if ((rc = device_scan(e, d.bsums, c.lead.as<unsigned>(), n, c.lpos.as<unsigned>(), &total_dev))) return rc;
    cluster_label_kernel<<<blocks, 256, 0, e->stream>>>(n, c.root_in.as<int>(), c.csize.as<int>(), c.cmin.as<int>(), flags, c.lead.as<unsigned>(), c.lpos.as<unsigned>(), total_dev,
                                                        c.labels.as<int>(), c.sizes.as<int>(), ctl);
    HIP_OR_FAIL(e, hipGetLastError());
    if ((rc = device_scan(e, d.bsums, flags, n, o.pos.as<unsigned>(), &total_dev))) return rc;
    outlier_compact_kernel<<<blocks, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, flags, o.pos.as<unsigned>(), total_dev, d.out.as<float>(), d.out4.as<float4>(), o.kept.as<int>(), &ctl->o);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  ClusterCtl* h = reinterpret_cast<ClusterCtl*>(e->pinned);
  HIP_OR_FAIL(e, hipMemcpyAsync(h, ctl, sizeof(ClusterCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  if (h->o.bad) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: non-finite coordinates in the input");
  d.out_n = (int)h->o.count;
  d.out4_valid = d.out_n > 0;
  d.out_stream = e->stream;
  d.out_complete = true;
  c.num_clusters = (int)h->num_clusters;
  o.valid = true;
  o.cluster = true;
  *out_n = d.out_n;
  *num_clusters = c.num_clusters;
  return FVH_OK;
}

int cluster_get_labels(Engine* e, OutlierDev& o, ClusterDev& c, int* labels, int* sizes) {
  if (!o.valid || !o.cluster) return e->fail(FVH_ERR_BAD_STATE, "get_cluster_labels: the last call on this handle was not cluster_euclidean");
  bool queued = false;
  if (labels && o.n_in > 0) { HIP_OR_FAIL(e, hipMemcpyAsync(labels, c.labels.p, sizeof(int) * (size_t)o.n_in, hipMemcpyDefault, e->stream)); queued = true; }
  if (sizes && c.num_clusters > 0) { HIP_OR_FAIL(e, hipMemcpyAsync(sizes, c.sizes.p, sizeof(int) * (size_t)c.num_clusters, hipMemcpyDefault, e->stream)); queued = true; }
  if (queued) HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return FVH_OK;
}
