// Euclidean cluster extraction on the voxel-grid filter's handle (kernels_cluster.hpp; the contract is in include/fast_vgicp_hip.h).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_outlier.inc.hpp)
//
// A mask stage of host_filter_stage.inc.hpp: get_kept_indices and get_scores work on its result as after an outlier filter; labels
// and cluster sizes are its own (ClusterDev). One stream, one synchronisation, one readback (ClusterCtl).

struct ClusterDev {
  DevBuf parent, root_in, csize, cmin;  // union-find over sorted positions; per input point its root; per root the size and smallest input index
  DevBuf lead, lpos, labels, sizes;     // leader flags and their scan; the label per input point; the size per cluster
  int num_clusters = 0;
  void release() { parent.release(); root_in.release(); csize.release(); cmin.release(); lead.release(); lpos.release(); labels.release(); sizes.release(); }
};

int cluster_euclidean(Engine* e, DownsampleDev& d, OutlierDev& o, ClusterDev& c, const float* xyz, int n, int stride, bool on_device, double tolerance, int min_size, int max_size,
                      int* num_clusters, int* out_n) {
  stage_begin(e, d, o);
  c.num_clusters = 0;
  if (out_n) *out_n = 0;
  if (num_clusters) *num_clusters = 0;
  if (!out_n || !num_clusters) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: null out_n / num_clusters");
  int rc = stage_check_cloud(e, "cluster_euclidean", xyz != nullptr, n, stride);
  if (rc) return rc;
  if (!std::isfinite(tolerance) || !(tolerance > 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: tolerance must be finite and > 0");
  if (min_size < 1) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: min_cluster_size must be >= 1");
  if (max_size > 0 && max_size < min_size) return e->fail(FVH_ERR_INVALID_ARGUMENT, "cluster_euclidean: max_cluster_size must be <= 0 (no upper bound) or >= min_cluster_size");
  o.n_in = n;
  o.threshold = (double)min_size;
  if (n == 0) return stage_publish(e, d, o, LAST_CLUSTER, 0, out_n);
  for (DevBuf* b : {&c.parent, &c.root_in, &c.csize, &c.cmin, &c.lead, &c.lpos, &c.labels, &c.sizes}) HIP_OR_FAIL(e, b->ensure(sizeof(int) * (size_t)n));
  if ((rc = mask_stage_setup(e, d, o, xyz, n, stride, on_device, sizeof(ClusterCtl)))) return rc;
  ClusterCtl* ctl = o.ctl.as<ClusterCtl>();
  unsigned* flags = o.flags.as<unsigned>();
  const int blocks = (n + 255) / 256;
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
    if ((rc = mask_stage_compact(e, d, o, n))) return rc;
  }
  if ((rc = mask_stage_finish(e, d, o, sizeof(ClusterCtl), "cluster_euclidean", LAST_CLUSTER, out_n))) return rc;
  c.num_clusters = (int)reinterpret_cast<const ClusterCtl*>(e->pinned)->num_clusters;
  *num_clusters = c.num_clusters;
  return FVH_OK;
}

int cluster_get_labels(Engine* e, OutlierDev& o, ClusterDev& c, int* labels, int* sizes) {
  if (o.last != LAST_CLUSTER) return e->fail(FVH_ERR_BAD_STATE, "get_cluster_labels: the last call on this handle was not cluster_euclidean");
  bool queued = false;
  if (labels && o.n_in > 0) { HIP_OR_FAIL(e, hipMemcpyAsync(labels, c.labels.p, sizeof(int) * (size_t)o.n_in, hipMemcpyDefault, e->stream)); queued = true; }
  if (sizes && c.num_clusters > 0) { HIP_OR_FAIL(e, hipMemcpyAsync(sizes, c.sizes.p, sizeof(int) * (size_t)c.num_clusters, hipMemcpyDefault, e->stream)); queued = true; }
  if (queued) HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return FVH_OK;
}
