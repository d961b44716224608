// The stage layer under crop / outlier removal, deskew, clustering and plane segmentation on the voxel-grid filter's handle.
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_downsample.inc.hpp)
//
// A stage is one fvh_voxelgrid_* call that replaces the handle's output state (DownsampleDev::out / out4 / out_n), so get_points,
// device_points and fvh_ndt_*_from_voxelgrid work on its result like on a voxel filter's. This section holds what every stage does,
// once: which call the handle saw last (the only thing the getters ask), the checks on the cloud, and -- for the stages that keep a
// subset of their input (a MASK stage: crop, the two outlier filters, clustering, plane) -- the set-up in front of the stage's own
// kernels and the compaction, readback and publication behind them. A new mask stage writes: its argument checks, its own buffers,
// the kernels that fill o.flags (1 = keep) and o.score, and what it reads from its control block beyond the OutlierCtl prefix.

enum FilterLast { LAST_NONE, LAST_VOXEL, LAST_OUTLIER, LAST_DESKEW, LAST_CLUSTER, LAST_PLANE };

struct OutlierDev {
  DevBuf flags, pos, score, kept, ctl;  // keep flag and scanned position per input point, its score, kept indices, the stage's control block
  FilterLast last = LAST_NONE;          // the last call on the handle, if it succeeded: written by this section only, read by the getters
  int n_in = 0;
  double threshold = 0.0;
  bool has_kept() const { return last == LAST_OUTLIER || last == LAST_CLUSTER || last == LAST_PLANE; }  // kept indices and scores exist
  void release() { flags.release(); pos.release(); score.release(); kept.release(); ctl.release(); }
};

// Where every stage call begins: whatever it goes on to refuse, the old output and the old getters are gone.
inline void stage_begin(Engine* e, DownsampleDev& d, OutlierDev& o) {
  if (e->stream_owner) e->stream_owner->quiet = false;  // work on a borrowed stream (see downsample())
  o.last = LAST_NONE;
  d.out_n = 0;
  d.out4_valid = false;
}

// `have`: every array the call reads per point was given
inline int stage_check_cloud(Engine* e, const char* who, bool have, int n, int stride, const char* what = "points") {
  if (n < 0 || (n > 0 && !have)) return e->fail(FVH_ERR_INVALID_ARGUMENT, std::string(who) + ": null " + what);
  if (stride != 3 && stride != 4) return e->fail(FVH_ERR_INVALID_ARGUMENT, std::string(who) + ": stride must be 3 or 4 floats");
  return FVH_OK;
}

// Where a stage call succeeds (count = 0: the empty cloud, nothing was queued).
inline int stage_publish(Engine* e, DownsampleDev& d, OutlierDev& o, FilterLast kind, int count, int* out_n) {
  d.out_n = count;
  d.out4_valid = count > 0;
  d.out_stream = e->stream;
  d.out_complete = true;
  o.last = kind;
  *out_n = count;
  return FVH_OK;
}

// The voxel filter as a stage: downsample() itself knows nothing of the tag.
inline int voxel_stage(Engine* e, DownsampleDev& d, OutlierDev& o, int method, const float* xyz, int n, int stride, bool on_device, float leaf, int* out_n, bool early = false) {
  o.last = LAST_NONE;
  const int rc = downsample(e, d, method, xyz, n, stride, on_device, leaf, out_n, early);
  if (!rc) o.last = LAST_VOXEL;
  return rc;
}

// The input of a stage may be the handle's own output (chaining on one handle): it is widened into d.cloud FIRST, and everything
// that writes out / out4 is queued behind that kernel on the same stream.
inline int stage_upload(Engine* e, DownsampleDev& d, const float* xyz, int n, int stride, bool on_device) {
  const int rc = upload_cloud(e, d.cloud, xyz, n, stride, on_device, false);
  if (rc) return rc;
  HIP_OR_FAIL(e, d.out.ensure(sizeof(float) * 3 * (size_t)n));  // never a reallocation when xyz is this buffer: its n points fit
  HIP_OR_FAIL(e, d.out4.ensure(sizeof(float4) * (size_t)n));
  return FVH_OK;
}

// Set-up of a mask stage (n > 0): the cloud, the side outputs, a zeroed control block of ctl_bytes (it begins with an OutlierCtl),
// and with `finite` the kernel that reports a non-finite coordinate there (crop_range drops such points itself).
inline int mask_stage_setup(Engine* e, DownsampleDev& d, OutlierDev& o, const float* xyz, int n, int stride, bool on_device, size_t ctl_bytes, bool finite = true) {
  const int rc = stage_upload(e, d, xyz, n, stride, on_device);
  if (rc) return rc;
  const size_t words = sizeof(unsigned) * (size_t)n;
  HIP_OR_FAIL(e, o.flags.ensure(words));
  HIP_OR_FAIL(e, o.pos.ensure(words));
  HIP_OR_FAIL(e, o.score.ensure(words));
  HIP_OR_FAIL(e, o.kept.ensure(words));
  HIP_OR_FAIL(e, o.ctl.ensure(ctl_bytes));
  HIP_OR_FAIL(e, hipMemsetAsync(o.ctl.p, 0, ctl_bytes, e->stream));
  if (finite) {
    outlier_finite_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, o.ctl.as<OutlierCtl>());
    HIP_OR_FAIL(e, hipGetLastError());
  }
  return FVH_OK;
}

// Scan of o.flags and the compaction into out / out4 / o.kept. Opens no profile scope: the caller's "compact" scope covers it.
inline int mask_stage_compact(Engine* e, DownsampleDev& d, OutlierDev& o, int n) {
  const unsigned* total_dev = nullptr;
  const int rc = device_scan(e, d.bsums, o.flags.as<unsigned>(), n, o.pos.as<unsigned>(), &total_dev);
  if (rc) return rc;
  outlier_compact_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(d.cloud.pts.as<float4>(), n, o.flags.as<unsigned>(), o.pos.as<unsigned>(), total_dev, d.out.as<float>(),
                                                                 d.out4.as<float4>(), o.kept.as<int>(), o.ctl.as<OutlierCtl>());
  HIP_OR_FAIL(e, hipGetLastError());
  return FVH_OK;
}

// The one readback and the one synchronisation of a mask stage: the control block lands in the engine's pinned memory (where the
// stage reads what follows the OutlierCtl prefix, from the same copy), then the refusal or the publication.
inline int mask_stage_finish(Engine* e, DownsampleDev& d, OutlierDev& o, size_t ctl_bytes, const char* who, FilterLast kind, int* out_n) {
  HIP_OR_FAIL(e, hipMemcpyAsync(e->pinned, o.ctl.p, ctl_bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  const OutlierCtl* h = reinterpret_cast<const OutlierCtl*>(e->pinned);
  if (h->bad) return e->fail(FVH_ERR_INVALID_ARGUMENT, std::string(who) + ": non-finite coordinates in the input");
  return stage_publish(e, d, o, kind, (int)h->count, out_n);
}
