// Incremental target voxel map of a VGICP or NDT handle (fvh_vgicp_map_* / fvh_ndt_map_*): a map that keeps its per-voxel sums, takes posed
// scans in place and can be pruned. Kernels and buffer layout: kernels_voxelmap.hpp ("incremental target map"). VoxelMapDev::inc.mode picks
// the voxel type: 0 / 2 VGICP additive / multiplicative (points + covariances), 1 NDT (points only: sum p, sum p p^T).
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_stages.inc.hpp)
//
// The map lives in the handle's VoxelMapDev like a batch map -- keys[cur], table, occupied, counter set `cur`, bitmap / grid -- so
// everything that consumes a target map (launch_cost, the getters) reads it unchanged. The sums, stamps and the dirty list are its own
// (VoxelMapDev::inc); VoxelMapDev::acc and its clean / dirty bookkeeping stay build_voxelmap's.
// Everything is queued on the handle's main stream; the callers (CHECK_HANDLE) have ordered it after a pending side-stream build.
// Whether a map is live is the callers' question too (fvh_capi.hip: map_live, asked once in front of every call below but incmap_begin).

constexpr int INCMAP_DEFAULT_VOXELS = 16384;
constexpr unsigned INCMAP_MIN_CAPACITY = 64;
constexpr long long INCMAP_MAX_VOXELS = 1LL << 28;  // 4 x this is the largest table a 32-bit bucket index (bit 31: "new") addresses

inline unsigned incmap_capacity_for(long long voxels) {  // load factor <= 0.25 at `voxels`, as the batch build sizes its table
  unsigned cap = INCMAP_MIN_CAPACITY;
  while ((long long)cap < 4 * voxels) cap <<= 1;
  return cap;
}

// the kernel instantiation of the live map's voxel type: f(std::integral_constant<int, 0 additive | 1 NDT sums | 2 multiplicative>{})
template <class F>
inline void incmap_by_mode(const VoxelMapDev& vm, F&& f) {
  if (vm.inc.mode == 2) f(std::integral_constant<int, 2>{});
  else if (vm.inc.mode == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{});
}

// buffers of side `which` at `cap` buckets, empty: keys EMPTY, sums / stamps 0
int incmap_prepare_side(Engine* e, VoxelMapDev& vm, int which, unsigned cap) {
  HIP_OR_FAIL(e, vm.keys[which].ensure((size_t)cap * 8));
  HIP_OR_FAIL(e, vm.inc.sums[which].ensure((size_t)cap * VM_ACC_STRIDE * sizeof(double)));
  HIP_OR_FAIL(e, vm.inc.stamps[which].ensure((size_t)cap * sizeof(unsigned)));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.keys[which].p, 0xFF, (size_t)cap * 8, e->stream));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.sums[which].p, 0, (size_t)cap * VM_ACC_STRIDE * sizeof(double), e->stream));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.stamps[which].p, 0, (size_t)cap * sizeof(unsigned), e->stream));
  vm.clean_cap = 0;  // (build_voxelmap's note on keys[cur ^ 1]: no longer true once this map has used either side)
  return FVH_OK;
}

int incmap_begin(Engine* e, VoxelMapDev& vm, double res, int mode, int expected_voxels) {
  if (!(res > 0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "map_begin: resolution must be > 0");
  const long long want = expected_voxels > 0 ? expected_voxels : INCMAP_DEFAULT_VOXELS;
  if (want > INCMAP_MAX_VOXELS) return e->fail(FVH_ERR_INVALID_ARGUMENT, "map_begin: expected_voxels too large");
  const unsigned cap = incmap_capacity_for(want);
  vm.invalidate();
  vm.inc.live = false;
  vm.res = res;
  vm.capacity = cap;
  HIP_OR_FAIL(e, vm.table.ensure((size_t)cap * 64));
  HIP_OR_FAIL(e, vm.occupied.ensure(sizeof(int) * (size_t)cap));
  HIP_OR_FAIL(e, vm.counters.ensure(2 * 16 * sizeof(int)));
  HIP_OR_FAIL(e, vm.inc.ctl.ensure(4 * sizeof(int)));
  { int rc = incmap_prepare_side(e, vm, vm.cur, cap); if (rc) return rc; }
  HIP_OR_FAIL(e, hipMemsetAsync(vm.counters.p, 0, 2 * 16 * sizeof(int), e->stream));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.ctl.p, 0, 4 * sizeof(int), e->stream));
  vm.inc.mode = mode == 2 ? 2 : (mode == 1 ? 1 : 0);  // (VGICP's ADDITIVE_WEIGHTED never reaches here as 1: fvh_vgicp::map_begin_mode folds it into 0)
  vm.inc.epoch = 0;
  vm.inc.num_points = 0;
  vm.inc.voxel_bound = 0;
  vm.inc.live = true;
  vm.valid = true;
  vm.nv_hint = -1;
  e->has_corr = false;
  return FVH_OK;
}

// occupancy bitmap of a large map, rebuilt from the compact list (the five launches of build_voxelmap)
int incmap_bitmap(Engine* e, VoxelMapDev& vm) {
  vm.has_bitmap = false;
  const size_t bitmap_bytes = (size_t)e->params.bitmap_max_bytes;
  if (vm.inc.num_points < (long long)e->params.bitmap_min_points || bitmap_bytes < 8) return FVH_OK;
  HIP_OR_FAIL(e, vm.bitmap.ensure(bitmap_bytes));
  HIP_OR_FAIL(e, vm.grid.ensure(sizeof(VmGrid)));
  VmGrid* g = vm.grid.as<VmGrid>();
  hipStream_t st = e->stream;
  unsigned long long* keys = vm.keys[vm.cur].as<unsigned long long>();
  vm_grid_init_kernel<<<1, 64, 0, st>>>(g);
  vm_grid_bounds_kernel<<<64, 256, 0, st>>>(keys, vm.occupied.as<int>(), vm.counters_cur(), g);
  vm_grid_setup_kernel<<<1, 64, 0, st>>>(g, (unsigned long long)(bitmap_bytes / 8));
  vm_grid_clear_kernel<<<512, 256, 0, st>>>(vm.bitmap.as<unsigned long long>(), g);
  vm_grid_set_kernel<<<256, 256, 0, st>>>(keys, vm.occupied.as<int>(), vm.counters_cur(), g, vm.bitmap.as<unsigned long long>());
  HIP_OR_FAIL(e, hipGetLastError());
  vm.has_bitmap = true;
  return FVH_OK;
}

// move the map into the other buffers at `new_cap` buckets, dropping what `prune` names: growth and pruning
int incmap_rehash(Engine* e, VoxelMapDev& vm, unsigned new_cap, const VmPrune& prune) {
  const int from = vm.cur, to = vm.cur ^ 1;
  const unsigned old_cap = vm.capacity;
  ProfScope ps(e, "map_rehash");  // (the clears of the other side included)
  { int rc = incmap_prepare_side(e, vm, to, new_cap); if (rc) return rc; }
  // the records are recomputed from the moved sums and the compact list is rebuilt: the old contents of both may go with a reallocation
  HIP_OR_FAIL(e, vm.table.ensure((size_t)new_cap * 64));
  HIP_OR_FAIL(e, vm.occupied.ensure(sizeof(int) * (size_t)new_cap));
  int* next_counters = vm.counters.as<int>() + 16 * to;
  vm_rehash_begin_kernel<<<1, 64, 0, e->stream>>>(vm.counters_cur(), next_counters, vm.inc.ctl.as<int>());
  const unsigned blocks = (old_cap + VM_FIN_THREADS - 1) / VM_FIN_THREADS;
  incmap_by_mode(vm, [&](auto m) {
    vm_rehash_kernel<decltype(m)::value><<<blocks, VM_FIN_THREADS, 0, e->stream>>>(vm.keys[from].as<unsigned long long>(), vm.inc.sums[from].as<double>(), vm.inc.stamps[from].as<unsigned>(), old_cap,
                                                                                   vm.keys[to].as<unsigned long long>(), new_cap - 1, vm.inc.sums[to].as<double>(), vm.inc.stamps[to].as<unsigned>(),
                                                                                   vm.table.as<uint4>(), next_counters, vm.occupied.as<int>(), prune, vm.inc.ctl.as<int>());
  });
  HIP_OR_FAIL(e, hipGetLastError());
  vm.cur = to;
  vm.capacity = new_cap;
  vm.host_valid = false;
  vm.has_canon = false;
  e->has_corr = false;  // stored correspondences are bucket indices of the old table
  return incmap_bitmap(e, vm);
}

inline VmPrune incmap_no_prune(const VoxelMapDev& vm) {
  VmPrune p;
  std::memset(&p, 0, sizeof(p));
  p.res = vm.res;
  p.epoch = vm.inc.epoch;
  return p;
}

int incmap_read_counts(Engine* e, VoxelMapDev& vm, int* counters3, int* ctl4) {
  if (counters3) HIP_OR_FAIL(e, hipMemcpyAsync(counters3, vm.counters_cur(), 3 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (ctl4) HIP_OR_FAIL(e, hipMemcpyAsync(ctl4, vm.inc.ctl.p, 4 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return FVH_OK;
}

// add cloud `c` (points + covariances) at pose T. Capacity is secured BEFORE the launch from a host-side upper bound of the voxel
// count (every point could open a voxel): an insert can neither drop a point nor need to be redone.
int incmap_insert(Engine* e, VoxelMapDev& vm, const CloudDev& c, const double* T16, const char* who) {
  if (vm.inc.mode == 1 ? !c.has_pts : (!c.has_pts || !c.has_cov)) return e->fail(FVH_ERR_BAD_STATE, std::string(who) + (vm.inc.mode == 1 ? ": the cloud is not set" : ": the cloud needs points and covariances"));
  if (!T16) return e->fail(FVH_ERR_INVALID_ARGUMENT, std::string(who) + ": null pose");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T16[i])) return e->fail(FVH_ERR_INVALID_ARGUMENT, std::string(who) + ": the pose is not finite");
  const int n = c.n;
  if (vm.inc.voxel_bound + (long long)n > INCMAP_MAX_VOXELS) {
    int cnt[3];
    { int rc = incmap_read_counts(e, vm, cnt, nullptr); if (rc) return rc; }
    vm.inc.voxel_bound = cnt[0];
    if (vm.inc.voxel_bound + (long long)n > INCMAP_MAX_VOXELS) return e->fail(FVH_ERR_UNSUPPORTED, std::string(who) + ": the map would exceed 2^28 voxels");
  }
  if (2 * (vm.inc.voxel_bound + (long long)n) > (long long)vm.capacity) {
    // the bound says the table could pass a load factor of 0.5: look at the real voxel count (one readback, only here), then grow if it is true
    int cnt[3];
    { int rc = incmap_read_counts(e, vm, cnt, nullptr); if (rc) return rc; }
    vm.inc.voxel_bound = cnt[0];
    if (2 * (vm.inc.voxel_bound + (long long)n) > (long long)vm.capacity) {
      int rc = incmap_rehash(e, vm, incmap_capacity_for(vm.inc.voxel_bound + (long long)n), incmap_no_prune(vm));
      if (rc) return rc;
    }
  }
  vm.inc.epoch++;
  vm.inc.num_points += n;
  vm.host_valid = false;
  vm.has_canon = false;
  e->has_corr = false;
  if (n == 0) return FVH_OK;
  HIP_OR_FAIL(e, vm.inc.dirty.ensure(sizeof(unsigned) * (size_t)n));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.ctl.p, 0, sizeof(int), e->stream));  // the dirty count
  const PoseD T = pose_from_colmajor16(T16);
  unsigned long long* keys = vm.keys[vm.cur].as<unsigned long long>();
  double* sums = vm.inc.sums[vm.cur].as<double>();
  unsigned* stamps = vm.inc.stamps[vm.cur].as<unsigned>();
  int* counters = vm.counters_cur();
  int* ctl = vm.inc.ctl.as<int>();
  unsigned* dirty = vm.inc.dirty.as<unsigned>();
  const int* order = coherent_order(c, e->params.coherent_min_points);
  VmGrid* grid = vm.has_bitmap ? vm.grid.as<VmGrid>() : nullptr;
  unsigned long long* bitmap = vm.has_bitmap ? vm.bitmap.as<unsigned long long>() : nullptr;
  const int blocks = (n + 255) / 256;
  {
    ProfScope ps(e, "map_insert");
    incmap_by_mode(vm, [&](auto m) {
      constexpr int M = decltype(m)::value;
      vm_insert_kernel<M><<<blocks, 256, 0, e->stream>>>(c.pts.as<float4>(), M == 1 ? nullptr : c.cov.as<float4>(), n, T, vm.res, keys, vm.capacity - 1, sums, stamps, vm.inc.epoch, dirty, ctl, counters + 1, order);
      vm_refresh_kernel<M><<<blocks, 256, 0, e->stream>>>(dirty, ctl, keys, sums, vm.table.as<uint4>(), counters, vm.occupied.as<int>(), grid, bitmap);
    });
  }
  HIP_OR_FAIL(e, hipGetLastError());
  vm.inc.voxel_bound += n;
  // a map that has grown into bitmap territory gets its bitmap here (once: later inserts set bits, or switch it off on the device when a
  // voxel falls outside its box -- the next rehash rebuilds it)
  if (!vm.has_bitmap) return incmap_bitmap(e, vm);
  return FVH_OK;
}

int incmap_prune(Engine* e, VoxelMapDev& vm, const double* center3, double radius, int max_age, int* num_removed) {
  VmPrune p = incmap_no_prune(vm);
  if (center3) {
    if (!std::isfinite(center3[0]) || !std::isfinite(center3[1]) || !std::isfinite(center3[2]) || !(radius >= 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "map_prune: centre must be finite and radius >= 0");
    p.by_distance = 1;
    p.center[0] = center3[0]; p.center[1] = center3[1]; p.center[2] = center3[2];
    p.radius = radius;
  }
  p.max_age = max_age > 0 ? (unsigned)max_age : 0u;
  if (num_removed) *num_removed = 0;
  if (!p.by_distance && !p.max_age) return FVH_OK;
  { int rc = incmap_rehash(e, vm, vm.capacity, p); if (rc) return rc; }
  int cnt[3], ctl[4];
  { int rc = incmap_read_counts(e, vm, cnt, ctl); if (rc) return rc; }
  vm.inc.voxel_bound = cnt[0];
  if (num_removed) *num_removed = ctl[2];
  return FVH_OK;
}

// ---- free space cleared along the rays of a posed scan (fvh_*_clear_rays_*; kernels_voxelmap.hpp: "free space cleared") -------------
// o' = (float)(R o + t): ((r0 x + r1 y) + r2 z) + t per axis in fp64 with no product contracted into a sum, rounded once
inline float clear_rays_origin_axis(const double* r3, const double* o, double t) {
#pragma clang fp contract(off)
  return (float)(((r3[0] * o[0] + r3[1] * o[1]) + r3[2] * o[2]) + t);
}
// what the host refuses before anything is queued (the cloud's own arguments -- n, xyz, stride -- are the caller's)
int incmap_clear_rays_check(Engine* e, const VoxelMapDev& vm, const double* T16, const double* origin3, double min_range, double max_range, double end_margin, int min_misses, const char* who) {
  const std::string w(who);
  if (!T16) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": null pose");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T16[i])) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": the pose is not finite");
  if (origin3 && !(std::isfinite(origin3[0]) && std::isfinite(origin3[1]) && std::isfinite(origin3[2]))) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": the origin is not finite");
  if (!(min_range >= 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": min_range must be >= 0");
  if (!std::isfinite(max_range) || max_range < min_range) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": max_range must be finite and >= min_range");
  if (max_range / vm.res > 4096.0) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": max_range is more than 4096 voxels (a lane would walk more than 12,291 cells)");
  if (!std::isfinite(end_margin) || end_margin < 0.0) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": end_margin must be finite and >= 0");
  if (min_misses < 1) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": min_misses must be >= 1");
  return FVH_OK;
}

// the rays origin3 -> point of cloud `c` (points only), both at pose T16: mark, sweep, one readback, and -- only if a voxel was condemned -- the
// rehash at the same capacity. Arguments checked by incmap_clear_rays_check.
int incmap_clear_rays(Engine* e, VoxelMapDev& vm, const CloudDev& c, const int* order, const double* T16, const double* origin3, double min_range, double max_range, double end_margin,
                      int min_misses, int* num_removed, int* rays_used) {
  if (num_removed) *num_removed = 0;
  if (rays_used) *rays_used = 0;
  const int n = c.n;
  if (n == 0) return FVH_OK;
  VmRays ry;
  ry.T = pose_from_colmajor16(T16);
  const double zero3[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 3; a++) ry.origin[a] = clear_rays_origin_axis(ry.T.r + 3 * a, origin3 ? origin3 : zero3, ry.T.t[a]);
  ry.res = vm.res; ry.min_range = min_range; ry.max_range = max_range; ry.end_margin = end_margin;
  // The sweep marks a condemned bucket by writing its stamp, and only the rehash removes it: nothing between the two may fail. The buffers
  // the rehash moves the map into are therefore secured here, before anything is written (same capacity: table and list are large enough).
  const int to = vm.cur ^ 1;
  HIP_OR_FAIL(e, vm.keys[to].ensure((size_t)vm.capacity * 8));
  HIP_OR_FAIL(e, vm.inc.sums[to].ensure((size_t)vm.capacity * VM_ACC_STRIDE * sizeof(double)));
  HIP_OR_FAIL(e, vm.inc.stamps[to].ensure((size_t)vm.capacity * sizeof(unsigned)));
  HIP_OR_FAIL(e, vm.inc.ray_marks.ensure((size_t)vm.capacity * sizeof(unsigned)));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.ray_marks.p, 0, (size_t)vm.capacity * sizeof(unsigned), e->stream));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.ctl.p, 0, 4 * sizeof(int), e->stream));
  const int n_bound = (int)std::min<long long>(vm.inc.voxel_bound, (long long)vm.capacity);  // (the host keeps the load factor <= 0.5: capacity bounds the count too)
  {
    ProfScope ps(e, "map_raymark");
    vm_raymark_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(c.pts.as<float4>(), n, order, ry, vm.keys_cur(), vm.capacity - 1, vm.inc.ray_marks.as<unsigned>(),
                                                              vm.has_bitmap ? vm.grid.as<VmGrid>() : nullptr, vm.has_bitmap ? vm.bitmap.as<unsigned long long>() : nullptr, vm.inc.ctl.as<int>());
  }
  if (n_bound > 0) {
    ProfScope ps(e, "map_raysweep");
    vm_raysweep_kernel<<<(n_bound + 255) / 256, 256, 0, e->stream>>>(vm.occupied.as<int>(), vm.counters_cur(), n_bound, vm.inc.ray_marks.as<unsigned>(), (unsigned)min_misses,
                                                                     vm.inc.stamps[vm.cur].as<unsigned>(), vm.inc.ctl.as<int>());
  }
  HIP_OR_FAIL(e, hipGetLastError());
  int cnt[3], ctl[4];
  { int rc = incmap_read_counts(e, vm, cnt, ctl); if (rc) return rc; }
  vm.inc.voxel_bound = cnt[0];
  if (rays_used) *rays_used = ctl[1];
  const int removed = ctl[3];
  if (removed > 0) {
    VmPrune p = incmap_no_prune(vm);
    p.max_age = vm.inc.epoch;  // epoch - stamp >= epoch: exactly the buckets whose stamp the sweep set to 0
    { int rc = incmap_rehash(e, vm, vm.capacity, p); if (rc) return rc; }
    vm.inc.voxel_bound = cnt[0] - removed;
  }
  if (num_removed) *num_removed = removed;
  return FVH_OK;
}

// ---- a posed scan scored against the target voxel map, per point (fvh_*_score_source / _score_cloud; kernels_mapscore.hpp) -----------------
static_assert(sizeof(fvh_map_score) == sizeof(VmScoreOut) && offsetof(fvh_map_score, n_explained) == offsetof(VmScoreOut, n_explained) &&
              offsetof(fvh_map_score, sum_best_m2) == offsetof(VmScoreOut, sum_best_m2) && offsetof(fvh_map_score, sum_score_all) == offsetof(VmScoreOut, sum_score_all),
              "VmScoreOut is the device image of fvh_map_score");
// what the host refuses before anything is queued (the cloud's own arguments -- n, xyz, stride -- are the caller's)
int map_score_check(Engine* e, const double* T16, int neighbors, double max_m2, double score_scale, const fvh_map_score* out, const char* who) {
  const std::string w(who);
  if (!T16) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": null pose");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T16[i])) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": the pose is not finite");
  if (!out) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": null result");
  if (neighbors != FVH_DIRECT1 && neighbors != FVH_DIRECT7 && neighbors != FVH_DIRECT27) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": neighbors must be FVH_DIRECT1, FVH_DIRECT7 or FVH_DIRECT27");
  if (!(max_m2 >= 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": max_m2 must be >= 0");
  if (!std::isfinite(score_scale) || !(score_scale > 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": score_scale must be finite and > 0");
  return FVH_OK;
}

// n points at d_xyz (device, `stride` floats apart; `order`: the walk order or null) at pose T16 against `vm`: the score kernel, the two-level
// fixed-order sum, ONE readback of the struct (+ the per-point rows that were asked for). Nothing of the engine or the map is written; the
// scratch is the map's own. Arguments checked by map_score_check. *overflowed: the map's table had dropped points (a hint-sized batch build):
// `out` is then not valid, the caller rebuilds the map and calls again.
int map_score_run(Engine* e, VoxelMapDev& vm, const float* d_xyz, int stride, int n, const int* order, const double* T16, int neighbors, int min_points, double max_m2, double score_scale,
              fvh_map_score* out, int* found, int* best, double* best_m2, bool* overflowed) {
  *overflowed = false;
  std::memset(out, 0, sizeof(*out));
  if (n == 0) return FVH_OK;
  const int nb = (n + VM_SCORE_CHUNK - 1) / VM_SCORE_CHUNK;
  // {VmScoreOut (64 B) | 3 nb chunk sums | 3 n terms | n best m2 | n found | n best}
  const size_t off_chunk = 64, off_terms = off_chunk + sizeof(double) * 3 * (size_t)nb, off_m2 = off_terms + sizeof(double) * 3 * (size_t)n, off_found = off_m2 + sizeof(double) * (size_t)n,
               off_best = off_found + sizeof(int) * (size_t)n;
  HIP_OR_FAIL(e, vm.score_buf.ensure(off_best + sizeof(int) * (size_t)n));
  char* base = vm.score_buf.as<char>();
  VmScoreOut* d_out = reinterpret_cast<VmScoreOut*>(base);
  double* d_chunk = reinterpret_cast<double*>(base + off_chunk);
  double* d_terms = reinterpret_cast<double*>(base + off_terms);
  double* d_m2 = best_m2 ? reinterpret_cast<double*>(base + off_m2) : nullptr;
  int* d_found = found ? reinterpret_cast<int*>(base + off_found) : nullptr;
  int* d_best = best ? reinterpret_cast<int*>(base + off_best) : nullptr;
  HIP_OR_FAIL(e, hipMemsetAsync(d_out, 0, sizeof(VmScoreOut), e->stream));
  VmScore sp;
  sp.T = pose_from_colmajor16(T16);
  sp.res = vm.res; sp.max_m2 = max_m2; sp.score_scale = score_scale; sp.min_points = min_points;
  const VmGrid* grid = vm.has_bitmap ? vm.grid.as<VmGrid>() : nullptr;
  const unsigned long long* bitmap = vm.has_bitmap ? vm.bitmap.as<unsigned long long>() : nullptr;
  {
    ProfScope ps(e, "map_score");
    auto launch = [&](auto noff) {
      vm_score_kernel<decltype(noff)::value><<<(n + 255) / 256, 256, 0, e->stream>>>(d_xyz, stride, n, order, sp, vm.keys_cur(), vm.capacity - 1, vm.table.as<uint4>(), grid, bitmap, vm.counters_cur(),
                                                                                    d_terms, d_found, d_best, d_m2, d_out);
    };
    if (neighbors == FVH_DIRECT1) launch(std::integral_constant<int, 1>{});
    else if (neighbors == FVH_DIRECT7) launch(std::integral_constant<int, 7>{});
    else launch(std::integral_constant<int, 27>{});
    // chunk sums, then their sum: one chunk goes straight into the struct (how many levels run depends on n alone)
    vm_score_sum_kernel<3><<<nb, 1024, 0, e->stream>>>(d_terms, n, VM_SCORE_CHUNK, nb == 1 ? &d_out->sum_best_m2 : d_chunk);
    if (nb > 1) vm_score_sum_kernel<3><<<1, 1024, 0, e->stream>>>(d_chunk, nb, 0x7FFFFFFF, &d_out->sum_best_m2);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  HIP_OR_FAIL(e, hipMemcpyAsync(out, d_out, sizeof(*out), hipMemcpyDeviceToHost, e->stream));
  if (found) HIP_OR_FAIL(e, hipMemcpyAsync(found, d_found, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (best) HIP_OR_FAIL(e, hipMemcpyAsync(best, d_best, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (best_m2) HIP_OR_FAIL(e, hipMemcpyAsync(best_m2, d_m2, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  if (out->n_points < 0) { *overflowed = true; std::memset(out, 0, sizeof(*out)); }
  return FVH_OK;
}

// ---- rays cast into the target voxel map: the first hit per ray (fvh_*_cast_rays_source / _cast_rays_cloud; kernels_raycast.hpp) ----------
static_assert(sizeof(fvh_ray_cast) == sizeof(VmCastOut) && offsetof(fvh_ray_cast, n_hit_at_origin) == offsetof(VmCastOut, n_hit_at_origin) &&
              offsetof(fvh_ray_cast, n_cells) == offsetof(VmCastOut, n_cells) && sizeof(long long) == 8,
              "VmCastOut is the device image of fvh_ray_cast");
// what the host refuses before anything is queued (the cloud's own arguments -- n, xyz, stride -- are the caller's)
int map_cast_check(Engine* e, const VoxelMapDev& vm, const double* T16, const double* origin3, double min_range, double max_range, double max_m2, const fvh_ray_cast* out, const char* who) {
  const std::string w(who);
  if (!T16) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": null pose");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T16[i])) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": the pose is not finite");
  if (origin3 && !(std::isfinite(origin3[0]) && std::isfinite(origin3[1]) && std::isfinite(origin3[2]))) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": the origin is not finite");
  if (!out) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": null result");
  if (!(min_range >= 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": min_range must be >= 0");
  if (!std::isfinite(max_range) || max_range < min_range) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": max_range must be finite and >= min_range");
  if (max_range / vm.res > 4096.0) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": max_range is more than 4096 voxels (a lane would walk more than 12,291 cells)");
  if (!(max_m2 >= 0.0)) return e->fail(FVH_ERR_INVALID_ARGUMENT, w + ": max_m2 must be >= 0");
  return FVH_OK;
}

// n segments origin3 -> d_xyz[i] (device, `stride` floats apart; `order`: the walk order or null), both at pose T16, against `vm`: the cast
// kernel and ONE readback of the struct (+ the per-ray rows that were asked for). Nothing of the engine or the map is written; the scratch is
// the map's own. Arguments checked by map_cast_check. *overflowed: the map's table had dropped points (a hint-sized batch build): `out` is
// then not valid, the caller rebuilds the map and calls again.
int map_cast_run(Engine* e, VoxelMapDev& vm, const float* d_xyz, int stride, int n, const int* order, const double* T16, const double* origin3, double min_range, double max_range,
                 int min_points, double max_m2, fvh_ray_cast* out, int* hit, int* cell3, double* range, double* m2, bool* overflowed) {
  *overflowed = false;
  std::memset(out, 0, sizeof(*out));
  if (n == 0) return FVH_OK;
  // {VmCastOut (64 B) | n ranges | n m2 | n hit | 3 n cell}
  const size_t off_range = 64, off_m2 = off_range + sizeof(double) * (size_t)n, off_hit = off_m2 + sizeof(double) * (size_t)n, off_cell = off_hit + sizeof(int) * (size_t)n;
  HIP_OR_FAIL(e, vm.cast_buf.ensure(off_cell + sizeof(int) * 3 * (size_t)n));
  char* base = vm.cast_buf.as<char>();
  VmCastOut* d_out = reinterpret_cast<VmCastOut*>(base);
  double* d_range = range ? reinterpret_cast<double*>(base + off_range) : nullptr;
  double* d_m2 = m2 ? reinterpret_cast<double*>(base + off_m2) : nullptr;
  int* d_hit = hit ? reinterpret_cast<int*>(base + off_hit) : nullptr;
  int* d_cell = cell3 ? reinterpret_cast<int*>(base + off_cell) : nullptr;
  HIP_OR_FAIL(e, hipMemsetAsync(d_out, 0, sizeof(VmCastOut), e->stream));
  VmCast cp;
  cp.T = pose_from_colmajor16(T16);
  const double zero3[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 3; a++) cp.origin[a] = clear_rays_origin_axis(cp.T.r + 3 * a, origin3 ? origin3 : zero3, cp.T.t[a]);
  cp.res = vm.res; cp.min_range = min_range; cp.max_range = max_range; cp.max_m2 = max_m2; cp.min_points = min_points;
  {
    ProfScope ps(e, "map_raycast");
    vm_raycast_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(d_xyz, stride, n, order, cp, vm.keys_cur(), vm.capacity - 1, vm.table.as<uint4>(), vm.has_bitmap ? vm.grid.as<VmGrid>() : nullptr,
                                                              vm.has_bitmap ? vm.bitmap.as<unsigned long long>() : nullptr, vm.counters_cur(), d_hit, d_cell, d_range, d_m2, d_out);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  HIP_OR_FAIL(e, hipMemcpyAsync(out, d_out, sizeof(*out), hipMemcpyDeviceToHost, e->stream));
  if (hit) HIP_OR_FAIL(e, hipMemcpyAsync(hit, d_hit, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (cell3) HIP_OR_FAIL(e, hipMemcpyAsync(cell3, d_cell, sizeof(int) * 3 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (range) HIP_OR_FAIL(e, hipMemcpyAsync(range, d_range, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (m2) HIP_OR_FAIL(e, hipMemcpyAsync(m2, d_m2, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  if (out->n_rays < 0) { *overflowed = true; std::memset(out, 0, sizeof(*out)); }
  return FVH_OK;
}

// ---- snapshots of the live map (fvh_vgicp_voxelmap_export / _import / _merge_from; kernels_voxelmap.hpp: "snapshots") ------------------
// A snapshot is the header {resolution, mode, num_inserts = epoch, num_points, num_voxels} and per voxel {coords[3], sums[10], age}, rows
// in ascending packed-key order. Rows ADD into a live map of the same grid: import (host rows) and merge_from (another handle's map, read
// in place) are one kernel + the insert's refresh.

// `mode` of a snapshot header: the VGICP accumulation mode (0 additive, 2 multiplicative), or FVH_VOXEL_NDT_SUMS for an NDT map -- whose
// sums (sum p, sum p p^T) must never add into VGICP voxels (sum p, sum C) or the other way round: import compares this value
inline int incmap_snapshot_mode(const VoxelMapDev& vm) { return vm.inc.mode == 1 ? (int)FVH_VOXEL_NDT_SUMS : vm.inc.mode; }

inline unsigned long long host_pack_key(int x, int y, int z) {
  return (unsigned long long)(unsigned)(x + FVH_COORD_BIAS) | ((unsigned long long)(unsigned)(y + FVH_COORD_BIAS) << 21) | ((unsigned long long)(unsigned)(z + FVH_COORD_BIAS) << 42);
}

// room for `n` more voxels, secured BEFORE a launch as incmap_insert does it: host bound + n, a readback only when the bound asks for one,
// growth by a rehash. Queues nothing that changes what the map holds.
int incmap_secure(Engine* e, VoxelMapDev& vm, long long n, const char* who) {
  if (vm.inc.voxel_bound + n > INCMAP_MAX_VOXELS || 2 * (vm.inc.voxel_bound + n) > (long long)vm.capacity) {
    int cnt[3];
    { int rc = incmap_read_counts(e, vm, cnt, nullptr); if (rc) return rc; }
    vm.inc.voxel_bound = cnt[0];
    if (vm.inc.voxel_bound + n > INCMAP_MAX_VOXELS) return e->fail(FVH_ERR_UNSUPPORTED, std::string(who) + ": the map would exceed 2^28 voxels");
    if (2 * (vm.inc.voxel_bound + n) > (long long)vm.capacity) {
      int rc = incmap_rehash(e, vm, incmap_capacity_for(vm.inc.voxel_bound + n), incmap_no_prune(vm));
      if (rc) return rc;
    }
  }
  return FVH_OK;
}

int incmap_export(Engine* e, VoxelMapDev& vm, int* num_voxels, double* resolution, int* mode, int* num_inserts, long long* num_points, int* coords3, double* sums10, unsigned* ages) {
  const bool rows = coords3 || sums10 || ages;
  if (rows && !(coords3 && sums10 && ages)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_export: coords3, sums10 and ages go together (all NULL: the header only)");
  int cnt[3];
  { int rc = incmap_read_counts(e, vm, cnt, nullptr); if (rc) return rc; }
  vm.inc.voxel_bound = cnt[0];
  const int n = cnt[0];
  if (num_voxels) *num_voxels = n;
  if (resolution) *resolution = vm.res;
  if (mode) *mode = incmap_snapshot_mode(vm);
  if (num_inserts) *num_inserts = (int)vm.inc.epoch;
  if (num_points) *num_points = vm.inc.num_points;
  if (!rows || n == 0) return FVH_OK;
  const size_t sums_bytes = sizeof(double) * VM_ACC_STRIDE * (size_t)n, coords_bytes = sizeof(int) * 3 * (size_t)n, ages_bytes = sizeof(unsigned) * (size_t)n;
  HIP_OR_FAIL(e, vm.inc.xfer.ensure(sums_bytes + coords_bytes + ages_bytes));
  double* d_sums = vm.inc.xfer.as<double>();
  int* d_coords = reinterpret_cast<int*>(static_cast<char*>(vm.inc.xfer.p) + sums_bytes);
  unsigned* d_ages = reinterpret_cast<unsigned*>(static_cast<char*>(vm.inc.xfer.p) + sums_bytes + coords_bytes);
  {
    ProfScope ps(e, "map_export");
    vm_export_kernel<<<(n + VM_SNAP_THREADS - 1) / VM_SNAP_THREADS, VM_SNAP_THREADS, 0, e->stream>>>(vm.keys_cur(), vm.inc.sums[vm.cur].as<double>(), vm.inc.stamps[vm.cur].as<unsigned>(), vm.occupied.as<int>(),
                                                                                                      vm.counters_cur(), vm.inc.epoch, n, d_coords, d_sums, d_ages);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  // the rows arrive in the order of the compact list; the contract's order -- ascending packed key -- is made here, on the host
  std::vector<double> h_sums((size_t)n * VM_ACC_STRIDE);
  std::vector<int> h_coords((size_t)n * 3);
  std::vector<unsigned> h_ages((size_t)n);
  {
    ProfScope ps(e, "map_export_copy");
    HIP_OR_FAIL(e, hipMemcpyAsync(h_sums.data(), d_sums, sums_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_OR_FAIL(e, hipMemcpyAsync(h_coords.data(), d_coords, coords_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_OR_FAIL(e, hipMemcpyAsync(h_ages.data(), d_ages, ages_bytes, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  std::vector<std::pair<unsigned long long, int>> order((size_t)n);
  for (int i = 0; i < n; i++) order[i] = {host_pack_key(h_coords[3 * (size_t)i], h_coords[3 * (size_t)i + 1], h_coords[3 * (size_t)i + 2]), i};
  std::sort(order.begin(), order.end());
  for (int r = 0; r < n; r++) {
    const size_t i = (size_t)order[r].second;
    std::memcpy(coords3 + 3 * (size_t)r, &h_coords[3 * i], 3 * sizeof(int));
    std::memcpy(sums10 + VM_ACC_STRIDE * (size_t)r, &h_sums[VM_ACC_STRIDE * i], VM_ACC_STRIDE * sizeof(double));
    ages[r] = h_ages[i];
  }
  return FVH_OK;
}

// what import and merge_from share once the rows are on the device: the new epoch, the launch, the insert's refresh and bookkeeping
template <bool FROM_MAP>
int incmap_add_rows(Engine* e, VoxelMapDev& vm, int n_rows, const int* d_coords, const double* d_sums, const unsigned* d_ages, const VoxelMapDev* from, unsigned in_epoch, long long in_points,
                    const char* prof_class) {
  vm.inc.epoch = std::max(vm.inc.epoch, in_epoch);
  vm.inc.num_points += in_points;
  vm.host_valid = false;
  vm.has_canon = false;
  e->has_corr = false;
  if (n_rows == 0) return FVH_OK;
  HIP_OR_FAIL(e, vm.inc.dirty.ensure(sizeof(unsigned) * (size_t)n_rows));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.ctl.p, 0, sizeof(int), e->stream));  // the dirty count
  unsigned long long* keys = vm.keys[vm.cur].as<unsigned long long>();
  double* sums = vm.inc.sums[vm.cur].as<double>();
  unsigned* stamps = vm.inc.stamps[vm.cur].as<unsigned>();
  int* counters = vm.counters_cur();
  int* ctl = vm.inc.ctl.as<int>();
  unsigned* dirty = vm.inc.dirty.as<unsigned>();
  VmGrid* grid = vm.has_bitmap ? vm.grid.as<VmGrid>() : nullptr;
  unsigned long long* bitmap = vm.has_bitmap ? vm.bitmap.as<unsigned long long>() : nullptr;
  const int blocks = (n_rows + VM_SNAP_THREADS - 1) / VM_SNAP_THREADS;
  {
    ProfScope ps(e, prof_class);
    vm_import_kernel<FROM_MAP><<<blocks, VM_SNAP_THREADS, 0, e->stream>>>(d_coords, d_sums, d_ages, n_rows, from ? from->keys_cur() : nullptr, from ? from->occupied.as<int>() : nullptr,
                                                                           from ? from->counters_cur() : nullptr, from ? from->inc.stamps[from->cur].as<unsigned>() : nullptr, in_epoch,
                                                                           keys, vm.capacity - 1, sums, stamps, vm.inc.epoch, dirty, ctl, counters + 1);
    incmap_by_mode(vm, [&](auto m) {
      vm_refresh_kernel<decltype(m)::value><<<(n_rows + 255) / 256, 256, 0, e->stream>>>(dirty, ctl, keys, sums, vm.table.as<uint4>(), counters, vm.occupied.as<int>(), grid, bitmap);
    });
  }
  HIP_OR_FAIL(e, hipGetLastError());
  vm.inc.voxel_bound += n_rows;
  if (!vm.has_bitmap) return incmap_bitmap(e, vm);  // (as an insert: a map that has grown into bitmap territory gets its bitmap here)
  return FVH_OK;
}

int incmap_import(Engine* e, VoxelMapDev& vm, int n, const int* coords3, const double* sums10, const unsigned* ages, double resolution, int mode, int num_inserts, long long num_points) {
  // everything is validated on the host before anything is queued: a refused import leaves the map as it was
  if (n < 0) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: n < 0");
  if ((long long)n > INCMAP_MAX_VOXELS) return e->fail(FVH_ERR_UNSUPPORTED, "voxelmap_import: more than 2^28 voxels");
  if (n > 0 && (!coords3 || !sums10)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: null coords3 / sums10 with n > 0");
  if (!(resolution == vm.res)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: the snapshot's resolution is not the live map's");
  if (mode != incmap_snapshot_mode(vm)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: the snapshot's accumulation mode is not the live map's");
  if (num_inserts < 0 || num_points < 0) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: negative num_inserts / num_points");
  const int lim = FVH_COORD_BIAS - 4096;  // the range voxel_index_ok gives an inserted point
  for (int i = 0; i < n; i++) {
    const int* c = coords3 + 3 * (size_t)i;
    const double* s = sums10 + VM_ACC_STRIDE * (size_t)i;
    for (int a = 0; a < 3; a++)
      if (c[a] <= -lim || c[a] >= lim) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: voxel " + std::to_string(i) + ": coordinate out of range (|c| < 2^20 - 4096)");
    for (int j = 0; j < VM_ACC_STRIDE; j++)
      if (!std::isfinite(s[j])) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: voxel " + std::to_string(i) + ": a sum is not finite");
    if (!(s[9] >= 1.0) || s[9] != std::floor(s[9]) || s[9] > 2147483647.0) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: voxel " + std::to_string(i) + ": the count is not an integer >= 1");
    if ((ages ? ages[i] : 0u) >= (unsigned)num_inserts) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_import: voxel " + std::to_string(i) + ": age >= num_inserts");
  }
  { int rc = incmap_secure(e, vm, n, "voxelmap_import"); if (rc) return rc; }
  const size_t sums_bytes = sizeof(double) * VM_ACC_STRIDE * (size_t)n, coords_bytes = sizeof(int) * 3 * (size_t)n, ages_bytes = sizeof(unsigned) * (size_t)n;
  double* d_sums = nullptr;
  int* d_coords = nullptr;
  unsigned* d_ages = nullptr;
  if (n > 0) {
    HIP_OR_FAIL(e, vm.inc.xfer.ensure(sums_bytes + coords_bytes + ages_bytes));
    d_sums = vm.inc.xfer.as<double>();
    d_coords = reinterpret_cast<int*>(static_cast<char*>(vm.inc.xfer.p) + sums_bytes);
    HIP_OR_FAIL(e, hipMemcpyAsync(d_sums, sums10, sums_bytes, hipMemcpyHostToDevice, e->stream));
    HIP_OR_FAIL(e, hipMemcpyAsync(d_coords, coords3, coords_bytes, hipMemcpyHostToDevice, e->stream));
    if (ages) {
      d_ages = reinterpret_cast<unsigned*>(static_cast<char*>(vm.inc.xfer.p) + sums_bytes + coords_bytes);
      HIP_OR_FAIL(e, hipMemcpyAsync(d_ages, ages, ages_bytes, hipMemcpyHostToDevice, e->stream));
    }
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));  // the caller's arrays are free again when the call returns
  }
  return incmap_add_rows<false>(e, vm, n, d_coords, d_sums, d_ages, nullptr, (unsigned)num_inserts, num_points, "map_import");
}

// `from` (a live map of another handle on the same device, stream from_stream) added into `vm`, device to device. The reads of `from` are
// fenced on both sides: e's stream waits for what from_stream holds, and from_stream waits for the kernel.
int incmap_merge_from(Engine* e, VoxelMapDev& vm, VoxelMapDev& from, hipStream_t from_stream, hipEvent_t ev_before, hipEvent_t ev_after) {
  if (!(from.res == vm.res)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_merge_from: the two maps differ in resolution");
  if (from.inc.mode != vm.inc.mode) return e->fail(FVH_ERR_INVALID_ARGUMENT, "voxelmap_merge_from: the two maps differ in accumulation mode");
  HIP_OR_FAIL(e, hipEventRecord(ev_before, from_stream));
  HIP_OR_FAIL(e, hipStreamWaitEvent(e->stream, ev_before, 0));
  // the other map's voxel count stays on the device: its host bound sizes the launch, a readback refines it only when it would force a growth
  long long n_bound = from.inc.voxel_bound;
  if (vm.inc.voxel_bound + n_bound > INCMAP_MAX_VOXELS || 2 * (vm.inc.voxel_bound + n_bound) > (long long)vm.capacity) {
    int cnt[3];
    HIP_OR_FAIL(e, hipMemcpyAsync(cnt, from.counters_cur(), 3 * sizeof(int), hipMemcpyDeviceToHost, e->stream));  // (e's stream: ordered after from_stream by the event)
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
    from.inc.voxel_bound = n_bound = cnt[0];
  }
  { int rc = incmap_secure(e, vm, n_bound, "voxelmap_merge_from"); if (rc) return rc; }
  const int rc = incmap_add_rows<true>(e, vm, (int)n_bound, nullptr, from.inc.sums[from.cur].as<double>(), nullptr, &from, from.inc.epoch, from.inc.num_points, "map_merge");
  HIP_OR_FAIL(e, hipEventRecord(ev_after, e->stream));
  HIP_OR_FAIL(e, hipStreamWaitEvent(from_stream, ev_after, 0));
  return rc;
}

// ---- a live map added under a rigid pose (fvh_*_posed_merge_from / fvh_*_transform_map; kernels_voxelmap.hpp: "added under a
// rigid pose"). The callers have validated T16 (deskew_rigid) before anything is queued.

// the rows of `src` (buffers of side src_side, counter set src_side) under T into side `to` of `vm`: kernel + the insert's refresh.
// ctl[0] (dirty count) and ctl[1] (rows skipped) are zeroed in front; `grid` as incmap_add_rows passes it, or null when the bitmap is rebuilt afterwards
int incmap_posed_launch(Engine* e, VoxelMapDev& vm, int to, const VoxelMapDev& src, int src_side, int n_rows, const double* T16, bool live_bitmap, const char* prof_class) {
  HIP_OR_FAIL(e, vm.inc.dirty.ensure(sizeof(unsigned) * (size_t)n_rows));
  HIP_OR_FAIL(e, hipMemsetAsync(vm.inc.ctl.p, 0, 2 * sizeof(int), e->stream));
  const PoseD T = pose_from_colmajor16(T16);
  unsigned long long* keys = vm.keys[to].as<unsigned long long>();
  double* sums = vm.inc.sums[to].as<double>();
  unsigned* stamps = vm.inc.stamps[to].as<unsigned>();
  int* counters = vm.counters.as<int>() + 16 * to;
  int* ctl = vm.inc.ctl.as<int>();
  unsigned* dirty = vm.inc.dirty.as<unsigned>();
  VmGrid* grid = live_bitmap ? vm.grid.as<VmGrid>() : nullptr;
  unsigned long long* bitmap = live_bitmap ? vm.bitmap.as<unsigned long long>() : nullptr;
  const int blocks = (n_rows + VM_SNAP_THREADS - 1) / VM_SNAP_THREADS;
  {
    ProfScope ps(e, prof_class);
    incmap_by_mode(vm, [&](auto m) {
      constexpr int M = decltype(m)::value;
      vm_import_posed_kernel<M><<<blocks, VM_SNAP_THREADS, 0, e->stream>>>(src.keys[src_side].as<unsigned long long>(), src.inc.sums[src_side].as<double>(), src.inc.stamps[src_side].as<unsigned>(),
                                                                           src.occupied.as<int>(), src.counters.as<int>() + 16 * src_side, n_rows, src.inc.epoch, T, vm.res, keys,
                                                                           vm.capacity - 1, sums, stamps, vm.inc.epoch, dirty, ctl, counters + 1);
      vm_refresh_kernel<M><<<(n_rows + 255) / 256, 256, 0, e->stream>>>(dirty, ctl, keys, sums, vm.table.as<uint4>(), counters, vm.occupied.as<int>(), grid, bitmap);
    });
  }
  HIP_OR_FAIL(e, hipGetLastError());
  return FVH_OK;
}

int incmap_read_rows_skipped(Engine* e, VoxelMapDev& vm, int* rows_skipped) {
  if (!rows_skipped) return FVH_OK;
  HIP_OR_FAIL(e, hipMemcpyAsync(rows_skipped, vm.inc.ctl.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
  return FVH_OK;
}

// `from` seen from pose T added into `vm`: incmap_merge_from's fences, capacity and bookkeeping around the posed kernel
int incmap_merge_from_posed(Engine* e, VoxelMapDev& vm, VoxelMapDev& from, hipStream_t from_stream, hipEvent_t ev_before, hipEvent_t ev_after, const double* T16, int* rows_skipped) {
  if (!(from.res == vm.res)) return e->fail(FVH_ERR_INVALID_ARGUMENT, "posed_merge_from: the two maps differ in resolution");
  if (from.inc.mode != vm.inc.mode) return e->fail(FVH_ERR_INVALID_ARGUMENT, "posed_merge_from: the two maps differ in accumulation mode");
  HIP_OR_FAIL(e, hipEventRecord(ev_before, from_stream));
  HIP_OR_FAIL(e, hipStreamWaitEvent(e->stream, ev_before, 0));
  long long n_bound = std::min<long long>(from.inc.voxel_bound, (long long)from.capacity);  // (the host keeps the load factor <= 0.5: capacity bounds the count too)
  if (vm.inc.voxel_bound + n_bound > INCMAP_MAX_VOXELS || 2 * (vm.inc.voxel_bound + n_bound) > (long long)vm.capacity) {
    int cnt[3];
    HIP_OR_FAIL(e, hipMemcpyAsync(cnt, from.counters_cur(), 3 * sizeof(int), hipMemcpyDeviceToHost, e->stream));  // (e's stream: ordered after from_stream by the event)
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
    from.inc.voxel_bound = n_bound = cnt[0];
  }
  { int rc = incmap_secure(e, vm, n_bound, "posed_merge_from"); if (rc) return rc; }
  vm.inc.epoch = std::max(vm.inc.epoch, from.inc.epoch);
  vm.inc.num_points += from.inc.num_points;
  vm.host_valid = false;
  vm.has_canon = false;
  e->has_corr = false;
  if (rows_skipped) *rows_skipped = 0;
  if (n_bound == 0) return FVH_OK;  // (nothing was queued on our stream that reads `from`)
  int rc = incmap_posed_launch(e, vm, vm.cur, from, from.cur, (int)n_bound, T16, vm.has_bitmap, "map_merge_posed");
  if (rc) return rc;
  vm.inc.voxel_bound += n_bound;
  HIP_OR_FAIL(e, hipEventRecord(ev_after, e->stream));
  HIP_OR_FAIL(e, hipStreamWaitEvent(from_stream, ev_after, 0));
  if (!vm.has_bitmap) rc = incmap_bitmap(e, vm);  // (as an insert: a map that has grown into bitmap territory gets its bitmap here)
  return rc ? rc : incmap_read_rows_skipped(e, vm, rows_skipped);
}

// the live map re-anchored in place: one pass from the current key / sums / stamp buffers into the other set at the same capacity (the
// voxel count cannot grow), which ADDS -- rows may meet in one voxel --, then the refresh and the bitmap as after a rehash. Insert count,
// num_points and every row's age stay: a row's stamp goes over as it is (age = epoch - stamp on both sides).
int incmap_transform(Engine* e, VoxelMapDev& vm, const double* T16, int* rows_skipped) {
  const int from = vm.cur, to = vm.cur ^ 1;
  const int n_bound = (int)std::min<long long>(vm.inc.voxel_bound, (long long)vm.capacity);
  { int rc = incmap_prepare_side(e, vm, to, vm.capacity); if (rc) return rc; }
  vm_rehash_begin_kernel<<<1, 64, 0, e->stream>>>(vm.counters_cur(), vm.counters.as<int>() + 16 * to, vm.inc.ctl.as<int>());
  HIP_OR_FAIL(e, hipGetLastError());
  if (rows_skipped) *rows_skipped = 0;
  if (n_bound > 0) { int rc = incmap_posed_launch(e, vm, to, vm, from, n_bound, T16, false, "transform_map"); if (rc) return rc; }
  vm.cur = to;
  vm.host_valid = false;
  vm.has_canon = false;
  e->has_corr = false;  // stored correspondences are bucket indices of the old table
  { int rc = incmap_bitmap(e, vm); if (rc) return rc; }
  return n_bound > 0 ? incmap_read_rows_skipped(e, vm, rows_skipped) : (int)FVH_OK;
}

// ---- the live map as a point target (fvh_vgicp_target_from_map / fvh_ndt_target_from_map; kernels_voxelmap.hpp: "point target") ---------
// Cloud `c` becomes one point per voxel with >= min_points points -- the record's float mean, with_cov: + the record's covariance -- rows in
// ascending packed-key order (the row order of incmap_export). The map is only read. Everything is queued on the main stream with scratch of
// the map's own (VoxelMapDev::inc.tm_*): a preparation on the second stream may hold the Engine-wide sort buffers (finding 1),
// which is also why the cloud's Morton order stays lazy here (ensure_sorted where it is consumed, as for any cloud).
// One readback {selected, voxel count, bounds} sizes the sort and names the key route; the cloud's size is host state, so it is not optional.
// Order by the 63-bit key: ONE radix sweep over the key compressed against the bounds of the selected voxels whenever that box fits 32 bits
// (a 300 m x 300 m x 30 m map at 0.5 m: 10 + 10 + 6 bits = 3 passes of 9 bits), else two stable sweeps, low word then high word (8 passes).
inline int bits_for_span(unsigned span) { int b = 0; while (b < 32 && (span >> b) != 0u) b++; return b; }  // values 0..span need this many bits

int incmap_to_cloud(Engine* e, VoxelMapDev& vm, int min_points, CloudDev& c, bool with_cov, bool want_box, int* num_points) {
  VoxelMapDev::Incremental& inc = vm.inc;
  const int bound = (int)std::min<long long>(inc.voxel_bound, (long long)vm.capacity);  // (the host keeps the load factor <= 0.5: capacity bounds the count too)
  HIP_OR_FAIL(e, inc.tm_ctl.ensure(sizeof(VmTargetCtl)));
  VmTargetCtl* d_ctl = inc.tm_ctl.as<VmTargetCtl>();
  unsigned long long* sel_keys = nullptr;
  unsigned* sel_buckets = nullptr;
  VmTargetCtl ctl;
  std::memset(&ctl, 0, sizeof(ctl));
  if (bound > 0) {
    HIP_OR_FAIL(e, inc.tm_sel.ensure((sizeof(unsigned long long) + sizeof(unsigned)) * (size_t)bound));
    sel_keys = inc.tm_sel.as<unsigned long long>();
    sel_buckets = reinterpret_cast<unsigned*>(sel_keys + bound);
    {
      ProfScope ps(e, "map_target");
      const int chunks = (bound + VM_FIN_THREADS - 1) / VM_FIN_THREADS;
      vm_target_begin_kernel<<<1, 64, 0, e->stream>>>(d_ctl);
      vm_target_select_kernel<<<std::min(chunks, VM_TARGET_MAX_WGS), VM_FIN_THREADS, 0, e->stream>>>(vm.table.as<uint4>(), vm.occupied.as<int>(), vm.counters_cur(), bound, min_points, sel_keys,
                                                                                                      sel_buckets, d_ctl);
    }
    HIP_OR_FAIL(e, hipGetLastError());
    HIP_OR_FAIL(e, hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, e->stream));
    HIP_OR_FAIL(e, hipStreamSynchronize(e->stream));
    inc.voxel_bound = ctl.num_voxels;
  }
  const int m = ctl.selected;
  // from here on the cloud is replaced (what set_*_cloud drops: covariances, neighbours, Morton order)
  c.has_cov = false; c.has_nbr = false; c.has_cov_sorted = false; c.has_sorted = false;
  if (num_points) *num_points = m;
  if (m == 0) { c.n = 0; c.has_pts = false; return FVH_OK; }  // no voxel qualifies: no target cloud
  HIP_OR_FAIL(e, inc.tm_keys.ensure(sizeof(unsigned) * 2 * (size_t)m));
  HIP_OR_FAIL(e, inc.tm_idx.ensure(sizeof(int) * 2 * (size_t)m));
  HIP_OR_FAIL(e, inc.tm_rows.ensure(sizeof(float4) * (size_t)m));
  if (with_cov) HIP_OR_FAIL(e, c.cov.ensure(sizeof(float4) * 2 * (size_t)m));
  unsigned* keys[2] = {inc.tm_keys.as<unsigned>(), inc.tm_keys.as<unsigned>() + m};
  int* idx[2] = {inc.tm_idx.as<int>(), inc.tm_idx.as<int>() + m};
  const int blocks = (m + 255) / 256;
  VmTargetKey kp;
  std::memset(&kp, 0, sizeof(kp));
  const int bx = bits_for_span(ctl.umax[0] - ctl.umin[0]), by = bits_for_span(ctl.umax[1] - ctl.umin[1]), bz = bits_for_span(ctl.umax[2] - ctl.umin[2]);
  const int* order = nullptr;
  {
    ProfScope ps(e, "map_target");
    int sorted = 0;
    if (bx + by + bz <= 32) {
      for (int a = 0; a < 3; a++) kp.lo[a] = ctl.umin[a];
      kp.bx = bx; kp.bxy = bx + by; kp.part = 0;
      vm_target_keys_kernel<<<blocks, 256, 0, e->stream>>>(sel_keys, nullptr, m, kp, keys[0], idx[0]);
      { const int rc = radix_sort_pairs(e, keys, idx, m, bx + by + bz, &sorted, e->stream, &inc.tm_hist); if (rc) return rc; }
      order = idx[sorted];
    } else {
      kp.part = 1;
      vm_target_keys_kernel<<<blocks, 256, 0, e->stream>>>(sel_keys, nullptr, m, kp, keys[0], idx[0]);
      { const int rc = radix_sort_pairs(e, keys, idx, m, 32, &sorted, e->stream, &inc.tm_hist); if (rc) return rc; }
      // the second sweep starts from the first one's result: radix_sort_pairs reads pair 0 first
      unsigned* keys2[2] = {keys[sorted], keys[sorted ^ 1]};
      int* idx2[2] = {idx[sorted], idx[sorted ^ 1]};
      kp.part = 2;
      vm_target_keys_kernel<<<blocks, 256, 0, e->stream>>>(sel_keys, idx2[0], m, kp, keys2[0], idx2[0]);
      { const int rc = radix_sort_pairs(e, keys2, idx2, m, 31, &sorted, e->stream, &inc.tm_hist); if (rc) return rc; }
      order = idx2[sorted];
    }
    vm_target_gather_kernel<<<blocks, 256, 0, e->stream>>>(vm.table.as<float4>(), sel_buckets, order, m, inc.tm_rows.as<float4>(), with_cov ? c.cov.as<float4>() : nullptr);
  }
  HIP_OR_FAIL(e, hipGetLastError());
  // into the cloud as fvh_*_set_target_cloud_device takes a float4 array: the same pack kernel, the same bounding cube for the sort
  { const int rc = upload_cloud(e, c, inc.tm_rows.as<float>(), m, 4, true, want_box); if (rc) return rc; }
  c.has_cov = with_cov;
  return FVH_OK;
}
