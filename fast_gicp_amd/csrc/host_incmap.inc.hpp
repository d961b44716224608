// Incremental target voxel map of a VGICP handle (fvh_vgicp_map_*): a map that keeps its per-voxel sums, takes posed scans in place and
// can be pruned. Kernels and buffer layout: kernels_voxelmap.hpp ("incremental target map").
// (a section of the host translation unit: included by fvh_capi.hip inside its anonymous namespace, after host_stages.inc.hpp)
//
// The map lives in the handle's VoxelMapDev like a batch map -- keys[cur], table, occupied, counter set `cur`, bitmap / grid -- so
// everything that consumes a target map (launch_cost, the getters) reads it unchanged. The sums, stamps and the dirty list are its own
// (VoxelMapDev::inc); VoxelMapDev::acc and its clean / dirty bookkeeping stay build_voxelmap's.
// Everything is queued on the handle's main stream; the callers (CHECK_HANDLE) have ordered it after a pending side-stream build.

constexpr int INCMAP_DEFAULT_VOXELS = 16384;
constexpr unsigned INCMAP_MIN_CAPACITY = 64;
constexpr long long INCMAP_MAX_VOXELS = 1LL << 28;  // 4 x this is the largest table a 32-bit bucket index (bit 31: "new") addresses

inline unsigned incmap_capacity_for(long long voxels) {  // load factor <= 0.25 at `voxels`, as the batch build sizes its table
  unsigned cap = INCMAP_MIN_CAPACITY;
  while ((long long)cap < 4 * voxels) cap <<= 1;
  return cap;
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
  vm.inc.mode = mode == 2 ? 2 : 0;
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
  if (vm.inc.mode == 2)
    vm_rehash_kernel<2><<<blocks, VM_FIN_THREADS, 0, e->stream>>>(vm.keys[from].as<unsigned long long>(), vm.inc.sums[from].as<double>(), vm.inc.stamps[from].as<unsigned>(), old_cap,
                                                                   vm.keys[to].as<unsigned long long>(), new_cap - 1, vm.inc.sums[to].as<double>(), vm.inc.stamps[to].as<unsigned>(),
                                                                   vm.table.as<uint4>(), next_counters, vm.occupied.as<int>(), prune, vm.inc.ctl.as<int>());
  else
    vm_rehash_kernel<0><<<blocks, VM_FIN_THREADS, 0, e->stream>>>(vm.keys[from].as<unsigned long long>(), vm.inc.sums[from].as<double>(), vm.inc.stamps[from].as<unsigned>(), old_cap,
                                                                   vm.keys[to].as<unsigned long long>(), new_cap - 1, vm.inc.sums[to].as<double>(), vm.inc.stamps[to].as<unsigned>(),
                                                                   vm.table.as<uint4>(), next_counters, vm.occupied.as<int>(), prune, vm.inc.ctl.as<int>());
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
  if (!vm.inc.live || !vm.valid) return e->fail(FVH_ERR_BAD_STATE, std::string(who) + ": no incremental map is live (fvh_vgicp_map_begin)");
  if (!c.has_pts || !c.has_cov) return e->fail(FVH_ERR_BAD_STATE, std::string(who) + ": the cloud needs points and covariances");
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
    if (vm.inc.mode == 2) {
      vm_insert_kernel<2><<<blocks, 256, 0, e->stream>>>(c.pts.as<float4>(), c.cov.as<float4>(), n, T, vm.res, keys, vm.capacity - 1, sums, stamps, vm.inc.epoch, dirty, ctl, counters + 1, order);
      vm_refresh_kernel<2><<<blocks, 256, 0, e->stream>>>(dirty, ctl, keys, sums, vm.table.as<uint4>(), counters, vm.occupied.as<int>(), grid, bitmap);
    } else {
      vm_insert_kernel<0><<<blocks, 256, 0, e->stream>>>(c.pts.as<float4>(), c.cov.as<float4>(), n, T, vm.res, keys, vm.capacity - 1, sums, stamps, vm.inc.epoch, dirty, ctl, counters + 1, order);
      vm_refresh_kernel<0><<<blocks, 256, 0, e->stream>>>(dirty, ctl, keys, sums, vm.table.as<uint4>(), counters, vm.occupied.as<int>(), grid, bitmap);
    }
  }
  HIP_OR_FAIL(e, hipGetLastError());
  vm.inc.voxel_bound += n;
  // a map that has grown into bitmap territory gets its bitmap here (once: later inserts set bits, or switch it off on the device when a
  // voxel falls outside its box -- the next rehash rebuilds it)
  if (!vm.has_bitmap) return incmap_bitmap(e, vm);
  return FVH_OK;
}

int incmap_prune(Engine* e, VoxelMapDev& vm, const double* center3, double radius, int max_age, int* num_removed) {
  if (!vm.inc.live || !vm.valid) return e->fail(FVH_ERR_BAD_STATE, "map_prune: no incremental map is live (fvh_vgicp_map_begin)");
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
