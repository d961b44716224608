// Gaussian voxel map build for gfx950: spatial-hash insert + LDS-staged bucket accumulation.
//
// Replaces the reference's K10-K17 chain: voxel_coord_kernel,
// voxel_bucket_assignment_kernel (+ host retry loop that drops up to 1 % of the points),
// voxel_coord_select_kernel, accumulate_points_kernel (13 global float atomics per point),
// finalize_voxels_kernel / ndt_finalize_voxels_kernel  (src/fast_gicp/cuda/gaussian_voxelmap.cu:9-289).
//
// HBM layout
//   keys  : capacity x u64 voxel key (EMPTY = ~0). capacity = pow2 >= 4 x (voxel count of the previous
//           build on this handle); first build / overflow fallback: pow2 >= 2 * N_t, which can never
//           overflow. No point is ever dropped: an exhausted probe budget is reported and the host rebuilds.
//           The keys are their own dense array because most probes of the cost kernel MISS (DIRECT27 on
//           a 100k-point scene: 65 %): a miss touches 8 B of a 2 MB array that stays in the XCD's L2
//           instead of a 64-B line of a 16 MB table.
//   table : capacity x 64-byte voxel record, bucket index == key slot (no id indirection):
//           q0 = {key_lo, key_hi, num_points, 0}   q1 = {mean.xyz, (float)num_points}
//           q2 = {c_xx, c_xy, c_xz, c_yy}          q3 = {c_yz, c_zz, 0, 0}
//           Only occupied buckets are ever written or (meaningfully) read: the table is never cleared.
//   acc   : capacity x 10 doubles scratch {sum p (3), sum C or sum pp^T (6), count}; fp64 so the
//           result is independent of the atomic arrival order to ~1e-16.
//   The keys (and the two counters) are double buffered and the finalize pass of build N clears the
//   buffers build N+1 will fill and zeroes the accumulators it consumed, so a steady-state rebuild
//   (swapSourceAndTarget in the reference's loop) is two launches; vm_clear_kernel only runs for the
//   first build at a capacity.
//
// Pass 1 (vm_accumulate): one point per thread. Each workgroup first aggregates its 256 points in
// an LDS mini hash table (ds_cmpst_rtn_b64 claim + ds_add_f64), then flushes each occupied LDS slot
// with ONE global claim (global_atomic_cmpswap_x2) and 10 global_atomic_add_f64 -- instead of 13
// global atomics per point. Scan-ordered clouds put 10-40 points of a block in the same voxel.
// Pass 2 (vm_finalize): one thread per bucket: mean/cov from the sums (+ MIN_EIG for NDT), written
// into the bucket; occupied buckets are also listed compactly (getters, D2D source iteration).
#pragma once
#include "dev_math.hpp"

namespace fvh {

constexpr int VM_LDS_SLOTS = 512;
constexpr int VM_LDS_PROBES = 8;
constexpr int VM_ACC_STRIDE = 10;
// Two accumulator sets per bucket: the workgroup whose CAS CREATED the bucket is its owner and writes its partial sums with
// plain stores; every other contributor adds into the visitor set with memory-side fp64 atomics. In Morton order nearly every
// voxel has one contributing workgroup, so most of the ~10 atomics per (workgroup, voxel) -- 21 of this pass's 33 us at 100k
// points -- become stores. vm_finalize_kernel adds the two sets.
constexpr int VM_ACC_BUCKET = 2 * VM_ACC_STRIDE;
constexpr unsigned VM_MAX_PROBE = 255;

// Claim (or find) the bucket of `key`, linear probing from `slot`. CAS first: an atomic goes to the memory side (the
// XCDs' L2s are not coherent), ~2 us per round trip, and the CAS alone answers both "free" and "already this key".
// `created`: this call's CAS turned an empty bucket into the key's (exactly one caller per bucket and build sees that).
__device__ __forceinline__ unsigned global_claim_from(unsigned long long* keys, unsigned mask, unsigned long long key, unsigned slot, unsigned probes_done, bool& created) {
  const unsigned max_probe = mask < VM_MAX_PROBE ? mask : VM_MAX_PROBE;
  created = false;
  for (unsigned it = probes_done; it <= max_probe; it++) {
    const unsigned long long old = atomicCAS(keys + slot, FVH_EMPTY_KEY, key);
    if (old == FVH_EMPTY_KEY) { created = true; return slot; }
    if (old == key) return slot;
    slot = (slot + 1) & mask;
  }
  return 0xFFFFFFFFu;  // probe budget exhausted: the caller counts it in `dropped` and the host rebuilds at the safe size
}
__device__ __forceinline__ unsigned global_claim(unsigned long long* keys, unsigned mask, unsigned long long key) {
  bool created;
  return global_claim_from(keys, mask, key, hash_slot(key, mask), 0, created);
}

// first build at a capacity (afterwards vm_finalize_kernel leaves everything clean): keys -> EMPTY, accumulators and counters -> 0
__global__ __launch_bounds__(256) void vm_clear_kernel(unsigned long long* __restrict__ keys, double* __restrict__ acc, unsigned capacity, int* __restrict__ counters) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i < capacity) keys[i] = FVH_EMPTY_KEY;
  if (i < capacity * 10) reinterpret_cast<uint4*>(acc)[i] = make_uint4(0, 0, 0, 0);  // 2 x 10 doubles = 10 quads per bucket
  if (i < 16) counters[i] = 0;
}

// ---- target map sharded by the ranks' spatial tiles (multi-GPU) --------------------------------------------------
// A rank that walks one spatial tile of the source only ever looks up the voxels around T * tile: its map may hold just those -- the
// voxels of the tile's bounding box (in voxel coordinates, at the initial guess) widened by a halo = the reach of the neighbour offsets +
// a margin for the motion of the pose during the align. A voxel inside the box receives ALL its points (the box is voxel-aligned), so
// its record is the replicated map's. The cost kernel reports (in a spare slot of its sums, so that every rank learns it) if a source
// element ever leaves the inner box -- then some of its neighbours may be missing from the shard -- and the host redoes the align on the
// full map.
struct VmRegion {
  int lo[3], hi[3];              // voxel coordinates this shard holds, inclusive; lo > hi: nothing
  int inner_lo[3], inner_hi[3];  // base voxels whose whole neighbourhood lies inside
  int pad[2];
};
__global__ __launch_bounds__(1024) void vm_region_kernel(const float4* __restrict__ sorted, int lo, int hi, PoseD T, double res, int halo, int reach, VmRegion* __restrict__ out) {
  __shared__ int smin[3][16], smax[3][16];
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-0x7fffffff - 1, -0x7fffffff - 1, -0x7fffffff - 1};
  for (int j = lo + (int)threadIdx.x; j < hi; j += 1024) {
    const float4 p = sorted[j];
    const double q[3] = {T.r[0] * p.x + T.r[1] * p.y + T.r[2] * p.z + T.t[0], T.r[3] * p.x + T.r[4] * p.y + T.r[5] * p.z + T.t[1], T.r[6] * p.x + T.r[7] * p.y + T.r[8] * p.z + T.t[2]};
    const double f[3] = {floor(q[0] / res - 0.5), floor(q[1] / res - 0.5), floor(q[2] / res - 0.5)};
    if (!voxel_index_ok(f[0], f[1], f[2])) continue;
#pragma unroll
    for (int a = 0; a < 3; a++) { mn[a] = min(mn[a], (int)f[a]); mx[a] = max(mx[a], (int)f[a]); }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    for (int o = 32; o >= 1; o >>= 1) { mn[a] = min(mn[a], __shfl_xor(mn[a], o)); mx[a] = max(mx[a], __shfl_xor(mx[a], o)); }
    if ((threadIdx.x & 63) == 0) { smin[a][threadIdx.x >> 6] = mn[a]; smax[a][threadIdx.x >> 6] = mx[a]; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int a = 0; a < 3; a++) {
      int l = smin[a][0], h = smax[a][0];
      for (int w = 1; w < 16; w++) { l = min(l, smin[a][w]); h = max(h, smax[a][w]); }
      const bool any = l <= h;
      out->lo[a] = any ? l - halo : 1; out->hi[a] = any ? h + halo : 0;
      out->inner_lo[a] = any ? l - halo + reach : 1; out->inner_hi[a] = any ? h + halo - reach : 0;
    }
    out->pad[0] = out->pad[1] = 0;
  }
}

// MODE 0: VGICP additive (sum of points and of point covariances); MODE 1: NDT (sum of points and p p^T);
// MODE 2: VGICP multiplicative (MultiplicativeGaussianVoxel::append, fast_vgicp_voxel.hpp:86-94: sum of C^-1 p and of C^-1)
template <int MODE>
__global__ __launch_bounds__(256) void vm_accumulate_kernel(const float4* __restrict__ pts, const float4* __restrict__ cov, int n, double res,
                                                            unsigned long long* __restrict__ table_keys, unsigned mask, double* __restrict__ acc,
                                                            int* __restrict__ dropped, const int* __restrict__ order, const VmRegion* __restrict__ region = nullptr,
                                                            int float_coord = 0 /* FVH_COMPUTE_CUDA_COMPAT: the coordinate in float, as vector3_hash.cuh:35-38 */) {
  __shared__ unsigned long long lkey[VM_LDS_SLOTS];
  __shared__ double lacc[VM_LDS_SLOTS * VM_ACC_STRIDE];
  const int tid = threadIdx.x;
  for (int s = tid; s < VM_LDS_SLOTS; s += 256) lkey[s] = FVH_EMPTY_KEY;
  for (int s = tid; s < VM_LDS_SLOTS * VM_ACC_STRIDE; s += 256) lacc[s] = 0.0;
  __syncthreads();

  const int i0 = blockIdx.x * 256 + tid;
  if (i0 < n) {
    const int i = order ? order[i0] : i0;  // Morton order: a workgroup's 256 points share a handful of voxels -> the LDS stage absorbs them
    const float4 p = pts[i];
    // fp64 coordinate, as the CPU reference (fast_vgicp_voxel.hpp:158-160); float_coord: (x.array() / resolution - 0.5).floor() in float like the
    // CUDA class -- the two differ for points within float rounding of a voxel face when the resolution is not a power of two
    double fx, fy, fz;
    if (float_coord) {
      const float rf = (float)res;
      fx = (double)floorf(__fsub_rn(__fdiv_rn(p.x, rf), 0.5f)); fy = (double)floorf(__fsub_rn(__fdiv_rn(p.y, rf), 0.5f)); fz = (double)floorf(__fsub_rn(__fdiv_rn(p.z, rf), 0.5f));
    } else {
      fx = floor((double)p.x / res - 0.5); fy = floor((double)p.y / res - 0.5); fz = floor((double)p.z / res - 0.5);
    }
    const bool ok = voxel_index_ok(fx, fy, fz);
    const int cx = ok ? (int)fx : 0, cy = ok ? (int)fy : 0, cz = ok ? (int)fz : 0;
    bool outside = false;  // a sharded map (VmRegion) holds the voxels of its box only: other points are somebody else's
    if (region && ok) outside = cx < region->lo[0] || cx > region->hi[0] || cy < region->lo[1] || cy > region->hi[1] || cz < region->lo[2] || cz > region->hi[2];
    if (outside) {
    } else if (!ok) {
      // non-finite or absurdly far point: it belongs to no voxel. Counted apart from `dropped` (table overflow, which the
      // host answers with a rebuild at the safe size) so that one lidar NaN cannot fail an align.
      atomicAdd(dropped + 1, 1);
    } else {
      const unsigned long long key = pack_key(cx, cy, cz);
      double v[VM_ACC_STRIDE];
      v[0] = p.x; v[1] = p.y; v[2] = p.z;
      if (MODE == 0) {
        const float4 c0 = cov[2 * i], c1 = cov[2 * i + 1];
        v[3] = c0.x; v[4] = c0.y; v[5] = c0.z; v[6] = c0.w; v[7] = c1.x; v[8] = c1.y;
      } else if (MODE == 2) {
        const float4 c0 = cov[2 * i], c1 = cov[2 * i + 1];
        const Sym3<double> Ci = inverse(Sym3<double>{(double)c0.x, (double)c0.y, (double)c0.z, (double)c0.w, (double)c1.x, (double)c1.y});
        const Vec3<double> cp = mul(Ci, Vec3<double>{(double)p.x, (double)p.y, (double)p.z});
        v[0] = cp.x; v[1] = cp.y; v[2] = cp.z;
        v[3] = Ci.xx; v[4] = Ci.xy; v[5] = Ci.xz; v[6] = Ci.yy; v[7] = Ci.yz; v[8] = Ci.zz;
      } else {
        const double x = p.x, y = p.y, z = p.z;
        v[3] = x * x; v[4] = x * y; v[5] = x * z; v[6] = y * y; v[7] = y * z; v[8] = z * z;
      }
      v[9] = 1.0;
      // stage in the workgroup's LDS mini table
      unsigned slot = hash_slot(key, VM_LDS_SLOTS - 1);
      bool staged = false;
#pragma unroll 1
      for (int pr = 0; pr < VM_LDS_PROBES; pr++) {
        unsigned long long old = atomicCAS(&lkey[slot], FVH_EMPTY_KEY, key);
        if (old == FVH_EMPTY_KEY || old == key) { staged = true; break; }
        slot = (slot + 1) & (VM_LDS_SLOTS - 1);
      }
      if (staged) {
#pragma unroll
        for (int j = 0; j < VM_ACC_STRIDE; j++) atomicAdd(&lacc[slot * VM_ACC_STRIDE + j], v[j]);
      } else {  // LDS table crowded: go straight to the global table
        unsigned b = global_claim(table_keys, mask, key);
        if (b != 0xFFFFFFFFu) {
#pragma unroll
          for (int j = 0; j < VM_ACC_STRIDE; j++) atomicAdd(&acc[(size_t)b * VM_ACC_BUCKET + VM_ACC_STRIDE + j], v[j]);  // (a lone point: always a visitor)
        } else {
          atomicAdd(dropped, 1);
        }
      }
    }
  }
  __syncthreads();
  // flush: one global claim + 10 fp64 atomics per (workgroup, voxel). A thread owns two LDS slots: the first probes of
  // both are in flight together (each is a memory-side round trip).
  static_assert(VM_LDS_SLOTS == 512, "two LDS slots per thread of a 256-thread workgroup");
  unsigned long long fk[2], fold[2];
  unsigned fslot[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    fk[u] = lkey[tid + 256 * u];
    fslot[u] = hash_slot(fk[u], mask);
    fold[u] = FVH_EMPTY_KEY;
    if (fk[u] != FVH_EMPTY_KEY) fold[u] = atomicCAS(table_keys + fslot[u], FVH_EMPTY_KEY, fk[u]);
  }
#pragma unroll
  for (int u = 0; u < 2; u++) {
    if (fk[u] == FVH_EMPTY_KEY) continue;
    const int s = tid + 256 * u;
    unsigned b = fslot[u];
    bool created = fold[u] == FVH_EMPTY_KEY;
    if (fold[u] != FVH_EMPTY_KEY && fold[u] != fk[u]) b = global_claim_from(table_keys, mask, fk[u], (fslot[u] + 1) & mask, 1, created);
    if (b == 0xFFFFFFFFu) { atomicAdd(dropped, 1); continue; }
    if (created) {  // owner: nobody else writes this half
      uint4* dst = reinterpret_cast<uint4*>(acc + (size_t)b * VM_ACC_BUCKET);
#pragma unroll
      for (int j = 0; j < VM_ACC_STRIDE / 2; j++) {
        const double lo = lacc[s * VM_ACC_STRIDE + 2 * j], hi = lacc[s * VM_ACC_STRIDE + 2 * j + 1];
        dst[j] = make_uint4((unsigned)__double2loint(lo), (unsigned)__double2hiint(lo), (unsigned)__double2loint(hi), (unsigned)__double2hiint(hi));
      }
    } else {
#pragma unroll
      for (int j = 0; j < VM_ACC_STRIDE; j++) atomicAdd(&acc[(size_t)b * VM_ACC_BUCKET + VM_ACC_STRIDE + j], lacc[s * VM_ACC_STRIDE + j]);
    }
  }
}

// One thread per bucket. MODE 0: AdditiveGaussianVoxel::finalize (fast_vgicp_voxel.hpp:118-121,
// gaussian_voxelmap.cu:164-171). MODE 1: ndt_finalize_voxels_kernel (gaussian_voxelmap.cu:184-193)
// + MIN_EIG regularisation (ndt_cuda.cu:128,139).
constexpr int VM_FIN_THREADS = 1024;  // buckets per workgroup = counter atomics saved
template <int MODE>
__global__ __launch_bounds__(VM_FIN_THREADS) void vm_finalize_kernel(const unsigned long long* __restrict__ keys, uint4* __restrict__ table, unsigned capacity, double* __restrict__ acc,
                                                          int* __restrict__ num_voxels, int* __restrict__ occupied, float4* __restrict__ compact_pts, float4* __restrict__ compact_cov,
                                                          unsigned long long* __restrict__ next_keys, int* __restrict__ next_counters) {
  // NDT (MODE 1) regularises every voxel covariance through an eigen-decomposition (~1,000 dependent fp64 instructions). At a
  // load factor of 0.25 a wave of buckets holds ~16 voxels, i.e. it would pay the decomposition for a quarter-full wave: the
  // workgroup's voxels are compacted through LDS first and regularised by the first ceil(count / 64) waves, one voxel per lane.
  constexpr bool DENSE = (MODE == 1);
  __shared__ int s_wave_cnt[VM_FIN_THREADS / 64], s_base;
  __shared__ double s_cov[DENSE ? VM_FIN_THREADS : 1][7];  // raw covariance + the weight sqrt(n)
  __shared__ unsigned s_bucket[DENSE ? VM_FIN_THREADS : 1];
  const unsigned b = blockIdx.x * VM_FIN_THREADS + threadIdx.x;
  bool live = false;
  float mxf = 0.f, myf = 0.f, mzf = 0.f;
  float4 q2 = make_float4(0, 0, 0, 0), q3 = q2;
  Sym3<double> C = {0, 0, 0, 0, 0, 0};
  double wn = 0.0;
  unsigned long long key = FVH_EMPTY_KEY;
  if (b < capacity) {
    next_keys[b] = FVH_EMPTY_KEY;  // the buffers of the NEXT build (the map before this one is dead)
    if (b < 16) next_counters[b] = 0;
    key = keys[b];
  }
  if (key != FVH_EMPTY_KEY) {
    uint4 q0 = make_uint4((unsigned)key, (unsigned)(key >> 32), 0u, 0u);
    double a[VM_ACC_STRIDE];
    {
      uint4* aq = reinterpret_cast<uint4*>(acc + (size_t)b * VM_ACC_BUCKET);  // 2 x 80 B per bucket (owner sums, visitor sums), 16-B aligned
#pragma unroll
      for (int j = 0; j < VM_ACC_STRIDE / 2; j++) {
        const uint4 v = aq[j], w = aq[VM_ACC_STRIDE / 2 + j];
        a[2 * j] = __hiloint2double((int)v.y, (int)v.x) + __hiloint2double((int)w.y, (int)w.x);
        a[2 * j + 1] = __hiloint2double((int)v.w, (int)v.z) + __hiloint2double((int)w.w, (int)w.z);
        aq[j] = make_uint4(0, 0, 0, 0);  // consumed: clean for the next build
        aq[VM_ACC_STRIDE / 2 + j] = make_uint4(0, 0, 0, 0);
      }
    }
    const double cnt = a[9];
    const double inv = 1.0 / cnt;
    double mx = a[0] * inv, my = a[1] * inv, mz = a[2] * inv;
    if (MODE == 0) {
      C.xx = a[3] * inv; C.xy = a[4] * inv; C.xz = a[5] * inv; C.yy = a[6] * inv; C.yz = a[7] * inv; C.zz = a[8] * inv;
    } else if (MODE == 2) {  // MultiplicativeGaussianVoxel::finalize (fast_vgicp_voxel.hpp:96-102): cov = (sum C^-1)^-1, mean = cov * sum C^-1 p
      C = inverse(Sym3<double>{a[3], a[4], a[5], a[6], a[7], a[8]});
      const Vec3<double> m = mul(C, Vec3<double>{a[0], a[1], a[2]});
      mx = m.x; my = m.y; mz = m.z;
    } else {  // (regularised below, on dense waves)
      C.xx = (a[3] - mx * a[0]) * inv; C.xy = (a[4] - mx * a[1]) * inv; C.xz = (a[5] - mx * a[2]) * inv;
      C.yy = (a[6] - my * a[1]) * inv; C.yz = (a[7] - my * a[2]) * inv; C.zz = (a[8] - mz * a[2]) * inv;
    }
    const int n = (int)cnt;
    q0.z = (unsigned)n;
    q0.w = 0;
    // q3.zw: the GICP weight sqrt(n) of the voxel as a double (fast_vgicp_impl.hpp:149) -- once per voxel here instead of once per
    // correspondence and evaluation in the LM kernel
    wn = sqrt((double)n);
    mxf = (float)mx; myf = (float)my; mzf = (float)mz;
    table[(size_t)b * 4] = q0;
    reinterpret_cast<float4*>(table)[(size_t)b * 4 + 1] = make_float4(mxf, myf, mzf, (float)n);
    live = true;
  }  // occupied bucket
  // Compact list of the occupied buckets: ONE atomic per 1024-bucket WORKGROUP on the voxel counter. (Round 1 had one per wave: 4,096
  // same-address atomics at 100k points / 262k buckets -- the memory-side atomic unit retires them one after the other, ~12 ns
  // each, which was the 50 us this kernel took; per voxel it had been 60k of them.)
  const int wv = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(live);
  const int slot_in_wave = __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull));
  if ((threadIdx.x & 63) == 0) s_wave_cnt[wv] = __popcll(mask);
  __syncthreads();
  int total = 0, local = slot_in_wave;  // voxels of this workgroup; this voxel's position among them
  for (int w = 0; w < VM_FIN_THREADS / 64; w++) { const int c = s_wave_cnt[w]; total += c; local += (w < wv) ? c : 0; }
  if (threadIdx.x == 0) s_base = total ? atomicAdd(num_voxels, total) : 0;
  if (DENSE && live) {
    s_cov[local][0] = C.xx; s_cov[local][1] = C.xy; s_cov[local][2] = C.xz; s_cov[local][3] = C.yy; s_cov[local][4] = C.yz; s_cov[local][5] = C.zz; s_cov[local][6] = wn;
    s_bucket[local] = b;
  }
  __syncthreads();
  float4* tf = reinterpret_cast<float4*>(table);
  if (DENSE) {
    // one voxel per lane of the first waves: regularise (ndt_cuda.cu:128,139: MIN_EIG), write the covariance half of the record
    if ((int)threadIdx.x < total) {
      const int t = threadIdx.x;
      const Sym3<double> R = regularize_cov(Sym3<double>{s_cov[t][0], s_cov[t][1], s_cov[t][2], s_cov[t][3], s_cov[t][4], s_cov[t][5]}, 1 /* MIN_EIG */);
      const unsigned bt = s_bucket[t];
      const float4 r2 = make_float4((float)R.xx, (float)R.xy, (float)R.xz, (float)R.yy);
      const double w = s_cov[t][6];
      const float4 r3 = make_float4((float)R.yz, (float)R.zz, __int_as_float(__double2loint(w)), __int_as_float(__double2hiint(w)));
      tf[(size_t)bt * 4 + 2] = r2;
      tf[(size_t)bt * 4 + 3] = r3;
      if (compact_pts) {  // D2D NDT: the source voxels are the "source cloud"
        const int id = s_base + t;
        compact_cov[2 * id] = r2;
        compact_cov[2 * id + 1] = r3;
      }
    }
    if (!live) return;
    const int id = s_base + local;
    occupied[id] = (int)b;
    if (compact_pts) compact_pts[id] = make_float4(mxf, myf, mzf, 0.f);
    return;
  }
  if (!live) return;
  q2 = make_float4((float)C.xx, (float)C.xy, (float)C.xz, (float)C.yy);
  q3 = make_float4((float)C.yz, (float)C.zz, __int_as_float(__double2loint(wn)), __int_as_float(__double2hiint(wn)));
  tf[(size_t)b * 4 + 2] = q2;
  tf[(size_t)b * 4 + 3] = q3;
  const int id = s_base + local;
  occupied[id] = (int)b;
  if (compact_pts) {
    compact_pts[id] = make_float4(mxf, myf, mzf, 0.f);
    compact_cov[2 * id] = q2;
    compact_cov[2 * id + 1] = q3;
  }
}

// ---- canonical order of a map's voxel list (multi-GPU NDT D2D) -----------------------------------------------------------------
// The compact list of a map (`occupied`, compact_pts / compact_cov) is in the order in which the finalize pass's workgroups took their
// ranges from an atomic counter, and a voxel's bucket depends on the order of the build's CAS races: two ranks that build the same map
// hold the same voxels in different orders. Ranks that share a D2D registration must cut the SAME list (north_star: shard by spatial
// tile), so the voxels are ranked by their key -- z-major, then y, then x: contiguous ranges are slabs of space -- and walked in that
// order: order[rank of voxel i] = i. n_v^2 key compares out of LDS (a few thousand voxels: microseconds), one thread per voxel.
__global__ __launch_bounds__(256) void vm_canonical_order_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ occupied, const int* __restrict__ counters,
                                                                 int* __restrict__ order) {
  __shared__ unsigned long long s_keys[1024];
  const int nv = counters[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x * 256 >= nv) return;  // (whole workgroup: uniform)
  const unsigned long long mine = i < nv ? keys[occupied[i]] : 0ull;
  int rank = 0;
  for (int base = 0; base < nv; base += 1024) {
    __syncthreads();
    for (int j = threadIdx.x; j < 1024; j += 256) s_keys[j] = (base + j < nv) ? keys[occupied[base + j]] : FVH_EMPTY_KEY;  // (EMPTY = ~0: never below a voxel key)
    __syncthreads();
    const int m = min(1024, nv - base);
    for (int j = 0; j < m; j++) rank += (s_keys[j] < mine) ? 1 : 0;
  }
  if (i < nv) order[rank] = i;
}

// ---- occupancy bitmap of large maps ------------------------------------------------------------------------------------------
// 65 % of the DIRECT7 / DIRECT27 probes of a registration MISS (the neighbour voxel does not exist), and on a map that no longer
// fits the L2s every miss still pulls a 64-byte sector of the key table out of HBM for an 8-byte compare: at 1M points the LM
// kernel moved 1.46x its algorithmic bytes that way (PMC, round 2). A dense bit per voxel over the map's bounding box -- 4 x 4 x 4
// voxels per 64-bit word, ~1 MB for a 300 m x 300 m map at 0.5 m -- stays cache resident and answers the misses without touching
// the table; only probes whose bit is set (guaranteed hits) go on to the keys and records. Built on the device after the finalize
// pass (bounds of the occupied voxels -> grid -> clear -> set), for maps of FVH_BITMAP_MIN_POINTS points and up (builds of that
// size are rare; small maps are cache resident anyway).
struct VmGrid {
  unsigned umin[3], umax[3];   // bounds of the occupied voxels, biased coordinates (coord + FVH_COORD_BIAS)
  int b0[3], nb[3];            // first block (biased coordinate >> 2) and number of blocks per axis
  unsigned long long nwords;   // nb[0] * nb[1] * nb[2]
  int enabled;                 // 0: the box needs more words than the budget -- lookups go to the table as before
  int pad_;
};
__global__ void vm_grid_init_kernel(VmGrid* __restrict__ g) {
  if (threadIdx.x < 3) { g->umin[threadIdx.x] = 0xFFFFFFFFu; g->umax[threadIdx.x] = 0u; }
  if (threadIdx.x == 0) { g->enabled = 0; g->nwords = 0; }
}
__global__ __launch_bounds__(256) void vm_grid_bounds_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ occupied, const int* __restrict__ num_voxels,
                                                             VmGrid* __restrict__ g) {
  __shared__ unsigned s_min[3], s_max[3];
  if (threadIdx.x < 3) { s_min[threadIdx.x] = 0xFFFFFFFFu; s_max[threadIdx.x] = 0u; }
  __syncthreads();
  const int nv = *num_voxels;
  unsigned mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    const unsigned long long k = keys[occupied[i]];
    const unsigned c[3] = {(unsigned)(k & 0x1FFFFF), (unsigned)((k >> 21) & 0x1FFFFF), (unsigned)((k >> 42) & 0x1FFFFF)};
#pragma unroll
    for (int a = 0; a < 3; a++) { mn[a] = min(mn[a], c[a]); mx[a] = max(mx[a], c[a]); }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) { atomicMin(&s_min[a], mn[a]); atomicMax(&s_max[a], mx[a]); }
  __syncthreads();
  if (threadIdx.x < 3 && s_min[threadIdx.x] != 0xFFFFFFFFu) { atomicMin(&g->umin[threadIdx.x], s_min[threadIdx.x]); atomicMax(&g->umax[threadIdx.x], s_max[threadIdx.x]); }
}
__global__ void vm_grid_setup_kernel(VmGrid* __restrict__ g, unsigned long long budget_words) {
  if (threadIdx.x != 0) return;
  if (g->umin[0] == 0xFFFFFFFFu) { g->enabled = 0; g->nwords = 0; return; }  // empty map
  unsigned long long n = 1;
  for (int a = 0; a < 3; a++) {
    g->b0[a] = (int)(g->umin[a] >> 2);
    g->nb[a] = (int)(g->umax[a] >> 2) - g->b0[a] + 1;
    n *= (unsigned long long)g->nb[a];
  }
  g->nwords = n;
  g->enabled = n <= budget_words ? 1 : 0;
}
__global__ __launch_bounds__(256) void vm_grid_clear_kernel(unsigned long long* __restrict__ bitmap, const VmGrid* __restrict__ g) {
  if (!g->enabled) return;
  const unsigned long long n = g->nwords;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) bitmap[i] = 0ull;
}
__device__ __forceinline__ bool vm_grid_locate(const VmGrid& g, unsigned ux, unsigned uy, unsigned uz, unsigned long long& word, unsigned& bit) {
  const int bx = (int)(ux >> 2) - g.b0[0], by = (int)(uy >> 2) - g.b0[1], bz = (int)(uz >> 2) - g.b0[2];
  if ((unsigned)bx >= (unsigned)g.nb[0] || (unsigned)by >= (unsigned)g.nb[1] || (unsigned)bz >= (unsigned)g.nb[2]) return false;
  word = ((unsigned long long)bz * (unsigned)g.nb[1] + (unsigned)by) * (unsigned)g.nb[0] + (unsigned)bx;
  bit = (ux & 3u) | ((uy & 3u) << 2) | ((uz & 3u) << 4);
  return true;
}
__global__ __launch_bounds__(256) void vm_grid_set_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ occupied, const int* __restrict__ num_voxels,
                                                          const VmGrid* __restrict__ gp, unsigned long long* __restrict__ bitmap) {
  if (!gp->enabled) return;
  const VmGrid g = *gp;
  const int nv = *num_voxels;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    const unsigned long long k = keys[occupied[i]];
    unsigned long long word;
    unsigned bit;
    if (vm_grid_locate(g, (unsigned)(k & 0x1FFFFF), (unsigned)((k >> 21) & 0x1FFFFF), (unsigned)((k >> 42) & 0x1FFFFF), word, bit)) atomicOr(&bitmap[word], 1ull << bit);
  }
}

// ---- incremental target map (fvh_vgicp_map_*: host_incmap.inc.hpp) ------------------------------------------------------------
// A map that grows by accumulation: the per-voxel sums are KEPT (vm_finalize_kernel consumes and zeroes VoxelMapDev::acc; these
// kernels never touch that buffer), so a scan is added with work proportional to the scan:
//   sums   : capacity x 10 doubles {sum p | sum C^-1 p (3), sum C | sum C^-1 (6), count}, bucket index == key slot. One set: every
//            flush adds with fp64 atomics (a bucket lives across launches, so no workgroup can own it).
//   stamps : capacity x u32, the epoch (1-based insert number) of the last insert that touched the bucket; 0 = never touched.
//   dirty  : the buckets an insert touched, bit 31 set on those it created. Appended by the flush whose exchange CHANGED the stamp:
//            once per bucket and insert. One counter atomic per workgroup.
//   ctl    : {dirty count, 0, voxels removed by the last rehash, 0}
// vm_insert (pose applied on the way in) -> vm_refresh (one thread per DIRTY bucket: record from the sums, new buckets listed).
// vm_rehash moves the surviving buckets into the other key / sums / stamp buffers: growth and pruning (linear probing cannot
// delete in place); it recomputes every record from the moved sums, so the single record table needs no second copy.
constexpr unsigned VM_INC_NEW = 0x80000000u;

// the insert runs at a load factor <= 0.5 secured by the host BEFORE the launch, and may probe the whole table: it cannot fail
__device__ __forceinline__ unsigned inc_claim(unsigned long long* keys, unsigned mask, unsigned long long key) {
  unsigned slot = hash_slot(key, mask);
  for (unsigned it = 0; it <= mask; it++) {
    const unsigned long long old = atomicCAS(keys + slot, FVH_EMPTY_KEY, key);
    if (old == FVH_EMPTY_KEY || old == key) return slot;
    slot = (slot + 1) & mask;
  }
  return 0xFFFFFFFFu;
}

// NDT (MODE 1) record in two halves, the arithmetic of vm_finalize_kernel<1> restated expression by expression (equal sums give the batch
// record to the bit). Head: {key, n, mean} written, the raw covariance (sum pp^T - mean sum p^T) / n and the weight sqrt(n) handed back.
// Tail: the MIN_EIG regularisation (an eigen-decomposition, ~1,000 dependent fp64 instructions) and the covariance half of the record --
// apart, so that a pass over half-empty buckets (vm_rehash_kernel<1>) can run it on dense waves.
__device__ __forceinline__ void inc_ndt_record_head(unsigned long long key, const double* a, uint4* __restrict__ table, unsigned b, Sym3<double>& C, double& wn) {
  const double cnt = a[9];
  const double inv = 1.0 / cnt;
  const double mx = a[0] * inv, my = a[1] * inv, mz = a[2] * inv;
  C.xx = (a[3] - mx * a[0]) * inv; C.xy = (a[4] - mx * a[1]) * inv; C.xz = (a[5] - mx * a[2]) * inv;
  C.yy = (a[6] - my * a[1]) * inv; C.yz = (a[7] - my * a[2]) * inv; C.zz = (a[8] - mz * a[2]) * inv;
  const int n = (int)cnt;
  wn = sqrt((double)n);
  table[(size_t)b * 4] = make_uint4((unsigned)key, (unsigned)(key >> 32), (unsigned)n, 0u);
  reinterpret_cast<float4*>(table)[(size_t)b * 4 + 1] = make_float4((float)mx, (float)my, (float)mz, (float)n);
}
__device__ __forceinline__ void inc_ndt_record_tail(const Sym3<double>& C, double wn, uint4* __restrict__ table, unsigned b) {
  const Sym3<double> R = regularize_cov(C, 1 /* MIN_EIG */);
  float4* tf = reinterpret_cast<float4*>(table);
  tf[(size_t)b * 4 + 2] = make_float4((float)R.xx, (float)R.xy, (float)R.xz, (float)R.yy);
  tf[(size_t)b * 4 + 3] = make_float4((float)R.yz, (float)R.zz, __int_as_float(__double2loint(wn)), __int_as_float(__double2hiint(wn)));
}

// record {key, n, mean, cov, sqrt(n)} of bucket b from its sums: the arithmetic of vm_finalize_kernel<MODE>
template <int MODE>
__device__ __forceinline__ void inc_write_record(unsigned long long key, const double* a, uint4* __restrict__ table, unsigned b) {
  if (MODE == 1) {
    Sym3<double> Craw;
    double w;
    inc_ndt_record_head(key, a, table, b, Craw, w);
    inc_ndt_record_tail(Craw, w, table, b);
    return;
  }
  const double cnt = a[9];
  const double inv = 1.0 / cnt;
  double mx = a[0] * inv, my = a[1] * inv, mz = a[2] * inv;
  Sym3<double> C;
  if (MODE == 0) {
    C.xx = a[3] * inv; C.xy = a[4] * inv; C.xz = a[5] * inv; C.yy = a[6] * inv; C.yz = a[7] * inv; C.zz = a[8] * inv;
  } else {
    C = inverse(Sym3<double>{a[3], a[4], a[5], a[6], a[7], a[8]});
    const Vec3<double> m = mul(C, Vec3<double>{a[0], a[1], a[2]});
    mx = m.x; my = m.y; mz = m.z;
  }
  const int n = (int)cnt;
  const double wn = sqrt((double)n);
  float4* tf = reinterpret_cast<float4*>(table);
  table[(size_t)b * 4] = make_uint4((unsigned)key, (unsigned)(key >> 32), (unsigned)n, 0u);
  tf[(size_t)b * 4 + 1] = make_float4((float)mx, (float)my, (float)mz, (float)n);
  tf[(size_t)b * 4 + 2] = make_float4((float)C.xx, (float)C.xy, (float)C.xz, (float)C.yy);
  tf[(size_t)b * 4 + 3] = make_float4((float)C.yz, (float)C.zz, __int_as_float(__double2loint(wn)), __int_as_float(__double2hiint(wn)));
}

// MODE 0 additive, 2 multiplicative, 1 NDT (sum p', sum p' p'^T: no covariances, `cov` is never read). An inserted point is
// p' = (float)(R p + t) and its covariance C' = (float)(R C R^T), both formed in fp64 and rounded once: the values a batch build of the
// transformed cloud would be handed.
template <int MODE>
__global__ __launch_bounds__(256) void vm_insert_kernel(const float4* __restrict__ pts, const float4* __restrict__ cov, int n, PoseD T, double res,
                                                        unsigned long long* __restrict__ table_keys, unsigned mask, double* __restrict__ sums, unsigned* __restrict__ stamps,
                                                        unsigned epoch, unsigned* __restrict__ dirty, int* __restrict__ ctl, int* __restrict__ dropped, const int* __restrict__ order) {
  __shared__ unsigned long long lkey[VM_LDS_SLOTS];
  __shared__ double lacc[VM_LDS_SLOTS * VM_ACC_STRIDE];
  __shared__ int s_cnt, s_base;
  const int tid = threadIdx.x;
  for (int s = tid; s < VM_LDS_SLOTS; s += 256) lkey[s] = FVH_EMPTY_KEY;
  for (int s = tid; s < VM_LDS_SLOTS * VM_ACC_STRIDE; s += 256) lacc[s] = 0.0;
  if (tid == 0) s_cnt = 0;
  __syncthreads();

  unsigned pend[3];  // buckets whose stamp this thread changed: the lone unstaged point + two flushed LDS slots
  int npend = 0;
  const int i0 = blockIdx.x * 256 + tid;
  if (i0 < n) {
    const int i = order ? order[i0] : i0;
    const float4 p = pts[i];
    const double x = p.x, y = p.y, z = p.z;
    const float px = (float)(T.r[0] * x + T.r[1] * y + T.r[2] * z + T.t[0]);
    const float py = (float)(T.r[3] * x + T.r[4] * y + T.r[5] * z + T.t[1]);
    const float pz = (float)(T.r[6] * x + T.r[7] * y + T.r[8] * z + T.t[2]);
    const double fx = floor((double)px / res - 0.5), fy = floor((double)py / res - 0.5), fz = floor((double)pz / res - 0.5);
    if (!voxel_index_ok(fx, fy, fz)) {
      atomicAdd(dropped + 1, 1);  // non-finite / absurdly far: belongs to no voxel (counted as vm_accumulate_kernel does)
    } else {
      const unsigned long long key = pack_key((int)fx, (int)fy, (int)fz);
      double v[VM_ACC_STRIDE];
      if constexpr (MODE == 1) {  // points only: `cov` may be null. The terms vm_accumulate_kernel<1> adds for a cloud that holds p'
        const double qx = px, qy = py, qz = pz;
        v[0] = px; v[1] = py; v[2] = pz;
        v[3] = qx * qx; v[4] = qx * qy; v[5] = qx * qz; v[6] = qy * qy; v[7] = qy * qz; v[8] = qz * qz;
      } else {
        const float4 c0 = cov[2 * i], c1 = cov[2 * i + 1];
        const double C[3][3] = {{(double)c0.x, (double)c0.y, (double)c0.z}, {(double)c0.y, (double)c0.w, (double)c1.x}, {(double)c0.z, (double)c1.x, (double)c1.y}};
        double M[3][3];  // R C
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int c = 0; c < 3; c++) M[r][c] = T.r[3 * r] * C[0][c] + T.r[3 * r + 1] * C[1][c] + T.r[3 * r + 2] * C[2][c];
        auto rcr = [&](int r, int c) { return (double)(float)(M[r][0] * T.r[3 * c] + M[r][1] * T.r[3 * c + 1] + M[r][2] * T.r[3 * c + 2]); };
        const Sym3<double> Cp = {rcr(0, 0), rcr(0, 1), rcr(0, 2), rcr(1, 1), rcr(1, 2), rcr(2, 2)};
        if (MODE == 0) {
          v[0] = px; v[1] = py; v[2] = pz;
          v[3] = Cp.xx; v[4] = Cp.xy; v[5] = Cp.xz; v[6] = Cp.yy; v[7] = Cp.yz; v[8] = Cp.zz;
        } else {
          const Sym3<double> Ci = inverse(Cp);
          const Vec3<double> cp = mul(Ci, Vec3<double>{(double)px, (double)py, (double)pz});
          v[0] = cp.x; v[1] = cp.y; v[2] = cp.z;
          v[3] = Ci.xx; v[4] = Ci.xy; v[5] = Ci.xz; v[6] = Ci.yy; v[7] = Ci.yz; v[8] = Ci.zz;
        }
      }
      v[9] = 1.0;
      unsigned slot = hash_slot(key, VM_LDS_SLOTS - 1);
      bool staged = false;
#pragma unroll 1
      for (int pr = 0; pr < VM_LDS_PROBES; pr++) {
        unsigned long long old = atomicCAS(&lkey[slot], FVH_EMPTY_KEY, key);
        if (old == FVH_EMPTY_KEY || old == key) { staged = true; break; }
        slot = (slot + 1) & (VM_LDS_SLOTS - 1);
      }
      if (staged) {
#pragma unroll
        for (int j = 0; j < VM_ACC_STRIDE; j++) atomicAdd(&lacc[slot * VM_ACC_STRIDE + j], v[j]);
      } else {  // LDS table crowded: straight to the map
        const unsigned b = inc_claim(table_keys, mask, key);
        if (b != 0xFFFFFFFFu) {
#pragma unroll
          for (int j = 0; j < VM_ACC_STRIDE; j++) atomicAdd(&sums[(size_t)b * VM_ACC_STRIDE + j], v[j]);
          const unsigned was = atomicExch(stamps + b, epoch);
          if (was != epoch) pend[npend++] = b | (was == 0u ? VM_INC_NEW : 0u);
        } else {
          atomicAdd(dropped, 1);
        }
      }
    }
  }
  __syncthreads();
  // flush: one claim, 10 fp64 adds and one stamp exchange per (workgroup, voxel); the first probes of a thread's two slots are in flight together
  static_assert(VM_LDS_SLOTS == 512, "two LDS slots per thread of a 256-thread workgroup");
  unsigned long long fk[2], fold[2];
  unsigned fslot[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    fk[u] = lkey[tid + 256 * u];
    fslot[u] = hash_slot(fk[u], mask);
    fold[u] = FVH_EMPTY_KEY;
    if (fk[u] != FVH_EMPTY_KEY) fold[u] = atomicCAS(table_keys + fslot[u], FVH_EMPTY_KEY, fk[u]);
  }
#pragma unroll
  for (int u = 0; u < 2; u++) {
    if (fk[u] == FVH_EMPTY_KEY) continue;
    const int s = tid + 256 * u;
    unsigned b = fslot[u];
    if (fold[u] != FVH_EMPTY_KEY && fold[u] != fk[u]) b = inc_claim(table_keys, mask, fk[u]);
    if (b == 0xFFFFFFFFu) { atomicAdd(dropped, 1); continue; }
#pragma unroll
    for (int j = 0; j < VM_ACC_STRIDE; j++) atomicAdd(&sums[(size_t)b * VM_ACC_STRIDE + j], lacc[s * VM_ACC_STRIDE + j]);
    const unsigned was = atomicExch(stamps + b, epoch);
    if (was != epoch) pend[npend++] = b | (was == 0u ? VM_INC_NEW : 0u);
  }
  // dirty list: positions from an LDS counter, ONE memory-side atomic per workgroup
  const int pos = npend ? atomicAdd(&s_cnt, npend) : 0;
  __syncthreads();
  if (tid == 0) s_base = s_cnt ? atomicAdd(ctl, s_cnt) : 0;
  __syncthreads();
  for (int k = 0; k < npend; k++) dirty[s_base + pos + k] = pend[k];
}

// One thread per DIRTY bucket: the record from the (kept) sums; new buckets join the compact list and the voxel count, and the occupancy
// bitmap of a large map: a bit inside its box is set, a voxel outside it switches the bitmap off on the device (the LM kernel reads
// VmGrid::enabled per launch) until the next rehash rebuilds it.
template <int MODE>
__global__ __launch_bounds__(256) void vm_refresh_kernel(const unsigned* __restrict__ dirty, int* __restrict__ ctl, const unsigned long long* __restrict__ keys,
                                                         const double* __restrict__ sums, uint4* __restrict__ table, int* __restrict__ num_voxels, int* __restrict__ occupied,
                                                         VmGrid* __restrict__ grid, unsigned long long* __restrict__ bitmap) {
  __shared__ int s_cnt, s_base;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int nd = ctl[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool is_new = false;
  unsigned b = 0;
  int local = 0;
  if (i < nd) {
    const unsigned d = dirty[i];
    b = d & ~VM_INC_NEW;
    is_new = (d & VM_INC_NEW) != 0u;
    const unsigned long long key = keys[b];
    double a[VM_ACC_STRIDE];
#pragma unroll
    for (int j = 0; j < VM_ACC_STRIDE; j++) a[j] = sums[(size_t)b * VM_ACC_STRIDE + j];
    inc_write_record<MODE>(key, a, table, b);
    if (is_new) {
      local = atomicAdd(&s_cnt, 1);
      if (grid && grid->enabled) {
        unsigned long long word;
        unsigned bit;
        if (vm_grid_locate(*grid, (unsigned)(key & 0x1FFFFF), (unsigned)((key >> 21) & 0x1FFFFF), (unsigned)((key >> 42) & 0x1FFFFF), word, bit)) atomicOr(&bitmap[word], 1ull << bit);
        else grid->enabled = 0;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(num_voxels, s_cnt) : 0;
  __syncthreads();
  if (is_new) occupied[s_base + local] = (int)b;
}

// what the next counter set starts from when the map moves to the other buffers: no voxels yet, the running `dropped` / skipped counts kept
__global__ void vm_rehash_begin_kernel(const int* __restrict__ cur_counters, int* __restrict__ next_counters, int* __restrict__ ctl) {
  if (threadIdx.x == 0) { next_counters[0] = 0; next_counters[1] = cur_counters[1]; next_counters[2] = cur_counters[2]; ctl[2] = 0; }
}

struct VmPrune {
  double center[3], radius, res;
  int by_distance;         // drop voxels whose centre (c + 1) * res is further than `radius` from `center`
  unsigned epoch, max_age;  // max_age > 0: drop voxels no insert has touched during the last max_age inserts
};
// One thread per bucket of the OLD table: a surviving bucket is claimed in the new keys (every key is unique: the claim is a creation),
// its sums and stamp move, its record is recomputed at the new index and it joins the new compact list. The only pass proportional to the map.
template <int MODE>
__global__ __launch_bounds__(VM_FIN_THREADS) void vm_rehash_kernel(const unsigned long long* __restrict__ old_keys, const double* __restrict__ old_sums, const unsigned* __restrict__ old_stamps,
                                                                   unsigned old_capacity, unsigned long long* __restrict__ new_keys, unsigned new_mask, double* __restrict__ new_sums,
                                                                   unsigned* __restrict__ new_stamps, uint4* __restrict__ table, int* __restrict__ counters, int* __restrict__ occupied,
                                                                   VmPrune prune, int* __restrict__ ctl) {
  // NDT (MODE 1): at the load factor <= 0.5 the host keeps, a wave of old buckets is at most half survivors, and each survivor's record
  // needs the MIN_EIG eigen-decomposition. As vm_finalize_kernel<1>: the workgroup's survivors are compacted through LDS (raw covariance,
  // weight, new bucket at the position the keep counter hands out) and regularised by the first ceil(count / 64) waves, one voxel per lane.
  // Rows of 7 doubles: lane t reads 8 bytes at 56 t -- the 32 lanes of a half wave fall on 32 distinct bank pairs.
  constexpr bool DENSE = (MODE == 1);
  __shared__ int s_keep, s_drop, s_base;
  __shared__ double s_cov[DENSE ? VM_FIN_THREADS : 1][7];
  __shared__ unsigned s_bucket[DENSE ? VM_FIN_THREADS : 1];
  if (threadIdx.x == 0) { s_keep = 0; s_drop = 0; }
  __syncthreads();
  const unsigned b = blockIdx.x * VM_FIN_THREADS + threadIdx.x;
  unsigned long long key = FVH_EMPTY_KEY;
  if (b < old_capacity) key = old_keys[b];
  bool keep = key != FVH_EMPTY_KEY;
  unsigned stamp = 0;
  if (keep) {
    stamp = old_stamps[b];
    if (prune.by_distance) {
      int cx, cy, cz;
      unpack_key(key, cx, cy, cz);
      const double dx = ((double)cx + 1.0) * prune.res - prune.center[0], dy = ((double)cy + 1.0) * prune.res - prune.center[1], dz = ((double)cz + 1.0) * prune.res - prune.center[2];
      if (sqrt(dx * dx + dy * dy + dz * dz) > prune.radius) keep = false;
    }
    if (prune.max_age > 0u && prune.epoch - stamp >= prune.max_age) keep = false;
    if (!keep) atomicAdd(&s_drop, 1);
  }
  unsigned nb = 0xFFFFFFFFu;
  int local = 0;
  if (keep) {
    nb = inc_claim(new_keys, new_mask, key);
    if (nb == 0xFFFFFFFFu) {
      atomicAdd(counters + 1, 1);  // (cannot happen: the host sizes the new table for every bucket of the old one)
    } else {
      double a[VM_ACC_STRIDE];
#pragma unroll
      for (int j = 0; j < VM_ACC_STRIDE; j++) { a[j] = old_sums[(size_t)b * VM_ACC_STRIDE + j]; new_sums[(size_t)nb * VM_ACC_STRIDE + j] = a[j]; }
      new_stamps[nb] = stamp;
      if constexpr (DENSE) {
        Sym3<double> C;
        double wn;
        inc_ndt_record_head(key, a, table, nb, C, wn);
        local = atomicAdd(&s_keep, 1);  // (< VM_FIN_THREADS: one survivor per thread at most)
        s_cov[local][0] = C.xx; s_cov[local][1] = C.xy; s_cov[local][2] = C.xz; s_cov[local][3] = C.yy; s_cov[local][4] = C.yz; s_cov[local][5] = C.zz; s_cov[local][6] = wn;
        s_bucket[local] = nb;
      } else {
        inc_write_record<MODE>(key, a, table, nb);
        local = atomicAdd(&s_keep, 1);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s_base = s_keep ? atomicAdd(counters, s_keep) : 0;
    if (s_drop) atomicAdd(ctl + 2, s_drop);
  }
  if constexpr (DENSE) {
    const int t = threadIdx.x;
    if (t < s_keep) inc_ndt_record_tail(Sym3<double>{s_cov[t][0], s_cov[t][1], s_cov[t][2], s_cov[t][3], s_cov[t][4], s_cov[t][5]}, s_cov[t][6], table, s_bucket[t]);
  }
  __syncthreads();
  if (nb != 0xFFFFFFFFu) occupied[s_base + local] = (int)nb;
}

// ---- snapshots of an incremental map (fvh_vgicp_voxelmap_export / _import / _merge_from: host_incmap.inc.hpp) --------------------
// A snapshot row is {coords[3], sums[10], age = epoch - stamp}. Both additive and multiplicative voxels are pure sums, so rows ADD into a
// live map on the same grid: vm_import_kernel (one thread per incoming row: claim, stamp) -> the existing vm_refresh_kernel (records,
// compact list, bitmap). The kernel needs no MODE: only the refresh turns sums into a record.
// The ten sums of a row are 80 contiguous bytes. A thread per row would give every wave instruction 64 segments of 8 bytes, 80 bytes
// apart -- the one-lane-per-row shape memory-side atomics are slowest at -- so the sums move in a second phase: the workgroup's 256 rows
// are 2,560 values, value e belongs to row e / 10, and ten neighbouring lanes cover one row's 80 bytes (the dense side is fully coalesced).
constexpr int VM_SNAP_THREADS = 256;

// FROM_MAP false: rows i < n_rows of a host snapshot (in_coords, in_sums, in_ages; in_ages may be null = all 0).
// FROM_MAP true : the compact list of ANOTHER live map, read in place: src_occupied[i < src_counters[0]] names the bucket whose key, sums
//                 (in_sums = that map's sums) and stamp are row i; age = src_epoch - stamp.
// A row's bucket is claimed (found or created), its stamp becomes max(old, epoch - age) -- never 0: the host refuses age >= epoch -- and
// the bucket joins the dirty list, marked new when the old stamp was 0. A key listed twice is listed twice in `dirty` (room: one entry
// per row), marked new once: the refresh then writes its record twice, from the same finished sums.
// With unique keys every sum receives exactly one add: old + incoming, to the bit.
template <bool FROM_MAP>
__global__ __launch_bounds__(VM_SNAP_THREADS) void vm_import_kernel(const int* __restrict__ in_coords, const double* __restrict__ in_sums, const unsigned* __restrict__ in_ages, int n_rows,
                                                                    const unsigned long long* __restrict__ src_keys, const int* __restrict__ src_occupied, const int* __restrict__ src_counters,
                                                                    const unsigned* __restrict__ src_stamps, unsigned src_epoch,
                                                                    unsigned long long* __restrict__ table_keys, unsigned mask, double* __restrict__ sums, unsigned* __restrict__ stamps,
                                                                    unsigned epoch, unsigned* __restrict__ dirty, int* __restrict__ ctl, int* __restrict__ dropped) {
  __shared__ unsigned s_dst[VM_SNAP_THREADS], s_src[VM_SNAP_THREADS];
  __shared__ int s_cnt, s_base;
  const int tid = threadIdx.x;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const int n = FROM_MAP ? min(src_counters[0], n_rows) : n_rows;  // (n_rows: what the host sized `dirty` and the grid for)
  const int base = blockIdx.x * VM_SNAP_THREADS;
  const int i = base + tid;
  unsigned b = 0xFFFFFFFFu, sb = 0u, entry = 0u;
  int local = -1;
  if (i < n) {
    unsigned long long key;
    unsigned age;
    if (FROM_MAP) {
      sb = (unsigned)src_occupied[i];
      key = src_keys[sb];
      age = src_epoch - src_stamps[sb];
    } else {
      sb = (unsigned)i;
      key = pack_key(in_coords[3 * (size_t)i], in_coords[3 * (size_t)i + 1], in_coords[3 * (size_t)i + 2]);
      age = in_ages ? in_ages[i] : 0u;
    }
    b = inc_claim(table_keys, mask, key);
    if (b != 0xFFFFFFFFu) {
      const unsigned was = atomicMax(stamps + b, epoch - age);
      entry = b | (was == 0u ? VM_INC_NEW : 0u);
      local = atomicAdd(&s_cnt, 1);
    } else {
      atomicAdd(dropped, 1);  // (cannot happen: the host secures a load factor <= 0.5 before the launch)
    }
  }
  s_dst[tid] = b;
  s_src[tid] = sb;
  __syncthreads();
  if (tid == 0) s_base = s_cnt ? atomicAdd(ctl, s_cnt) : 0;
  const int rows = min(VM_SNAP_THREADS, n - base);
  for (int e = tid; e < rows * VM_ACC_STRIDE; e += VM_SNAP_THREADS) {
    const int v = e / VM_ACC_STRIDE, j = e - v * VM_ACC_STRIDE;
    const unsigned db = s_dst[v];
    if (db == 0xFFFFFFFFu) continue;
    atomicAdd(&sums[(size_t)db * VM_ACC_STRIDE + j], in_sums[(size_t)s_src[v] * VM_ACC_STRIDE + j]);
  }
  __syncthreads();
  if (local >= 0) dirty[s_base + local] = entry;
}

// The compact list gathered into three dense arrays (rows in list order; the host sorts them by key): coords from the key, the ten sums,
// age = epoch - stamp. n_rows: the voxel count the host read and sized the arrays for.
__global__ __launch_bounds__(VM_SNAP_THREADS) void vm_export_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ sums, const unsigned* __restrict__ stamps,
                                                                    const int* __restrict__ occupied, const int* __restrict__ counters, unsigned epoch, int n_rows,
                                                                    int* __restrict__ out_coords, double* __restrict__ out_sums, unsigned* __restrict__ out_ages) {
  __shared__ unsigned s_src[VM_SNAP_THREADS];
  const int tid = threadIdx.x;
  const int n = min(counters[0], n_rows);
  const int base = blockIdx.x * VM_SNAP_THREADS;
  const int i = base + tid;
  if (i < n) {
    const unsigned b = (unsigned)occupied[i];
    int cx, cy, cz;
    unpack_key(keys[b], cx, cy, cz);
    out_coords[3 * (size_t)i] = cx; out_coords[3 * (size_t)i + 1] = cy; out_coords[3 * (size_t)i + 2] = cz;
    out_ages[i] = epoch - stamps[b];
    s_src[tid] = b;
  }
  __syncthreads();
  const int rows = min(VM_SNAP_THREADS, n - base);
  for (int e = tid; e < rows * VM_ACC_STRIDE; e += VM_SNAP_THREADS) {
    const int v = e / VM_ACC_STRIDE, j = e - v * VM_ACC_STRIDE;
    out_sums[(size_t)base * VM_ACC_STRIDE + e] = sums[(size_t)s_src[v] * VM_ACC_STRIDE + j];
  }
}

// ---- a live map added under a rigid pose (fvh_*_posed_merge_from / fvh_*_transform_map: host_incmap.inc.hpp) ------------
// The voxel sums transform in closed form under x -> R x + t (n = the count, sp / b the first three sums, the six others a symmetric matrix):
//   MODE 0 additive       : sp' = R sp + n t             SC' = R SC R^T
//   MODE 2 multiplicative : A'  = R A R^T                b'  = R b + A' t
//   MODE 1 NDT, u = R sp  : sp' = u + n t                S'  = R S R^T + u t^T + t u^T + n t t^T
// all in fp64, each expression in the order tests/posedmerge_ref.py restates. A row goes to the voxel of the float32 mean its transformed
// sums have ON THEIR OWN -- the record arithmetic, taken from inc_write_record<MODE> / inc_ndt_record_head themselves by handing them a
// four-quad record in registers -- binned as vm_insert_kernel bins a point. This re-bins voxel Gaussians, not points: several rows may
// meet in one voxel (their sums add), and a row whose mean leaves the key range is skipped and counted (rows in ctl[1], its points in
// dropped[1], where an insert counts skipped points).
// Rows are the compact list of a live map read in place, as vm_import_kernel<true> reads one: another handle's map (merge), or this map's
// own current buffers on their way into the other set (transform: keys are no longer unique afterwards, so the pass ADDS where
// vm_rehash_kernel moves). Shaped like vm_import_kernel for the same reason: the workgroup's 256 x 10 sums come into LDS (20 KB) with ten
// neighbouring lanes per row, one thread per row transforms its row out of LDS and back (80-byte rows: a half wave's 8-byte reads fall
// two to a bank pair), and the adds leave in the coalesced second phase.
template <int MODE>
__device__ __forceinline__ void vm_posed_sums(const PoseD& T, const double* a, double* o) {
  const double* R = T.r;
  const double* t = T.t;
  const double n = a[9];
  const double S[3][3] = {{a[3], a[4], a[5]}, {a[4], a[6], a[7]}, {a[5], a[7], a[8]}};
  double u[3], M[3][3], Q[3][3];  // R sp, R S, R S R^T
#pragma unroll
  for (int r = 0; r < 3; r++) {
    u[r] = R[3 * r] * a[0] + R[3 * r + 1] * a[1] + R[3 * r + 2] * a[2];
#pragma unroll
    for (int c = 0; c < 3; c++) M[r][c] = R[3 * r] * S[0][c] + R[3 * r + 1] * S[1][c] + R[3 * r + 2] * S[2][c];
  }
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = r; c < 3; c++) Q[r][c] = M[r][0] * R[3 * c] + M[r][1] * R[3 * c + 1] + M[r][2] * R[3 * c + 2];
  Q[1][0] = Q[0][1]; Q[2][0] = Q[0][2]; Q[2][1] = Q[1][2];
  if (MODE == 2) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = u[r] + Q[r][0] * t[0] + Q[r][1] * t[1] + Q[r][2] * t[2];
  } else {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = u[r] + n * t[r];
  }
  if (MODE == 1) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = r; c < 3; c++) Q[r][c] = Q[r][c] + u[r] * t[c] + t[r] * u[c] + (n * t[r]) * t[c];
  }
  o[3] = Q[0][0]; o[4] = Q[0][1]; o[5] = Q[0][2]; o[6] = Q[1][1]; o[7] = Q[1][2]; o[8] = Q[2][2];
  o[9] = n;
}

template <int MODE>
__global__ __launch_bounds__(VM_SNAP_THREADS) void vm_import_posed_kernel(const unsigned long long* __restrict__ src_keys, const double* __restrict__ src_sums, const unsigned* __restrict__ src_stamps,
                                                                          const int* __restrict__ src_occupied, const int* __restrict__ src_counters, int n_rows, unsigned src_epoch, PoseD T,
                                                                          double res, unsigned long long* __restrict__ table_keys, unsigned mask, double* __restrict__ sums,
                                                                          unsigned* __restrict__ stamps, unsigned epoch, unsigned* __restrict__ dirty, int* __restrict__ ctl,
                                                                          int* __restrict__ dropped) {
  __shared__ double s_val[VM_SNAP_THREADS * VM_ACC_STRIDE];
  __shared__ unsigned s_dst[VM_SNAP_THREADS], s_src[VM_SNAP_THREADS];
  __shared__ int s_cnt, s_base;
  const int tid = threadIdx.x;
  if (tid == 0) s_cnt = 0;
  const int n = min(src_counters[0], n_rows);  // (n_rows: what the host sized `dirty` and the grid for)
  const int base = blockIdx.x * VM_SNAP_THREADS;
  const int i = base + tid;
  unsigned age = 0u;
  if (i < n) {
    const unsigned sb = (unsigned)src_occupied[i];
    age = src_epoch - src_stamps[sb];
    s_src[tid] = sb;
  }
  __syncthreads();
  const int rows = min(VM_SNAP_THREADS, n - base);
  for (int e = tid; e < rows * VM_ACC_STRIDE; e += VM_SNAP_THREADS) {
    const int v = e / VM_ACC_STRIDE, j = e - v * VM_ACC_STRIDE;
    s_val[e] = src_sums[(size_t)s_src[v] * VM_ACC_STRIDE + j];
  }
  __syncthreads();
  unsigned b = 0xFFFFFFFFu, entry = 0u;
  int local = -1;
  if (i < n) {
    double a[VM_ACC_STRIDE], o[VM_ACC_STRIDE];
#pragma unroll
    for (int j = 0; j < VM_ACC_STRIDE; j++) a[j] = s_val[tid * VM_ACC_STRIDE + j];
    vm_posed_sums<MODE>(T, a, o);
    float4 rec[4];  // the record the transformed sums would get, in registers: only its mean (quad 1, which the record functions store as a float4) is used
    if constexpr (MODE == 1) {
      Sym3<double> Craw;
      double wn;
      inc_ndt_record_head(0ull, o, reinterpret_cast<uint4*>(rec), 0u, Craw, wn);
    } else {
      inc_write_record<MODE>(0ull, o, reinterpret_cast<uint4*>(rec), 0u);
    }
    const float mx = rec[1].x, my = rec[1].y, mz = rec[1].z;
    const double fx = floor((double)mx / res - 0.5), fy = floor((double)my / res - 0.5), fz = floor((double)mz / res - 0.5);
    if (!voxel_index_ok(fx, fy, fz)) {
      atomicAdd(ctl + 1, 1);
      atomicAdd(dropped + 1, (int)a[9]);
    } else {
      b = inc_claim(table_keys, mask, pack_key((int)fx, (int)fy, (int)fz));
      if (b != 0xFFFFFFFFu) {
        const unsigned was = atomicMax(stamps + b, epoch - age);
        entry = b | (was == 0u ? VM_INC_NEW : 0u);
        local = atomicAdd(&s_cnt, 1);
#pragma unroll
        for (int j = 0; j < VM_ACC_STRIDE; j++) s_val[tid * VM_ACC_STRIDE + j] = o[j];
      } else {
        atomicAdd(dropped, 1);  // (cannot happen: the host secures a load factor <= 0.5 before the launch)
      }
    }
  }
  s_dst[tid] = b;
  __syncthreads();
  if (tid == 0) s_base = s_cnt ? atomicAdd(ctl, s_cnt) : 0;
  for (int e = tid; e < rows * VM_ACC_STRIDE; e += VM_SNAP_THREADS) {
    const int v = e / VM_ACC_STRIDE;
    const unsigned db = s_dst[v];
    if (db == 0xFFFFFFFFu) continue;
    atomicAdd(&sums[(size_t)db * VM_ACC_STRIDE + (e - v * VM_ACC_STRIDE)], s_val[e]);
  }
  __syncthreads();
  if (local >= 0) dirty[s_base + local] = entry;
}

// ---- the live incremental map as a point target (fvh_vgicp_target_from_map / fvh_ndt_target_from_map: host_incmap.inc.hpp) --------
// One point per voxel (the record's float mean; VGICP: + the record's covariance), rows in ascending packed-key order, written where a
// target cloud lives -- so the exact 1-NN search, the fitness score and the FastGICP cost run on the map unchanged. Three steps:
//   select : the compact list -> (key, bucket) of the voxels with >= min_points points, in whatever order the workgroups arrive (the sort
//            below makes the rows deterministic: keys are unique), their count and the bounds of their biased coordinates
//   keys   : the 32-bit words radix_sort_pairs (host_downsample.inc.hpp) sorts by: the key compressed against those bounds when the box
//            fits 32 bits -- one sweep over exactly the bits the box needs --, else the key's low word, then, re-gathered through the
//            first sweep's order, its high word (two stable sweeps = one 63-bit sort)
//   gather : row r <- the record of the r-th bucket in key order
struct VmTargetCtl { int selected, num_voxels; unsigned umin[3], umax[3]; };
__global__ void vm_target_begin_kernel(VmTargetCtl* __restrict__ ctl) {
  if (threadIdx.x < 3) { ctl->umin[threadIdx.x] = 0xFFFFFFFFu; ctl->umax[threadIdx.x] = 0u; }
  if (threadIdx.x == 0) { ctl->selected = 0; ctl->num_voxels = 0; }
}

// Workgroups of VM_FIN_THREADS walk the list grid-stride: one counter atomic per 1,024 voxels hands out the output range, and the bounds
// stay in registers until the end -- six atomics per WORKGROUP, on a grid capped at VM_TARGET_MAX_WGS (same-address atomics retire one
// after the other at the memory side: vm_finalize_kernel's note). n_bound: what the host sized sel_keys / sel_buckets for.
constexpr int VM_TARGET_MAX_WGS = 64;
__global__ __launch_bounds__(VM_FIN_THREADS) void vm_target_select_kernel(const uint4* __restrict__ table, const int* __restrict__ occupied, const int* __restrict__ counters, int n_bound,
                                                                          int min_points, unsigned long long* __restrict__ sel_keys, unsigned* __restrict__ sel_buckets,
                                                                          VmTargetCtl* __restrict__ ctl) {
  __shared__ int s_wave_cnt[VM_FIN_THREADS / 64], s_base;
  __shared__ unsigned s_min[3], s_max[3];
  if (threadIdx.x < 3) { s_min[threadIdx.x] = 0xFFFFFFFFu; s_max[threadIdx.x] = 0u; }
  const int nv = min(counters[0], n_bound);
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->num_voxels = counters[0];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  for (int base = blockIdx.x * VM_FIN_THREADS; base < nv; base += gridDim.x * VM_FIN_THREADS) {  // (uniform per workgroup: the barriers are safe)
    const int i = base + (int)threadIdx.x;
    bool pass = false;
    unsigned b = 0;
    unsigned long long key = 0;
    if (i < nv) {
      b = (unsigned)occupied[i];
      const uint4 q0 = table[(size_t)b * 4];  // {key_lo, key_hi, num_points, 0}
      key = (unsigned long long)q0.x | ((unsigned long long)q0.y << 32);
      pass = (int)q0.z >= min_points;
    }
    const unsigned long long mask = __ballot(pass);
    const int slot_in_wave = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_cnt[wv] = __popcll(mask);
    __syncthreads();
    int total = 0, local = slot_in_wave;
    for (int w = 0; w < VM_FIN_THREADS / 64; w++) { const int c = s_wave_cnt[w]; total += c; local += (w < wv) ? c : 0; }
    if (threadIdx.x == 0) s_base = total ? atomicAdd(&ctl->selected, total) : 0;
    __syncthreads();
    if (pass) {
      const int r = s_base + local;  // (< nv <= n_bound: every selected voxel takes one slot)
      sel_keys[r] = key;
      sel_buckets[r] = b;
      const unsigned c[3] = {(unsigned)(key & 0x1FFFFF), (unsigned)((key >> 21) & 0x1FFFFF), (unsigned)((key >> 42) & 0x1FFFFF)};
#pragma unroll
      for (int a = 0; a < 3; a++) { mn[a] = min(mn[a], c[a]); mx[a] = max(mx[a], c[a]); }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    for (int o = 32; o >= 1; o >>= 1) { mn[a] = min(mn[a], (unsigned)__shfl_xor((int)mn[a], o)); mx[a] = max(mx[a], (unsigned)__shfl_xor((int)mx[a], o)); }
  }
  __syncthreads();  // (s_min / s_max initialised: a workgroup with no chunk never met a barrier above)
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { atomicMin(&s_min[a], mn[a]); atomicMax(&s_max[a], mx[a]); }
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_min[threadIdx.x] != 0xFFFFFFFFu) { atomicMin(&ctl->umin[threadIdx.x], s_min[threadIdx.x]); atomicMax(&ctl->umax[threadIdx.x], s_max[threadIdx.x]); }
}

// part 0: the key compressed against the box of the selected voxels, z-major like pack_key: (z - lo_z) << bxy | (y - lo_y) << bx | (x - lo_x)
// part 1: the key's low word; part 2: its high word. idx_in null: the identity (rows of the select pass); part 2 runs in place over the
// first sweep's result (idx_out == idx_in: every thread rewrites the element it read).
struct VmTargetKey { unsigned lo[3]; int bx, bxy, part; };
__global__ __launch_bounds__(256) void vm_target_keys_kernel(const unsigned long long* __restrict__ sel_keys, const int* idx_in, int m, VmTargetKey kp, unsigned* __restrict__ keys_out,
                                                             int* idx_out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const int src = idx_in ? idx_in[r] : r;
  const unsigned long long k = sel_keys[src];
  unsigned v;
  if (kp.part == 0) {
    const unsigned long long dx = (unsigned)(k & 0x1FFFFF) - kp.lo[0], dy = (unsigned)((k >> 21) & 0x1FFFFF) - kp.lo[1], dz = (unsigned)((k >> 42) & 0x1FFFFF) - kp.lo[2];
    v = (unsigned)(dx | (dy << kp.bx) | (dz << kp.bxy));  // (64-bit shifts: bxy may be 32 when the box is one voxel thick in z -- dz is 0 then)
  } else {
    v = kp.part == 1 ? (unsigned)k : (unsigned)(k >> 32);
  }
  keys_out[r] = v;
  idx_out[r] = src;
}

// Row r <- the record of bucket sel_buckets[order[r]]: the point {mean, 0} as pack_points_kernel writes one, the covariance in the cloud's
// layout {xx, xy, xz, yy | yz, zz, 0, 0} -- the record's q2 and q3.xy (q3.zw of a record is the weight sqrt(n), not covariance). Moves only:
// every float arrives bit for bit. out_cov null: points only (NDT handles).
__global__ __launch_bounds__(256) void vm_target_gather_kernel(const float4* __restrict__ table, const unsigned* __restrict__ sel_buckets, const int* __restrict__ order, int m,
                                                               float4* __restrict__ out_pts, float4* __restrict__ out_cov) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const size_t b = sel_buckets[order[r]];
  const float4 q1 = table[b * 4 + 1];
  out_pts[r] = make_float4(q1.x, q1.y, q1.z, 0.f);
  if (out_cov) {
    const float4 q3 = table[b * 4 + 3];
    out_cov[2 * (size_t)r] = table[b * 4 + 2];
    out_cov[2 * (size_t)r + 1] = make_float4(q3.x, q3.y, 0.f, 0.f);
  }
}

// ---- free space cleared along the rays of a posed scan (fvh_*_clear_rays_*: host_incmap.inc.hpp, incmap_clear_rays) -----------
// The ray from the sensor origin to a measured point proves the voxels it crosses empty. Two kernels and the existing rehash:
//   marks : capacity x u32 parallel to the buckets, zeroed per call: bits 0..30 count the rays of THIS call that crossed the voxel (an
//           integer: the order of the adds does not matter), bit 31 says a ray of this call ended in it.
//   vm_raymark  one ray per lane: the endpoint's voxel gets bit 31, an Amanatides-Woo walk in fp64 (the contract, operation by operation,
//               is in include/fast_vgicp_hip.h; tests/clearrays_ref.py restates it) adds 1 to every crossed voxel that exists. The map is
//               only read: a probe by hash_slot and linear probing to the key or an empty slot.
//   vm_raysweep one thread per entry of the compact list: a voxel with >= min_misses crossings and no hit is condemned -- its stamp
//               becomes 0, the value of a bucket nothing ever touched, which no live voxel holds -- and counted in ctl[3].
// vm_rehash_kernel with max_age = epoch then drops exactly the buckets whose stamp is 0 (epoch - stamp >= epoch); it is launched only
// when ctl[3] > 0, so a call that removes nothing writes nothing to the map.
// ctl here: {-, rays used, (the rehash's removed count), voxels condemned}
constexpr unsigned VM_RAY_HIT = 0x80000000u;
constexpr int VM_RAY_MAX_STEPS = 3 * 4097;  // what max_range <= 4096 voxels (the host's rule) allows |dc_x| + |dc_y| + |dc_z| to be

struct VmRays {
  PoseD T;          // scan frame -> map frame
  float origin[3];  // o' = (float)(R o + t), formed by the host
  double res, min_range, max_range, end_margin;
};

__device__ __forceinline__ double ray_range_nofma(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  return __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
}

// read-only lookup: the bucket of `key`, 0xFFFFFFFF when the map has no such voxel
__device__ __forceinline__ unsigned vm_find_bucket(const unsigned long long* __restrict__ keys, unsigned mask, unsigned long long key) {
  unsigned slot = hash_slot(key, mask);
  for (unsigned it = 0; it <= mask; it++) {
    const unsigned long long k = keys[slot];
    if (k == key) return slot;
    if (k == FVH_EMPTY_KEY) break;
    slot = (slot + 1) & mask;
  }
  return 0xFFFFFFFFu;
}
// ... of cell (cx, cy, cz). A live bitmap answers for the cells that do not exist (every voxel of the map lies inside its box while it is
// enabled: vm_refresh_kernel), so the result is the same with and without it.
__device__ __forceinline__ unsigned ray_cell_bucket(int cx, int cy, int cz, const unsigned long long* __restrict__ keys, unsigned mask, bool use_grid, const VmGrid& g,
                                                    const unsigned long long* __restrict__ bitmap) {
  if (!coord_in_range(cx, cy, cz)) return 0xFFFFFFFFu;
  if (use_grid) {
    unsigned long long word;
    unsigned bit;
    if (!vm_grid_locate(g, (unsigned)(cx + FVH_COORD_BIAS), (unsigned)(cy + FVH_COORD_BIAS), (unsigned)(cz + FVH_COORD_BIAS), word, bit)) return 0xFFFFFFFFu;
    if (!((bitmap[word] >> bit) & 1ull)) return 0xFFFFFFFFu;
  }
  return vm_find_bucket(keys, mask, pack_key(cx, cy, cz));
}

// One ray per lane; trip counts diverge inside a wave, which is why the host hands the source's Morton order in when it has one
// (neighbouring lanes then walk rays of similar length through neighbouring cells). p' is formed by the expression vm_insert_kernel bins.
__global__ __launch_bounds__(256) void vm_raymark_kernel(const float4* __restrict__ pts, int n, const int* __restrict__ order, VmRays ry, const unsigned long long* __restrict__ keys,
                                                         unsigned mask, unsigned* __restrict__ marks, const VmGrid* __restrict__ grid, const unsigned long long* __restrict__ bitmap,
                                                         int* __restrict__ ctl) {
  __shared__ int s_used;
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  const bool use_grid = grid != nullptr && grid->enabled != 0;
  VmGrid g = {};
  if (use_grid) g = *grid;
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  if (i0 < n) {
    const int i = order ? order[i0] : i0;
    const float4 p = pts[i];
    const PoseD& T = ry.T;
    const double res = ry.res;
    const double x = p.x, y = p.y, z = p.z;
    const float px = (float)(T.r[0] * x + T.r[1] * y + T.r[2] * z + T.t[0]);
    const float py = (float)(T.r[3] * x + T.r[4] * y + T.r[5] * z + T.t[1]);
    const float pz = (float)(T.r[6] * x + T.r[7] * y + T.r[8] * z + T.t[2]);
    const double ax = (double)ry.origin[0] / res - 0.5, ay = (double)ry.origin[1] / res - 0.5, az = (double)ry.origin[2] / res - 0.5;
    const double bx = (double)px / res - 0.5, by = (double)py / res - 0.5, bz = (double)pz / res - 0.5;
    const double fax = floor(ax), fay = floor(ay), faz = floor(az), fbx = floor(bx), fby = floor(by), fbz = floor(bz);
    const double r = ray_range_nofma((double)px - (double)ry.origin[0], (double)py - (double)ry.origin[1], (double)pz - (double)ry.origin[2]);
    const bool finite_in = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    if (finite_in && !(r == 0.0) && !(r < ry.min_range) && !(r > ry.max_range) && voxel_index_ok(fax, fay, faz) && voxel_index_ok(fbx, fby, fbz)) {
      atomicAdd(&s_used, 1);
      int cx = (int)fax, cy = (int)fay, cz = (int)faz;
      const int ex = (int)fbx, ey = (int)fby, ez = (int)fbz;
      const unsigned hb = ray_cell_bucket(ex, ey, ez, keys, mask, use_grid, g, bitmap);
      if (hb != 0xFFFFFFFFu) atomicOr(marks + hb, VM_RAY_HIT);
      const double dx = bx - ax, dy = by - ay, dz = bz - az;
      const int sx = dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0), sy = dy > 0.0 ? 1 : (dy < 0.0 ? -1 : 0), sz = dz > 0.0 ? 1 : (dz < 0.0 ? -1 : 0);
      const double tdx = 1.0 / fabs(dx), tdy = 1.0 / fabs(dy), tdz = 1.0 / fabs(dz);
      const double inf = __longlong_as_double(0x7FF0000000000000ll);
      double tmx = dx > 0.0 ? ((double)(cx + 1) - ax) / dx : (dx < 0.0 ? (ax - (double)cx) / (-dx) : inf);
      double tmy = dy > 0.0 ? ((double)(cy + 1) - ay) / dy : (dy < 0.0 ? (ay - (double)cy) / (-dy) : inf);
      double tmz = dz > 0.0 ? ((double)(cz + 1) - az) / dz : (dz < 0.0 ? (az - (double)cz) / (-dz) : inf);
      const double t_end = 1.0 - ry.end_margin / r;
      const int nsteps = min(abs(ex - cx) + abs(ey - cy) + abs(ez - cz), VM_RAY_MAX_STEPS);
      double t_in = 0.0;
#pragma unroll 1
      for (int step = 0; t_in < t_end; step++) {
        const unsigned b = ray_cell_bucket(cx, cy, cz, keys, mask, use_grid, g, bitmap);
        if (b != 0xFFFFFFFFu) atomicAdd(marks + b, 1u);  // (result unused: a no-return atomic)
        if (step == nsteps) break;
        if (tmx <= tmy && tmx <= tmz) { t_in = tmx; cx += sx; tmx += tdx; }       // ties: x before y before z
        else if (tmy <= tmz) { t_in = tmy; cy += sy; tmy += tdy; }
        else { t_in = tmz; cz += sz; tmz += tdz; }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_used) atomicAdd(ctl + 1, s_used);
}

// n_bound: the voxel count the host sized the grid for (its bound; the count itself is read here)
__global__ __launch_bounds__(256) void vm_raysweep_kernel(const int* __restrict__ occupied, const int* __restrict__ counters, int n_bound, const unsigned* __restrict__ marks,
                                                          unsigned min_misses, unsigned* __restrict__ stamps, int* __restrict__ ctl) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int n = min(counters[0], n_bound);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const unsigned b = (unsigned)occupied[i];
    const unsigned m = marks[b];
    if (!(m & VM_RAY_HIT) && m >= min_misses) {  // (no hit bit: m is the count)
      stamps[b] = 0u;
      atomicAdd(&s_cnt, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(ctl + 3, s_cnt);
}

}  // namespace fvh
