// A posed scan scored against the target voxel map, per point (fvh_*_score_source / _score_cloud: host_incmap.inc.hpp, map_score_run).
// How well does the map explain the scan at this pose: for every point the voxels around it (DIRECT1 / 7 / 27, the order of
// Engine::set_offsets) are looked up, the squared Mahalanobis distance to each voxel's Gaussian is formed in fp64, and the point keeps the
// number of voxels found, the best of them and its distance. The contract, operation by operation, is in include/fast_vgicp_hip.h;
// tests/mapscore_ref.py restates it.
//   vm_score    one point per lane, read-only on the map. The hash slots of all offsets are computed first and their key loads issued as ONE
//               batch (most DIRECT27 probes miss: they touch the dense key array only -- kernels_voxelmap.hpp, "HBM layout"); a first key
//               that is neither the voxel's nor EMPTY goes on by linear probing under vm_find_bucket's rule; the 64-byte record is loaded
//               for hits only. A live occupancy bitmap answers for absent cells first, as in ray_cell_bucket. The counts are integers
//               (LDS, then one atomic per workgroup and counter); the three fp64 terms of a point go to scratch AT ITS INPUT INDEX.
//   vm_score_sum  the terms summed in an order that depends on n alone: chunks of VM_SCORE_CHUNK entries, one workgroup each (thread t: entries
//               t, t + 1024, ... of the chunk in four interleaved partial sums, then a fixed tree -- fitness_reduce_kernel's), then the chunk
//               sums the same way. Neither the walk order of vm_score nor its grid reaches the sums. No floating-point atomics anywhere.
#pragma once
#include "kernels_voxelmap.hpp"

namespace fvh {

constexpr int VM_SCORE_CHUNK = 16384;

// the device image of fvh_map_score (include/fast_vgicp_hip.h): read back as it stands
struct VmScoreOut {
  int n_points, n_used, n_in_voxel, n_near, n_explained, pad_;
  double sum_best_m2, sum_score_max, sum_score_all;
};

struct VmScore {
  PoseD T;  // scan frame -> map frame
  double res, max_m2, score_scale;
  int min_points;
};

template <int NOFF>
__device__ __forceinline__ void score_offset(int o, int& dx, int& dy, int& dz) {
  static_assert(NOFF == 1 || NOFF == 7 || NOFF == 27, "DIRECT1, DIRECT7 or DIRECT27");
  if (NOFF == 1) { dx = dy = dz = 0; }
  else if (NOFF == 7) { dx = o == 1 ? 1 : (o == 2 ? -1 : 0); dy = o == 3 ? 1 : (o == 4 ? -1 : 0); dz = o == 5 ? 1 : (o == 6 ? -1 : 0); }
  else { dx = o / 9 - 1; dy = (o / 3) % 3 - 1; dz = o % 3 - 1; }
}

// squared Mahalanobis distance of d under the covariance {cxx .. czz} through the adjugate, every product and sum its own rounding;
// +inf for a record that is not positive (det <= 0) or not finite
__device__ __forceinline__ double score_m2_nofma(double dx, double dy, double dz, double cxx, double cxy, double cxz, double cyy, double cyz, double czz) {
#pragma clang fp contract(off)
  const double a00 = cyy * czz - cyz * cyz, a01 = cxz * cyz - cxy * czz, a02 = cxy * cyz - cxz * cyy;
  const double a11 = cxx * czz - cxz * cxz, a12 = cxy * cxz - cxx * cyz, a22 = cxx * cyy - cxy * cxy;
  const double det = (cxx * a00 + cxy * a01) + cxz * a02;
  const double q = (((dx * dx) * a00 + (dy * dy) * a11) + (dz * dz) * a22) + 2.0 * ((((dx * dy) * a01) + ((dx * dz) * a02)) + ((dy * dz) * a12));
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  if (!(det > 0.0) || !isfinite(det) || !isfinite(q)) return inf;
  const double m2 = q / det;
  return m2 < 0.0 ? 0.0 : m2;
}
// exp(-0.5 * score_scale * m2), the products from the left; 0 for m2 = +inf
__device__ __forceinline__ double score_exp_nofma(double score_scale, double m2) {
#pragma clang fp contract(off)
  if (!(m2 < __longlong_as_double(0x7FF0000000000000ll))) return 0.0;
  return exp((-0.5 * score_scale) * m2);
}

// terms: 3 x n doubles {best m2 of an explained point | exp of the best m2 of a near point | sum of the exps of a used point}, 0 otherwise.
// found / best / best_m2 (n each, input order) may be null. out: zeroed by the host; n_points is written here -- n, or -1 when the map's
// own overflow counter is set (a hint-sized batch table that dropped points: the host rebuilds it and asks again).
template <int NOFF>
__global__ __launch_bounds__(256) void vm_score_kernel(const float* __restrict__ xyz, int stride, int n, const int* __restrict__ order, VmScore sp, const unsigned long long* __restrict__ keys,
                                                       unsigned mask, const uint4* __restrict__ table, const VmGrid* __restrict__ grid, const unsigned long long* __restrict__ bitmap,
                                                       const int* __restrict__ map_counters, double* __restrict__ terms, int* __restrict__ found_out, int* __restrict__ best_out,
                                                       double* __restrict__ best_m2_out, VmScoreOut* __restrict__ out) {
  __shared__ int s_cnt[4];  // used, in own voxel, near, explained
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) out->n_points = map_counters[1] != 0 ? -1 : n;
  const bool use_grid = grid != nullptr && grid->enabled != 0;
  VmGrid g = {};
  if (use_grid) g = *grid;
  constexpr int OWN = NOFF == 27 ? 13 : 0;  // where (0, 0, 0) stands in the offset order
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  if (i0 < n) {
    const int i = order ? order[i0] : i0;
    const float* pp = xyz + (size_t)i * stride;
    const float sx = pp[0], sy = pp[1], sz = pp[2];
    // p' = (float)(R p + t): dev_math.hpp's transform(), the expression vm_insert_kernel and vm_raymark_kernel spell out
    const Vec3<double> q = transform(pose_cast<double>(sp.T), Vec3<double>{(double)sx, (double)sy, (double)sz});
    const float px = (float)q.x, py = (float)q.y, pz = (float)q.z;
    const double fx = floor((double)px / sp.res - 0.5), fy = floor((double)py / sp.res - 0.5), fz = floor((double)pz / sp.res - 0.5);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    int found = -1, best = -1;
    double best_m2 = __longlong_as_double(0x7FF8000000000000ll);
    double t_m2 = 0.0, t_max = 0.0, t_all = 0.0;
    if (isfinite(sx) && isfinite(sy) && isfinite(sz) && voxel_index_ok(fx, fy, fz)) {
      const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
      unsigned slot[NOFF];  // 0xFFFFFFFF: a cell no voxel can have, or one the bitmap says is absent
      unsigned long long first[NOFF];
      // 1. the cells and their hash slots; with a live bitmap the words of all cells are loaded as one batch too
      //    (the bitmap holds at most 2^31 words -- fvh_engine_params::bitmap_max_bytes <= 16 GiB --, so a word index fits 32 bits)
      if (use_grid) {
        unsigned widx[NOFF];
        unsigned long long w[NOFF];
#pragma unroll
        for (int o = 0; o < NOFF; o++) {
          int dx, dy, dz;
          score_offset<NOFF>(o, dx, dy, dz);
          const int vx = cx + dx, vy = cy + dy, vz = cz + dz;
          unsigned long long word = 0ull;
          unsigned bit = 0u;
          const bool ok = coord_in_range(vx, vy, vz) &&
                          vm_grid_locate(g, (unsigned)(vx + FVH_COORD_BIAS), (unsigned)(vy + FVH_COORD_BIAS), (unsigned)(vz + FVH_COORD_BIAS), word, bit);
          widx[o] = ok ? (unsigned)word : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int o = 0; o < NOFF; o++) w[o] = widx[o] != 0xFFFFFFFFu ? bitmap[widx[o]] : 0ull;
#pragma unroll
        for (int o = 0; o < NOFF; o++) {
          int dx, dy, dz;
          score_offset<NOFF>(o, dx, dy, dz);
          const unsigned ux = (unsigned)(cx + dx + FVH_COORD_BIAS), uy = (unsigned)(cy + dy + FVH_COORD_BIAS), uz = (unsigned)(cz + dz + FVH_COORD_BIAS);
          const unsigned bit = (ux & 3u) | ((uy & 3u) << 2) | ((uz & 3u) << 4);  // (vm_grid_locate's bit)
          slot[o] = ((w[o] >> bit) & 1ull) ? hash_slot(pack_key(cx + dx, cy + dy, cz + dz), mask) : 0xFFFFFFFFu;
        }
      } else {
#pragma unroll
        for (int o = 0; o < NOFF; o++) {
          int dx, dy, dz;
          score_offset<NOFF>(o, dx, dy, dz);
          const int vx = cx + dx, vy = cy + dy, vz = cz + dz;
          slot[o] = coord_in_range(vx, vy, vz) ? hash_slot(pack_key(vx, vy, vz), mask) : 0xFFFFFFFFu;
        }
      }
      // 2. the first key of every probe sequence, in one batch
#pragma unroll
      for (int o = 0; o < NOFF; o++) first[o] = slot[o] != 0xFFFFFFFFu ? keys[slot[o]] : FVH_EMPTY_KEY;
      // 3. collisions go on as vm_find_bucket does; records for hits only
      found = 0;
      best_m2 = inf;
      bool own = false;
#pragma unroll
      for (int o = 0; o < NOFF; o++) {
        if (first[o] == FVH_EMPTY_KEY) continue;
        int dx, dy, dz;
        score_offset<NOFF>(o, dx, dy, dz);
        const unsigned long long key = pack_key(cx + dx, cy + dy, cz + dz);
        unsigned b = slot[o];
        if (first[o] != key) {
          b = 0xFFFFFFFFu;
          unsigned s = (slot[o] + 1) & mask;
          for (unsigned it = 1; it <= mask; it++) {
            const unsigned long long k = keys[s];
            if (k == key) { b = s; break; }
            if (k == FVH_EMPTY_KEY) break;
            s = (s + 1) & mask;
          }
          if (b == 0xFFFFFFFFu) continue;
        }
        const float4* tf = reinterpret_cast<const float4*>(table);  // the whole 64-byte record in one go
        const uint4 q0 = table[(size_t)b * 4];
        const float4 q1 = tf[(size_t)b * 4 + 1], q2 = tf[(size_t)b * 4 + 2], q3 = tf[(size_t)b * 4 + 3];
        if (sp.min_points > 1 && (int)q0.z < sp.min_points) continue;
        const double m2 = score_m2_nofma((double)px - (double)q1.x, (double)py - (double)q1.y, (double)pz - (double)q1.z, (double)q2.x, (double)q2.y, (double)q2.z, (double)q2.w,
                                         (double)q3.x, (double)q3.y);
        found++;
        if (o == OWN) own = true;
        if (best < 0 || m2 < best_m2) { best = o; best_m2 = m2; }  // (ties: the first in offset order stays)
        t_all += score_exp_nofma(sp.score_scale, m2);
      }
      atomicAdd(&s_cnt[0], 1);
      if (own) atomicAdd(&s_cnt[1], 1);
      if (found > 0) {
        atomicAdd(&s_cnt[2], 1);
        t_max = score_exp_nofma(sp.score_scale, best_m2);
        if (best_m2 < inf && best_m2 <= sp.max_m2) { atomicAdd(&s_cnt[3], 1); t_m2 = best_m2; }  // (+inf explains nothing, whatever max_m2 is)
      }
    }
    terms[i] = t_m2;
    terms[(size_t)n + i] = t_max;
    terms[2 * (size_t)n + i] = t_all;
    if (found_out) found_out[i] = found;
    if (best_out) best_out[i] = best;
    if (best_m2_out) best_m2_out[i] = best_m2;
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&out->n_used + threadIdx.x, s_cnt[threadIdx.x]);
}

// K arrays of n doubles (array k at in + k * n); workgroup b sums entries [b * chunk, min(n, (b + 1) * chunk)) of each into
// out[k * gridDim.x + b]. Thread t: entries t, t + 1024, ... of the range in four interleaved partial sums, then a fixed tree.
template <int K>
__global__ __launch_bounds__(1024) void vm_score_sum_kernel(const double* __restrict__ in, int n, int chunk, double* __restrict__ out) {
  __shared__ double s_sum[K][16];
  const long long lo = (long long)blockIdx.x * chunk;
  const int hi = (int)min((long long)n, lo + chunk);
  double ps[K][4];
#pragma unroll
  for (int k = 0; k < K; k++)
#pragma unroll
    for (int u = 0; u < 4; u++) ps[k][u] = 0.0;
  for (long long j0 = lo + (long long)threadIdx.x; j0 < hi; j0 += 4096) {
#pragma unroll
    for (int k = 0; k < K; k++) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = in[(size_t)k * n + (size_t)min(j0 + 1024 * u, (long long)hi - 1)];
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (j0 + 1024 * u < hi) ps[k][u] += v[u];
    }
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    double sum = (ps[k][0] + ps[k][1]) + (ps[k][2] + ps[k][3]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) s_sum[k][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double a = 0.0;
    for (int w = 0; w < 16; w++) a += s_sum[threadIdx.x][w];
    out[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = a;
  }
}

}  // namespace fvh
