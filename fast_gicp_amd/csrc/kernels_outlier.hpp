// Point-cloud preparation behind the voxel filter, for gfx950 (wave64): range crop, statistical outlier removal, radius outlier
// removal (include/fast_vgicp_hip.h: fvh_voxelgrid_crop_range / _remove_statistical_outliers / _remove_radius_outliers).
//
// Every filter ends in the same three steps: one `unsigned` keep flag per input point, the exclusive scan of the flags
// (device_scan), and an order-preserving compaction that writes the kept points as bit copies of the input. What differs is how the
// flag is found:
//   crop         one thread per point: s = (x*x + y*y) + z*z in fp32 without contraction, min <= s <= max, all coordinates finite
//   radius       one query per WAVE on the Morton-sorted cloud, shaped like cov_rbf1_kernel (kernels_cov.hpp): the wave counts the
//                candidates within r of its query tile by tile and LEAVES as soon as the count reaches min_neighbors
//   statistical  the exact k-NN (find_neighbors, k = mean_k + 1) gives the neighbour lists; four lanes per point gather them in one
//                batch and sum sqrtf(d^2) in fp64; one workgroup reduces sum d and sum d^2 in a fixed order and leaves the
//                threshold in device memory for the flag kernel: no host round trip between scoring and compaction
// Distances are sqdist_nofma everywhere: the quantity the k-NN ranks by, and what the numpy twin of the tests evaluates.
#pragma once
#include "kernels_cov.hpp"
#include "kernels_downsample.hpp"

namespace fvh {

// control words of one filter call (zeroed by the host before the first kernel)
struct OutlierCtl {
  double sum, sumsq;   // statistical: sum d_i, sum d_i^2
  double threshold;    // statistical: mu + stddev_mul * sigma
  unsigned bad;        // a non-finite coordinate was met (the two outlier filters refuse such a cloud)
  unsigned count;      // kept points (written by the compaction kernel: one copy brings {threshold, bad, count} to the host)
};

__device__ __forceinline__ float sqnorm_nofma(const float4& p) {
#pragma clang fp contract(off)
  return (p.x * p.x + p.y * p.y) + p.z * p.z;
}
// (finite3: kernels_downsample.hpp)

// The outlier filters refuse a cloud with a non-finite coordinate, and the host learns of it with the count, at the end of the chain:
// until then the sort, the search and the sweep must see finite points only -- an offending point is replaced by the origin in the
// widened copy (never in the caller's array), which is discarded with the call's result.
__global__ __launch_bounds__(256) void outlier_finite_kernel(float4* __restrict__ pts, int n, OutlierCtl* __restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!finite3(pts[i])) {
    pts[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    atomicOr(&ctl->bad, 1u);
  }
}

// crop: keep iff finite and min_sq <= (double)s <= max_sq (max_sq may be +inf); score = s
__global__ __launch_bounds__(256) void crop_flag_kernel(const float4* __restrict__ pts, int n, double min_sq, double max_sq, unsigned* __restrict__ flags, float* __restrict__ score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const float s = sqnorm_nofma(p);
  const double sd = (double)s;
  score[i] = s;
  flags[i] = (finite3(p) && min_sq <= sd && sd <= max_sq) ? 1u : 0u;
}

// Radius outlier removal: #{ j != i : d^2(i, j) <= r2 } >= min_neighbors. One query per wave on the Morton-sorted cloud: the query's own
// tile first (on a LiDAR cloud it usually settles the answer), then the two-level box cull of cov_rbf1_kernel against r2, the next
// surviving tile's load in flight while the current one is counted. The count is a popcount of a ballot -- a scalar, so every exit
// below is wave-uniform. Slots past the end of the cloud are candidates at 3e18 (load_candidate: d^2 = 2.7e37) and r2 <= 1e37: never counted.
// Lane 0 writes flag and score = min(count, min_neighbors) at the query's original index. No LDS.
__global__ __launch_bounds__(256) void outlier_radius_count_kernel(const float4* __restrict__ spts, const float4* __restrict__ bbox1, const float4* __restrict__ bbox2, int n, float r2,
                                                                   int min_neighbors, unsigned* __restrict__ flags, float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= n) return;
  const int ntiles = (n + 63) >> 6, nsuper = (ntiles + 63) >> 6;
  const float4 qv = spts[q];
  const float qx = read_lane(qv.x, 0), qy = read_lane(qv.y, 0), qz = read_lane(qv.z, 0);
  const int own = read_lane(__float_as_int(qv.w), 0);
  const int t0 = q >> 6;
  int cnt = 0;
  auto count = [&](const float4& p) __attribute__((always_inline)) {
    const float sq = sqdist_nofma(p, qx, qy, qz);
    cnt += __popcll(__ballot(sq <= r2 && __float_as_int(p.w) != own));
  };
  count(load_candidate(spts, (t0 << 6) + lane, n));
  for (int sc = 0; sc < nsuper && cnt < min_neighbors; sc += 64) {
    const int s = sc + lane;
    const float lb2 = (s < nsuper) ? point_box_sq(bbox2[2 * s], bbox2[2 * s + 1], qx, qy, qz) : __builtin_inff();
    unsigned long long smask = __ballot(lb2 <= r2);
    while (smask && cnt < min_neighbors) {
      const int ssrc = __ffsll((long long)smask) - 1;
      smask &= smask - 1;
      const int t = ((sc + ssrc) << 6) + lane;
      const float lb = (t < ntiles) ? point_box_sq(bbox1[2 * t], bbox1[2 * t + 1], qx, qy, qz) : __builtin_inff();
      unsigned long long tmask = __ballot(lb <= r2 && t != t0);
      if (!tmask) continue;
      int cur = __ffsll((long long)tmask) - 1;
      tmask &= tmask - 1;
      float4 pcur = load_candidate(spts, ((((sc + ssrc) << 6) + cur) << 6) + lane, n);
      while (true) {  // the next tile is in flight while this one is counted
        int nxt = -1;
        float4 pnxt = pcur;
        if (tmask) {
          nxt = __ffsll((long long)tmask) - 1;
          tmask &= tmask - 1;
          pnxt = load_candidate(spts, ((((sc + ssrc) << 6) + nxt) << 6) + lane, n);
        }
        count(pcur);
        if (nxt < 0 || cnt >= min_neighbors) break;
        pcur = pnxt;
      }
    }
  }
  if (lane == 0) {
    flags[own] = cnt >= min_neighbors ? 1u : 0u;
    score[own] = (float)min(cnt, min_neighbors);
  }
}

// Statistical outlier removal, step 1: d_i = (float)(sum_j (double)sqrtf(d^2(i, j)) / mean_k) over the k1 = mean_k + 1 nearest points of
// the cloud (find_neighbors' lists, original indices; the nearest is at distance 0 and adds nothing). FOUR lanes per point as in
// cov_from_neighbors_kernel, for the same reason: all indices of a lane in one round trip, then all its points in a second one -- never
// "if (j < k1) p = pts[nbr[j]]", which puts every load behind its own wait. Slots past k1 read a valid neighbour again and are masked.
// The partial sums meet through two xor-shuffles in a fixed order.
constexpr int OUTLIER_LANES = 4;
template <int PER_LANE>  // neighbours a lane holds: k1 <= 4 * PER_LANE
__global__ __launch_bounds__(256) void outlier_mean_dist_kernel(const float4* __restrict__ pts, int n, int k1, const int* __restrict__ nbr, float* __restrict__ score) {
  const int gt = blockIdx.x * 256 + threadIdx.x;
  const int sub = gt % OUTLIER_LANES;
  const int i = min(gt / OUTLIER_LANES, n - 1);
  const int* nb = nbr + (size_t)i * k1;
  const float4 q = pts[i];
  int idx[PER_LANE];
#pragma unroll
  for (int u = 0; u < PER_LANE; u++) idx[u] = nb[min(sub + u * OUTLIER_LANES, k1 - 1)];
  float4 pq[PER_LANE];
#pragma unroll
  for (int u = 0; u < PER_LANE; u++) pq[u] = pts[idx[u]];
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < PER_LANE; u++) {
    // sqrtf, correctly rounded (hipcc's default for fp32 sqrt); NOT __fsqrt_rn, which this toolchain maps to the 1-ulp native instruction
    const double d = (double)sqrtf(sqdist_nofma(pq[u], q.x, q.y, q.z));
    s = (sub + u * OUTLIER_LANES < k1) ? s + d : s;
  }
#pragma unroll
  for (int off = 1; off < OUTLIER_LANES; off <<= 1) s += __shfl_xor(s, off);
  if (sub == 0 && gt / OUTLIER_LANES < n) score[i] = (float)(s / (double)(k1 - 1));
}

// step 2: mu = sum d / n, var = max(0, (sum d^2 - (sum d)^2 / n) / (n - 1)), t = mu + stddev_mul * sqrt(var), all in fp64. One workgroup,
// the summation order of fitness_reduce_kernel (thread t: entries t, t + 1024, ... in four interleaved partial sums, then a fixed tree):
// two runs give the same bits. The threshold stays on the device for outlier_flag_kernel.
__global__ __launch_bounds__(1024) void outlier_stats_kernel(const float* __restrict__ score, int n, double stddev_mul, OutlierCtl* __restrict__ ctl) {
  __shared__ double s_sum[16], s_sq[16];
  double ps[4] = {0.0, 0.0, 0.0, 0.0}, pq[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i0 = threadIdx.x; i0 < n; i0 += 4096) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = score[min(i0 + 1024 * u, n - 1)];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double d = (double)v[u];
      if (i0 + 1024 * u < n) { ps[u] += d; pq[u] += d * d; }
    }
  }
  double sum = (ps[0] + ps[1]) + (ps[2] + ps[3]), sq = (pq[0] + pq[1]) + (pq[2] + pq[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off); sq += __shfl_xor(sq, off); }
  if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_sq[threadIdx.x >> 6] = sq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < 16; w++) { a += s_sum[w]; b += s_sq[w]; }
    const double mu = a / (double)n;
    const double var = fmax(0.0, (b - a * a / (double)n) / (double)(n - 1));
    ctl->sum = a;
    ctl->sumsq = b;
    ctl->threshold = mu + stddev_mul * sqrt(var);
  }
}

// step 3: keep iff (double)d_i <= t
__global__ __launch_bounds__(256) void outlier_flag_kernel(const float* __restrict__ score, int n, const OutlierCtl* __restrict__ ctl, unsigned* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flags[i] = ((double)score[i] <= ctl->threshold) ? 1u : 0u;
}

// The kept points, in input order, at their scanned positions: packed xyz (`out`), float4 {x, y, z, 0} (`out4`: what
// fvh_ndt_*_from_voxelgrid swaps into a cloud) and their indices into the input. pts is the widened copy of the input: bit copies.
__global__ __launch_bounds__(256) void outlier_compact_kernel(const float4* __restrict__ pts, int n, const unsigned* __restrict__ flags, const unsigned* __restrict__ pos,
                                                              const unsigned* __restrict__ total, float* __restrict__ out, float4* __restrict__ out4, int* __restrict__ kept,
                                                              OutlierCtl* __restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) ctl->count = *total;
  if (i >= n || !flags[i]) return;
  const float4 p = pts[i];
  const size_t j = pos[i];
  out[3 * j] = p.x; out[3 * j + 1] = p.y; out[3 * j + 2] = p.z;
  out4[j] = make_float4(p.x, p.y, p.z, 0.f);
  kept[j] = i;
}

}  // namespace fvh
