// RANSAC plane segmentation behind the voxel filter, for gfx950 (wave64): pcl::SACSegmentation for SACMODEL_PLANE /
// SACMODEL_PERPENDICULAR_PLANE with SAC_RANSAC, with hypotheses from a counter-based generator (include/fast_vgicp_hip.h:
// fvh_voxelgrid_segment_plane is the contract; tests/plane_ref.py restates it in numpy).
//
//   hypo     one thread per hypothesis: three input indices from mix32, the plane through them in fp64, validity (distinct indices,
//            nn != 0, the axis test); counts[h] = 0, or -1 for an invalid hypothesis
//   sweep    the N x H point-against-plane tests. ONE HYPOTHESIS PER LANE with a private register counter; a workgroup stages a slab of
//            PLANE_SLAB points in LDS, widened to fp64 once, and each of its four waves (64 hypotheses each) walks the slab reading
//            every point at ONE address for all lanes (an LDS broadcast: no bank conflict, no cross-lane traffic, no ballot in the
//            loop); one integer atomicAdd per lane per slab at the end. Counts are integers: no result depends on the visiting order.
//   winner   one wave: the valid hypothesis with the largest count, ties to the smallest h; its plane goes into the control words
//   refit    (FVH_PLANE_REFINE) count, first and second moments of the winner's inliers about q = p[i0] in fp64: per workgroup of
//            1,024 points in a fixed order, then one wave adds the partial sums in a fixed order and takes the eigenvector of the
//            smallest eigenvalue from sym_eig3 (dev_math.hpp); the final coefficients stay on the device for the flag kernel
//   flag     one thread per input point: the keep flag (inlier, or its complement) and the score (float)(|s_i| / sqrt(nn))
// The flags then go through device_scan and outlier_compact_kernel like those of an outlier filter.
//
// Every expression the contract writes down is evaluated with its association and without contraction: twin and device agree on every
// count to the last point. There is no division and no square root in a test.
#pragma once
#include "dev_math.hpp"
#include "kernels_outlier.hpp"

namespace fvh {

constexpr int PLANE_SLAB = 256;         // points a workgroup of the sweep stages in LDS (6 KiB as fp64 x, y, z)
constexpr int PLANE_MAX_HYP = 16384;    // max_iterations
constexpr int PLANE_REFIT_ITEMS = 1024; // points per workgroup of the refit's partial sums
constexpr int PLANE_MOMENTS = 10;       // count, 3 first moments, 6 second moments

// one hypothesis: (a, b, c) = e1 x e2 (not normalised), nn = |(a, b, c)|^2, q = p[i0]
struct PlaneHyp {
  double a, b, c, nn, qx, qy, qz;
  int i0, i1, i2, valid;
};

// control words of one call: those of the filters (bad, count), the winner, and with a refit the final coefficients; one copy brings
// them to the host
struct PlaneCtl {
  OutlierCtl o;
  double coef[4];  // refit only: unit normal and d, sign fixed
  PlaneHyp win;    // the winner's plane (valid = 0: there is none)
  int winner, nvalid, count_w, refit;
};

__host__ __device__ __forceinline__ unsigned plane_mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ unsigned plane_seed_word(unsigned long long seed) {
  return plane_mix32((unsigned)(seed & 0xffffffffull) ^ plane_mix32((unsigned)(seed >> 32) ^ 0x9e3779b9u));
}
__host__ __device__ __forceinline__ int plane_sample_index(unsigned s0, int h, int j, int n) {
  const unsigned r = plane_mix32(s0 + 0x9e3779b9u * (unsigned)(3 * h + j + 1));
  return (int)(((unsigned long long)r * (unsigned long long)(unsigned)n) >> 32);
}

// (a, b, c, d) with d >= 0; d == 0: the first non-zero component of the normal is positive
__host__ __device__ __forceinline__ void plane_fix_sign(double* co) {
  const bool flip = co[3] < 0.0 || (co[3] == 0.0 && (co[0] < 0.0 || (co[0] == 0.0 && (co[1] < 0.0 || (co[1] == 0.0 && co[2] < 0.0)))));
  if (flip) { co[0] = -co[0]; co[1] = -co[1]; co[2] = -co[2]; co[3] = -co[3]; }
}

// s_i of the contract: u = p - q, (a ux + b uy) + c uz
__device__ __forceinline__ double plane_signed(const PlaneHyp& w, double x, double y, double z) {
#pragma clang fp contract(off)
  const double ux = x - w.qx, uy = y - w.qy, uz = z - w.qz;
  return (w.a * ux + w.b * uy) + w.c * uz;
}

__global__ __launch_bounds__(256) void plane_hypo_kernel(const float4* __restrict__ pts, int n, int H, unsigned s0, int use_axis, double ax, double ay, double az, double aa, double c2,
                                                         PlaneHyp* __restrict__ hyp, int* __restrict__ counts) {
#pragma clang fp contract(off)
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  PlaneHyp r;
  r.a = r.b = r.c = r.nn = r.qx = r.qy = r.qz = 0.0;
  r.i0 = r.i1 = r.i2 = 0;
  r.valid = 0;
  if (n > 0) {  // (n >= 1: the three indices are below n; n < 3 leaves two of them equal)
    r.i0 = plane_sample_index(s0, h, 0, n);
    r.i1 = plane_sample_index(s0, h, 1, n);
    r.i2 = plane_sample_index(s0, h, 2, n);
    const float4 p0 = pts[r.i0], p1 = pts[r.i1], p2 = pts[r.i2];
    r.qx = (double)p0.x; r.qy = (double)p0.y; r.qz = (double)p0.z;
    const double e1x = (double)p1.x - r.qx, e1y = (double)p1.y - r.qy, e1z = (double)p1.z - r.qz;
    const double e2x = (double)p2.x - r.qx, e2y = (double)p2.y - r.qy, e2z = (double)p2.z - r.qz;
    r.a = e1y * e2z - e1z * e2y;
    r.b = e1z * e2x - e1x * e2z;
    r.c = e1x * e2y - e1y * e2x;
    r.nn = (r.a * r.a + r.b * r.b) + r.c * r.c;
    bool ok = r.i0 != r.i1 && r.i0 != r.i2 && r.i1 != r.i2 && r.nn != 0.0;
    if (use_axis) {
      const double dot = (r.a * ax + r.b * ay) + r.c * az;
      ok = ok && dot * dot >= (c2 * r.nn) * aa;
    }
    r.valid = ok ? 1 : 0;
  }
  hyp[h] = r;
  counts[h] = r.valid ? 0 : -1;
}

// grid (slabs of PLANE_SLAB points, groups of 256 hypotheses), 256 threads. Thread t stages point base + t (t < m masks the slab's tail:
// nothing is read past the cloud); wave w takes the hypotheses (4 blockIdx.y + w) * 64 + lane (h < H masks the group's tail: nothing is
// read past the H records, and such a lane, like an invalid hypothesis, adds nothing). The loop bound m is workgroup-uniform.
__global__ __launch_bounds__(256) void plane_sweep_kernel(const float4* __restrict__ pts, int n, int H, double t2, const PlaneHyp* __restrict__ hyp, int* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ double sx[PLANE_SLAB], sy[PLANE_SLAB], sz[PLANE_SLAB];
  const int base = blockIdx.x * PLANE_SLAB;
  const int m = min(PLANE_SLAB, n - base);
  const int t = threadIdx.x;
  if (t < m) {
    const float4 p = pts[base + t];
    sx[t] = (double)p.x; sy[t] = (double)p.y; sz[t] = (double)p.z;
  }
  __syncthreads();
  const int h = (blockIdx.y * 4 + (t >> 6)) * 64 + (t & 63);
  if (h >= H) return;
  const PlaneHyp w = hyp[h];
  if (!w.valid) return;
  const double bound = t2 * w.nn;
  int cnt = 0;
#pragma unroll 4
  for (int j = 0; j < m; j++) {
    const double s = plane_signed(w, sx[j], sy[j], sz[j]);
    cnt += (s * s <= bound) ? 1 : 0;
  }
  if (cnt) atomicAdd(counts + h, cnt);
}

// One wave. Lane l scans h = l, l + 64, ... in ascending order (a strictly larger count replaces), then the lanes meet in a fixed
// butterfly on (count, h): larger count, then smaller h. Invalid hypotheses carry -1 and never win.
__global__ __launch_bounds__(64) void plane_winner_kernel(int H, const PlaneHyp* __restrict__ hyp, const int* __restrict__ counts, PlaneCtl* __restrict__ ctl) {
  const int lane = threadIdx.x;
  int best = -1, bh = 0x7fffffff, nvalid = 0;
  for (int h = lane; h < H; h += 64) {
    const int c = counts[h];
    nvalid += c >= 0 ? 1 : 0;
    if (c > best) { best = c; bh = h; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int ob = __shfl_xor(best, off), oh = __shfl_xor(bh, off);
    nvalid += __shfl_xor(nvalid, off);
    if (ob > best || (ob == best && oh < bh)) { best = ob; bh = oh; }
  }
  if (lane != 0) return;
  ctl->nvalid = nvalid;
  if (best < 0) {  // no valid hypothesis (ctl was zeroed: win.valid = 0, count_w = 0)
    ctl->winner = -1;
    return;
  }
  ctl->winner = bh;
  ctl->count_w = best;
  ctl->win = hyp[bh];
}

// Partial sums of the refit, one workgroup per PLANE_REFIT_ITEMS points: thread t adds its points base + t, base + t + 256, ... in that
// order, the wave meets in a fixed butterfly, thread 0 adds the four waves in order. part[block * PLANE_MOMENTS + k].
__global__ __launch_bounds__(256) void plane_refit_partial_kernel(const float4* __restrict__ pts, int n, double t2, const PlaneCtl* __restrict__ ctl, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sw[4][PLANE_MOMENTS];
  const PlaneHyp w = ctl->win;
  double acc[PLANE_MOMENTS];
#pragma unroll
  for (int k = 0; k < PLANE_MOMENTS; k++) acc[k] = 0.0;
  if (w.valid) {
    const double bound = t2 * w.nn;
    const int base = blockIdx.x * PLANE_REFIT_ITEMS + threadIdx.x;
#pragma unroll
    for (int u = 0; u < PLANE_REFIT_ITEMS / 256; u++) {
      const int i = base + u * 256;
      if (i < n) {
        const float4 p = pts[i];
        const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
        const double s = plane_signed(w, x, y, z);
        if (s * s <= bound) {
          const double ux = x - w.qx, uy = y - w.qy, uz = z - w.qz;
          acc[0] += 1.0;
          acc[1] += ux; acc[2] += uy; acc[3] += uz;
          acc[4] += ux * ux; acc[5] += ux * uy; acc[6] += ux * uz;
          acc[7] += uy * uy; acc[8] += uy * uz; acc[9] += uz * uz;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < PLANE_MOMENTS; k++) acc[k] += __shfl_xor(acc[k], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < PLANE_MOMENTS; k++) sw[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < PLANE_MOMENTS) {
    const int k = threadIdx.x;
    part[(size_t)blockIdx.x * PLANE_MOMENTS + k] = ((sw[0][k] + sw[1][k]) + sw[2][k]) + sw[3][k];
  }
}

// One wave. Lane l adds the partial sums of workgroups l, l + 64, ... in ascending order, the lanes meet in a fixed butterfly; lane 0
// forms mean and covariance about q, takes the eigenvector of the smallest eigenvalue and leaves the coefficients, sign fixed, in ctl.
// Fewer than 3 inliers: no refit (ctl->refit stays 0).
__global__ __launch_bounds__(64) void plane_refit_final_kernel(int nblocks, const double* __restrict__ part, PlaneCtl* __restrict__ ctl) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  double acc[PLANE_MOMENTS];
#pragma unroll
  for (int k = 0; k < PLANE_MOMENTS; k++) acc[k] = 0.0;
  for (int b = lane; b < nblocks; b += 64) {
#pragma unroll
    for (int k = 0; k < PLANE_MOMENTS; k++) acc[k] += part[(size_t)b * PLANE_MOMENTS + k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < PLANE_MOMENTS; k++) acc[k] += __shfl_xor(acc[k], off);
  }
  if (lane != 0 || !ctl->win.valid || ctl->count_w < 3) return;
  const double m = acc[0];
  const double mx = acc[1] / m, my = acc[2] / m, mz = acc[3] / m;
  Sym3<double> C;
  C.xx = acc[4] / m - mx * mx; C.xy = acc[5] / m - mx * my; C.xz = acc[6] / m - mx * mz;
  C.yy = acc[7] / m - my * my; C.yz = acc[8] / m - my * mz; C.zz = acc[9] / m - mz * mz;
  double wv[3], V[9];
  sym_eig3(C, wv, V);
  double co[4];
  co[0] = V[0]; co[1] = V[3]; co[2] = V[6];  // the column of the smallest eigenvalue
  const double cx = ctl->win.qx + mx, cy = ctl->win.qy + my, cz = ctl->win.qz + mz;
  co[3] = -((co[0] * cx + co[1] * cy) + co[2] * cz);
  plane_fix_sign(co);
#pragma unroll
  for (int k = 0; k < 4; k++) ctl->coef[k] = co[k];
  ctl->refit = 1;
}

// In input order: inlier = the winner's count test, or after a refit s * s <= t2 * ((a a + b b) + c c) with s = ((a x + b y) + c z) + d
// on the coefficients the call returns; keep = inlier, or its complement; score = (float)(|s_i| / sqrt(nn)) to the WINNER's plane
// (+inf when there is no model: every point is an outlier).
__global__ __launch_bounds__(256) void plane_flag_kernel(const float4* __restrict__ pts, int n, double t2, int keep_outliers, const PlaneCtl* __restrict__ ctl,
                                                         unsigned* __restrict__ flags, float* __restrict__ score) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const PlaneHyp w = ctl->win;
  bool inlier = false;
  float dist = __builtin_inff();
  if (w.valid) {
    const float4 p = pts[i];
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    const double s = plane_signed(w, x, y, z);
    dist = (float)(fabs(s) / sqrt(w.nn));
    if (ctl->refit) {
      const double a = ctl->coef[0], b = ctl->coef[1], c = ctl->coef[2], d = ctl->coef[3];
      const double r = ((a * x + b * y) + c * z) + d;
      inlier = r * r <= t2 * ((a * a + b * b) + c * c);
    } else {
      inlier = s * s <= t2 * w.nn;
    }
  }
  flags[i] = (inlier != (keep_outliers != 0)) ? 1u : 0u;
  score[i] = dist;
}

}  // namespace fvh
