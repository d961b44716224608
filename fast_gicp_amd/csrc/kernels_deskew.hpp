// Motion compensation ("deskew") of one LiDAR sweep behind the voxel filter's handle, for gfx950 (include/fast_vgicp_hip.h:
// fvh_voxelgrid_deskew). One point per lane: p' = float( T(t_ref)^-1 * T(t_i) * p_i ), T(x) = T[j] * exp(s * xi_j) on the piecewise
// constant-twist trajectory through the K knot poses. Everything before the final cast is fp64.
//
// The host (host_deskew.inc.hpp) folds T(t_ref)^-1 * T[j] into one 3 x 4 matrix A_j per segment and takes the logarithm of every
// segment once; what is left per point is the search for its segment, one SE(3) exponential and two 3 x 4 products. The at most 63
// segment records (160 B each) are read into LDS once per workgroup; a lane reads its own record from there (lanes of a wave are
// neighbours in the sweep: nearly always the same segment, a broadcast).
//
// The exponential here is written for per-lane twists (every lane its own s). dev_se3_exp of kernels_cost.hpp serves wave-uniform
// callers and is not used.
#pragma once
#include <hip/hip_runtime.h>

namespace fvh {

constexpr int DESKEW_MAX_KNOTS = 64;
constexpr int DESKEW_SEG_DOUBLES = 20;

// one segment [tau_j, tau_{j+1}) of the trajectory, as the kernel reads it
struct DeskewSeg {
  double a[12];    // A_j = T(t_ref)^-1 * T[j], 3 x 4 row-major {R | t}
  double w[3];     // rotation part of xi_j = log(T[j]^-1 * T[j+1])
  double v[3];     // translation part
  double tau;      // tau[j]
  double inv_dt;   // 1 / (tau[j+1] - tau[j])
};
static_assert(sizeof(DeskewSeg) == sizeof(double) * DESKEW_SEG_DOUBLES, "records are copied to LDS as doubles");

// q = exp(s * xi) * p for xi = (w, v), rotation first: R p + V (s v), with
//   R = I + a K + b K^2,  V = I + b K + c K^2,  K = [s w]x,  a = sin(th) / th,  b = (1 - cos(th)) / th^2,  c = (th - sin(th)) / th^3.
// sin(th) and 1 - cos(th) come from ONE sincos of the half angle (no cancellation in b). Below 1e-10 rad the series a = 1, b = 1/2,
// c = 1/6 (the terms dropped are below 1e-20 relative); th == 0 gives q = p + s v with p's bits when v is zero too.
__device__ __forceinline__ void deskew_se3_exp_apply(const double w0, const double w1, const double w2, const double u0, const double u1, const double u2,
                                                     const double px, const double py, const double pz, double& qx, double& qy, double& qz) {
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  const double th = sqrt(th2);
  double a = 1.0, b = 0.5, c = 1.0 / 6.0;
  if (th >= 1e-10) {
    double sh, ch;
    sincos(0.5 * th, &sh, &ch);
    const double sn = 2.0 * sh * ch;
    a = sn / th;
    b = 2.0 * sh * sh / th2;
    c = (th - sn) / (th2 * th);
  }
  // K p, K^2 p = w x (w x p)
  const double k1x = w1 * pz - w2 * py, k1y = w2 * px - w0 * pz, k1z = w0 * py - w1 * px;
  const double k2x = w1 * k1z - w2 * k1y, k2y = w2 * k1x - w0 * k1z, k2z = w0 * k1y - w1 * k1x;
  // K u, K^2 u
  const double l1x = w1 * u2 - w2 * u1, l1y = w2 * u0 - w0 * u2, l1z = w0 * u1 - w1 * u0;
  const double l2x = w1 * l1z - w2 * l1y, l2y = w2 * l1x - w0 * l1z, l2z = w0 * l1y - w1 * l1x;
  qx = (px + a * k1x + b * k2x) + (u0 + b * l1x + c * l2x);
  qy = (py + a * k1y + b * k2y) + (u1 + b * l1y + c * l2y);
  qz = (pz + a * k1z + b * k2z) + (u2 + b * l1z + c * l2z);
}

// pts: the input widened to float4 (upload_cloud). times[i * time_stride]: the time of point i. segs: nseg = K - 1 records, 1 <= nseg <= 63.
// out: packed xyz, out4: {x, y, z, 0}. A point with a non-finite coordinate or time comes out as three NaNs.
__global__ __launch_bounds__(256) void deskew_points_kernel(const float4* __restrict__ pts, int n, const float* __restrict__ times, int time_stride,
                                                            const double* __restrict__ segs, int nseg, float* __restrict__ out, float4* __restrict__ out4) {
  __shared__ double s_seg[(DESKEW_MAX_KNOTS - 1) * DESKEW_SEG_DOUBLES];
  __shared__ double s_tau[DESKEW_MAX_KNOTS];
  for (int k = threadIdx.x; k < nseg * DESKEW_SEG_DOUBLES; k += 256) s_seg[k] = segs[k];
  if ((int)threadIdx.x < nseg) s_tau[threadIdx.x] = segs[threadIdx.x * DESKEW_SEG_DOUBLES + 18];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const float tf = times[(size_t)i * time_stride];
  const double x = (double)tf;
  // the largest j with tau[j] <= x, within [0, nseg - 1]: before the first knot and after the last one the end segments extrapolate
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s_tau[mid] <= x) lo = mid; else hi = mid - 1;
  }
  const double* g = s_seg + lo * DESKEW_SEG_DOUBLES;
  const double s = (x - g[18]) * g[19];
  double qx, qy, qz;
  deskew_se3_exp_apply(s * g[12], s * g[13], s * g[14], s * g[15], s * g[16], s * g[17], (double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
  float rx = (float)(g[0] * qx + g[1] * qy + g[2] * qz + g[3]);
  float ry = (float)(g[4] * qx + g[5] * qy + g[6] * qz + g[7]);
  float rz = (float)(g[8] * qx + g[9] * qy + g[10] * qz + g[11]);
  const bool ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(tf);
  if (!ok) rx = ry = rz = __builtin_nanf("");
  out[3 * (size_t)i] = rx;
  out[3 * (size_t)i + 1] = ry;
  out[3 * (size_t)i + 2] = rz;
  out4[i] = make_float4(rx, ry, rz, 0.f);
}

}  // namespace fvh
