// Rays cast into the target voxel map: the first hit per ray (fvh_*_cast_rays_source / _cast_rays_cloud: host_incmap.inc.hpp, map_cast_run).
// What should a sensor at this pose see along this ray: the segment from the sensor origin to an endpoint is walked through the grid cell by
// cell (the fp64 Amanatides-Woo walk of vm_raymark_kernel, end_margin = 0); inside every occupied cell the point of the segment's part in that
// cell with the smallest squared Mahalanobis distance to the voxel's Gaussian is found in closed form, and the first cell where that distance
// is <= max_m2 is the hit. The range is therefore not quantised to the voxel size. The contract, operation by operation, is in
// include/fast_vgicp_hip.h; tests/raycast_ref.py restates it.
//   vm_raycast  one ray per lane, read-only on the map. Per visited cell: ray_cell_bucket (a live bitmap answers for absent cells first), and
//               for a cell that exists the 64-byte record in four 16-byte loads issued together, as vm_score_kernel loads it. The walk of a
//               lane ends at its first hit; the longest ray of a wave sets the wave's time, with one dependent chain bitmap word -> key ->
//               record per cell. The integer counts go to LDS, then one atomic per workgroup and counter (n_cells: 64 bits). The per-ray
//               rows are written AT THE RAY'S INPUT INDEX, whatever the walk order. No floating-point atomics.
#pragma once
#include "kernels_voxelmap.hpp"
#include "kernels_mapscore.hpp"

namespace fvh {

// the device image of fvh_ray_cast (include/fast_vgicp_hip.h): read back as it stands
struct VmCastOut {
  int n_rays, n_used, n_hit, n_hit_at_origin;
  long long n_cells;
};

struct VmCast {
  PoseD T;          // scan frame -> map frame
  float origin[3];  // o' = (float)(R o + t), formed by the host (clear_rays_origin_axis)
  double res, min_range, max_range, max_m2;
  int min_points;
};

// the closest approach of the segment x(s) = e + s dm, s in [lo, hi], to a Gaussian at the origin with covariance {cxx .. czz}: -> m2 at that
// point, s through s_out. Every product and sum its own rounding. A record that is singular for this ray (det or B(dm, dm) not > 0 or not
// finite, B(dm, e) not finite): s = lo, m2 = +inf.
__device__ __forceinline__ double cast_closest_nofma(double ex, double ey, double ez, double mx, double my, double mz, double lo, double hi, double cxx, double cxy, double cxz, double cyy,
                                                     double cyz, double czz, double& s_out) {
#pragma clang fp contract(off)
  const double a00 = cyy * czz - cyz * cyz, a01 = cxz * cyz - cxy * czz, a02 = cxy * cyz - cxz * cyy;
  const double a11 = cxx * czz - cxz * cxz, a12 = cxy * cxz - cxx * cyz, a22 = cxx * cyy - cxy * cxy;
  const double det = (cxx * a00 + cxy * a01) + cxz * a02;
  const double den = (((mx * mx) * a00 + (my * my) * a11) + (mz * mz) * a22) + ((((mx * my + my * mx) * a01) + ((mx * mz + mz * mx) * a02)) + ((my * mz + mz * my) * a12));
  const double num = (((mx * ex) * a00 + (my * ey) * a11) + (mz * ez) * a22) + ((((mx * ey + my * ex) * a01) + ((mx * ez + mz * ex) * a02)) + ((my * ez + mz * ey) * a12));
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  s_out = lo;
  if (!(det > 0.0) || !isfinite(det) || !(den > 0.0) || !isfinite(den) || !isfinite(num)) return inf;
  const double sstar = (-num) / den;
  const double s = sstar < lo ? lo : (sstar > hi ? hi : sstar);
  s_out = s;
  return score_m2_nofma(ex + s * mx, ey + s * my, ez + s * mz, cxx, cxy, cxz, cyy, cyz, czz);
}
__device__ __forceinline__ double cast_range_nofma(double s, double r) {
#pragma clang fp contract(off)
  return s * r;
}

// hit_out (n), cell_out (3 n), range_out (n), m2_out (n): rows in input order, each may be null. out: zeroed by the host; n_rays is written
// here -- n, or -1 when the map's own overflow counter is set (a hint-sized batch table that dropped points: the host rebuilds it and asks again).
__global__ __launch_bounds__(256) void vm_raycast_kernel(const float* __restrict__ xyz, int stride, int n, const int* __restrict__ order, VmCast cp, const unsigned long long* __restrict__ keys,
                                                         unsigned mask, const uint4* __restrict__ table, const VmGrid* __restrict__ grid, const unsigned long long* __restrict__ bitmap,
                                                         const int* __restrict__ map_counters, int* __restrict__ hit_out, int* __restrict__ cell_out, double* __restrict__ range_out,
                                                         double* __restrict__ m2_out, VmCastOut* __restrict__ out) {
  __shared__ int s_cnt[3];  // used, hit, hit in the origin's cell
  __shared__ unsigned long long s_cells;
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 3) s_cells = 0ull;
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) out->n_rays = map_counters[1] != 0 ? -1 : n;
  const bool use_grid = grid != nullptr && grid->enabled != 0;
  VmGrid g = {};
  if (use_grid) g = *grid;
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  if (i0 < n) {
    const int i = order ? order[i0] : i0;
    const float* pp = xyz + (size_t)i * stride;
    const float sx0 = pp[0], sy0 = pp[1], sz0 = pp[2];
    const PoseD& T = cp.T;
    const double res = cp.res;
    const double x = sx0, y = sy0, z = sz0;
    // p' by the expression vm_insert_kernel and vm_raymark_kernel spell out
    const float px = (float)(T.r[0] * x + T.r[1] * y + T.r[2] * z + T.t[0]);
    const float py = (float)(T.r[3] * x + T.r[4] * y + T.r[5] * z + T.t[1]);
    const float pz = (float)(T.r[6] * x + T.r[7] * y + T.r[8] * z + T.t[2]);
    const double ox = (double)cp.origin[0], oy = (double)cp.origin[1], oz = (double)cp.origin[2];
    const double ax = ox / res - 0.5, ay = oy / res - 0.5, az = oz / res - 0.5;
    const double bx = (double)px / res - 0.5, by = (double)py / res - 0.5, bz = (double)pz / res - 0.5;
    const double fax = floor(ax), fay = floor(ay), faz = floor(az), fbx = floor(bx), fby = floor(by), fbz = floor(bz);
    const double mx = (double)px - ox, my = (double)py - oy, mz = (double)pz - oz;  // d_m: the segment in metres
    const double r = ray_range_nofma(mx, my, mz);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int hit = -1, hx = 0, hy = 0, hz = 0;
    double range = nan, m2 = nan;
    if (isfinite(sx0) && isfinite(sy0) && isfinite(sz0) && !(r == 0.0) && !(r > cp.max_range) && voxel_index_ok(fax, fay, faz) && voxel_index_ok(fbx, fby, fbz)) {
      hit = 0;
      range = inf;
      m2 = inf;
      int cx = (int)fax, cy = (int)fay, cz = (int)faz;
      const int c0x = cx, c0y = cy, c0z = cz;
      const int ex = (int)fbx, ey = (int)fby, ez = (int)fbz;
      const double dx = bx - ax, dy = by - ay, dz = bz - az;
      const int sx = dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0), sy = dy > 0.0 ? 1 : (dy < 0.0 ? -1 : 0), sz = dz > 0.0 ? 1 : (dz < 0.0 ? -1 : 0);
      const double tdx = 1.0 / fabs(dx), tdy = 1.0 / fabs(dy), tdz = 1.0 / fabs(dz);
      double tmx = dx > 0.0 ? ((double)(cx + 1) - ax) / dx : (dx < 0.0 ? (ax - (double)cx) / (-dx) : inf);
      double tmy = dy > 0.0 ? ((double)(cy + 1) - ay) / dy : (dy < 0.0 ? (ay - (double)cy) / (-dy) : inf);
      double tmz = dz > 0.0 ? ((double)(cz + 1) - az) / dz : (dz < 0.0 ? (az - (double)cz) / (-dz) : inf);
      const double t_lo = cp.min_range / r;
      const int nsteps = min(abs(ex - cx) + abs(ey - cy) + abs(ez - cz), VM_RAY_MAX_STEPS);
      double t_in = 0.0;
      unsigned cells = 0;  // (at most VM_RAY_MAX_STEPS + 1)
#pragma unroll 1
      for (int step = 0; t_in < 1.0; step++) {
        cells++;
        const bool last = step == nsteps;
        const int axis = (tmx <= tmy && tmx <= tmz) ? 0 : (tmy <= tmz ? 1 : 2);  // ties: x before y before z
        const double t_next = axis == 0 ? tmx : (axis == 1 ? tmy : tmz);
        const double t_out = (last || !(t_next < 1.0)) ? 1.0 : t_next;
        if (t_out > t_lo) {
          const unsigned b = ray_cell_bucket(cx, cy, cz, keys, mask, use_grid, g, bitmap);
          if (b != 0xFFFFFFFFu) {
            const float4* tf = reinterpret_cast<const float4*>(table);  // the whole 64-byte record in one go
            const uint4 q0 = table[(size_t)b * 4];
            const float4 q1 = tf[(size_t)b * 4 + 1], q2 = tf[(size_t)b * 4 + 2], q3 = tf[(size_t)b * 4 + 3];
            if (!(cp.min_points > 1 && (int)q0.z < cp.min_points)) {
              const double lo = t_in > t_lo ? t_in : t_lo;
              double s;
              const double v = cast_closest_nofma(ox - (double)q1.x, oy - (double)q1.y, oz - (double)q1.z, mx, my, mz, lo, t_out, (double)q2.x, (double)q2.y, (double)q2.z, (double)q2.w,
                                                  (double)q3.x, (double)q3.y, s);
              if (v <= cp.max_m2) {
                hit = 1; hx = cx; hy = cy; hz = cz;
                range = cast_range_nofma(s, r);
                m2 = v;
                break;
              }
            }
          }
        }
        if (last) break;
        t_in = t_next;
        if (axis == 0) { cx += sx; tmx += tdx; }
        else if (axis == 1) { cy += sy; tmy += tdy; }
        else { cz += sz; tmz += tdz; }
      }
      atomicAdd(&s_cnt[0], 1);
      if (hit == 1) {
        atomicAdd(&s_cnt[1], 1);
        if (hx == c0x && hy == c0y && hz == c0z) atomicAdd(&s_cnt[2], 1);
      }
      atomicAdd(&s_cells, (unsigned long long)cells);
    }
    if (hit_out) hit_out[i] = hit;
    if (cell_out) { cell_out[3 * (size_t)i] = hx; cell_out[3 * (size_t)i + 1] = hy; cell_out[3 * (size_t)i + 2] = hz; }
    if (range_out) range_out[i] = range;
    if (m2_out) m2_out[i] = m2;
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&out->n_used + threadIdx.x, s_cnt[threadIdx.x]);
  if (threadIdx.x == 3 && s_cells) atomicAdd(reinterpret_cast<unsigned long long*>(&out->n_cells), s_cells);
}

}  // namespace fvh
