// Euclidean cluster extraction behind the voxel filter, for gfx950 (wave64): the connected components of the graph "i ~ j iff i != j and
// d2(i, j) <= r2" (include/fast_vgicp_hip.h: fvh_voxelgrid_cluster_euclidean), d2 = sqdist_nofma as in the radius filter.
//
//   link     one query per WAVE on the Morton-sorted cloud, the sweep of outlier_radius_count_kernel (kernels_outlier.hpp) without its
//            early exit: every candidate at a LOWER sorted position within r2 is united with the query in a lock-free union-find over
//            sorted positions (an edge is seen from its higher end, so only tiles up to the query's own are visited)
//   flatten  root of every sorted position; per root the component size (integer atomicAdd) and the smallest INPUT index (atomicMin)
//   flags    in input order: keep = the size window, leader = "this point is its kept component's smallest input index", score = size
//   labels   the exclusive scan of the leader flags numbers the clusters in ascending order of their smallest input index
// The keep flags then go through device_scan and outlier_compact_kernel like those of an outlier filter. Integers only: no result
// depends on the order in which waves run.
//
// Memory rules of the union-find (parent[], one int per sorted position, parent[x] <= x, a root has parent[x] == x):
//   * inside the link kernel parent[] is touched by agent-scope atomics only (relaxed atomic loads, atomicCAS, atomicMin): the L2s of
//     the eight XCDs are not coherent for plain loads within one kernel;
//   * a value read from parent[x] may be old, but it is never wrong: parent[x] only ever decreases, and every value it has held is a
//     member of x's set for good (sets only merge). A find over old values ends at a node that is in the set but may no longer be its
//     root; a hook under such a node joins the sets just the same, and the hook itself is an atomicCAS that succeeds only on a true root;
//   * no wave waits for another wave's store: a failed hook goes on from the value the atomic returned;
//   * the kernel boundary gives the flatten pass a coherent view of parent[].
#pragma once
#include <climits>

#include "kernels_outlier.hpp"

namespace fvh {

// control words of one clustering call: those of the filters (bad, count: written by outlier_finite_kernel / outlier_compact_kernel)
// and the number of kept components; one copy brings them to the host
struct ClusterCtl {
  OutlierCtl o;
  unsigned num_clusters;
  unsigned pad;
};

__device__ __forceinline__ int uf_load(const int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Terminates: parent[x] <= x with equality at a root only, so every step strictly lowers x.
__device__ __forceinline__ int uf_find(const int* parent, int x, int* hops = nullptr) {
  int p = uf_load(parent, x), h = 0;
  while (p != x) {
    x = p;
    p = uf_load(parent, x);
    h++;
  }
  if (hops) *hops = h;
  return x;
}

// Unite the sets of a and b; returns a member of the united set no larger than either root found (its root, unless another wave has
// hooked it since). The larger root hooks under the smaller one by atomicCAS(parent[hi], hi, lo): it succeeds only while hi is a root.
// Terminates: a pass either returns or replaces hi by the value the failed CAS returned, which is parent[hi] < hi -- a + b strictly
// decreases from pass to pass and is bounded below; nothing here waits for a value another wave has yet to write.
__device__ __forceinline__ int uf_unite(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return a;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = old;
    b = lo;
  }
}

__global__ __launch_bounds__(256) void cluster_init_kernel(int n, int* __restrict__ parent, int* __restrict__ csize, int* __restrict__ cmin) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  parent[i] = i;
  csize[i] = 0;
  cmin[i] = INT_MAX;
}

// One query per wave, q = its sorted position. The query's own tile first, then the two-level box cull of outlier_radius_count_kernel
// against r2 over the tiles BELOW its own, the next surviving tile's load in flight while the current one is tested. A hit is a candidate
// at a sorted position c < q with d2 <= r2 (slots past the end of the cloud sit at 3e18: d2 = 2.7e37 > r2, and c < q < n excludes them
// anyway; c < q also excludes the query itself, and keeps an exact duplicate). The hit lanes find their roots (each lane its own chain);
// the wave then makes ONE hook per distinct root: `rq`, the query's side of every union, is wave-uniform, the first lane whose root
// differs from it unites the two and hands the result to the wave, and every lane that held the same root or the new rq is done.
//
// Why every loop ends (no wave depends on another wave's progress): uf_find strictly descends; a pass of uf_unite that does not return
// lowers the sum of its two nodes; the `todo` loop clears at least the bit of the lane it served. Path compression is atomicMin with a
// member of the same set below the node: parent[] stays monotone and a root stays a root (a node is compressed only after a value
// other than itself was read from its parent word, and it never becomes a root again). No floating-point atomics, no flags, no LDS.
__global__ __launch_bounds__(256) void cluster_link_kernel(const float4* __restrict__ spts, const float4* __restrict__ bbox1, const float4* __restrict__ bbox2, int n, float r2,
                                                           int* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= n) return;
  const float4 qv = spts[q];
  const float qx = read_lane(qv.x, 0), qy = read_lane(qv.y, 0), qz = read_lane(qv.z, 0);
  const int t0 = q >> 6, s0 = t0 >> 6;
  int rq = q;
  auto link = [&](const float4& p, int base) __attribute__((always_inline)) {
    const int c = base + lane;
    const bool hit = sqdist_nofma(p, qx, qy, qz) <= r2 && c < q;
    if (!__ballot(hit)) return;
    int rc = -1;
    if (hit) {
      int hops;
      rc = uf_find(parent, c, &hops);
      if (hops > 1) atomicMin(parent + c, rc);
    }
    unsigned long long todo = __ballot(hit && rc != rq);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      const int r = read_lane(rc, src);
      int nr = rq;
      if (lane == src) nr = uf_unite(parent, rq, r);
      rq = read_lane(nr, src);
      todo &= ~__ballot(rc == r || rc == rq);
      todo &= ~(1ull << src);
    }
  };
  link(load_candidate(spts, (t0 << 6) + lane, n), t0 << 6);
  for (int sc = 0; sc <= s0; sc += 64) {
    const int s = sc + lane;
    const float lb2 = (s <= s0) ? point_box_sq(bbox2[2 * s], bbox2[2 * s + 1], qx, qy, qz) : __builtin_inff();
    unsigned long long smask = __ballot(lb2 <= r2);
    while (smask) {
      const int ssrc = __ffsll((long long)smask) - 1;
      smask &= smask - 1;
      const int t = ((sc + ssrc) << 6) + lane;
      const float lb = (t < t0) ? point_box_sq(bbox1[2 * t], bbox1[2 * t + 1], qx, qy, qz) : __builtin_inff();
      unsigned long long tmask = __ballot(lb <= r2);
      if (!tmask) continue;
      int cur = __ffsll((long long)tmask) - 1;
      tmask &= tmask - 1;
      float4 pcur = load_candidate(spts, ((((sc + ssrc) << 6) + cur) << 6) + lane, n);
      while (true) {  // the next tile is in flight while this one is tested
        int nxt = -1;
        float4 pnxt = pcur;
        if (tmask) {
          nxt = __ffsll((long long)tmask) - 1;
          tmask &= tmask - 1;
          pnxt = load_candidate(spts, ((((sc + ssrc) << 6) + nxt) << 6) + lane, n);
        }
        link(pcur, (((sc + ssrc) << 6) + cur) << 6);
        if (nxt < 0) break;
        pcur = pnxt;
        cur = nxt;
      }
    }
  }
  if (lane == 0 && rq != q) atomicMin(parent + q, rq);  // the next find from q starts near the root
}

// After the link kernel (a kernel boundary: plain loads see every hook): the root of every sorted position, at the point's INPUT index;
// per root its component's size and smallest input index.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const float4* __restrict__ spts, int n, const int* __restrict__ parent, int* __restrict__ root_in, int* __restrict__ csize,
                                                              int* __restrict__ cmin) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int x = i, p = parent[x];
  while (p != x) { x = p; p = parent[x]; }
  const int own = __float_as_int(spts[i].w);
  root_in[own] = x;
  atomicAdd(csize + x, 1);
  atomicMin(cmin + x, own);
}

// input order: keep iff min_size <= size and (max_size <= 0 or size <= max_size); leader iff kept and the component's smallest input index; score = size
__global__ __launch_bounds__(256) void cluster_flag_kernel(int n, const int* __restrict__ root_in, const int* __restrict__ csize, const int* __restrict__ cmin, int min_size, int max_size,
                                                           unsigned* __restrict__ flags, unsigned* __restrict__ lead, float* __restrict__ score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r = root_in[i], s = csize[r];
  const bool keep = s >= min_size && (max_size <= 0 || s <= max_size);
  flags[i] = keep ? 1u : 0u;
  lead[i] = (keep && cmin[r] == i) ? 1u : 0u;
  score[i] = (float)s;
}

// lpos = exclusive scan of the leader flags: the cluster number of a kept component is lpos at its smallest input index
__global__ __launch_bounds__(256) void cluster_label_kernel(int n, const int* __restrict__ root_in, const int* __restrict__ csize, const int* __restrict__ cmin,
                                                            const unsigned* __restrict__ flags, const unsigned* __restrict__ lead, const unsigned* __restrict__ lpos,
                                                            const unsigned* __restrict__ total, int* __restrict__ labels, int* __restrict__ sizes, ClusterCtl* __restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) ctl->num_clusters = *total;
  if (i >= n) return;
  const int r = root_in[i];
  labels[i] = flags[i] ? (int)lpos[cmin[r]] : -1;
  if (lead[i]) sizes[lpos[i]] = csize[r];
}

}  // namespace fvh
