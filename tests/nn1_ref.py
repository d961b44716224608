"""The exact nearest-point search and the fitness mean AS A DEFINITION, in numpy, independent of the engine and of the oracle
(what nn1_rows_kernel + fitness_reduce_kernel of fast_gicp_amd/csrc/kernels_cov.hpp must compute; fast_gicp_impl.hpp:118-156,
pcl::Registration::getFitnessScore):

  query    = (x r0 + y r1) + (z r2 + t) per row, in float32, the pose cast fp64 -> fp32 first (transform_row_nofma)
  distance = (dx dx + dy dy) + dz dz in float32 (numpy never fuses a multiply into an add)
  nearest  = the minimum of the 64-bit key (float bits << 32) | ORIGINAL index: equal distances -> the lower index

and, below the definition, the clouds of the edge suite (tests/test_gpu_nn1_edges.py) -- built here so that tests/test_nn1_ref_cpu.py
checks on the CPU that each of them is the edge case it claims to be."""
import math

import numpy as np

MAX_DIST_DEFAULT = 3.4028234663852886e38   # the handle's default max correspondence distance (the reference's float max)
MAX_DIST_CLAMP = 1.8446743e19              # threshold^2 must stay finite in fp64
NO_POINT_IN_RANGE = 1.7976931348623157e308


def transform_f32(src, T):
    s = np.asarray(src, np.float32)
    Tf = np.asarray(T, np.float64).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (s[:, 0:1] * Tf[:3, 0] + s[:, 1:2] * Tf[:3, 1]) + (s[:, 2:3] * Tf[:3, 2] + Tf[:3, 3])
    return np.ascontiguousarray(q, np.float32)


def _sqdist_block(tgt, q):
    """(len(q), len(tgt)) float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = tgt[None, :, 0] - q[:, None, 0]
        dy = tgt[None, :, 1] - q[:, None, 1]
        dz = tgt[None, :, 2] - q[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def nearest(tgt, q, block_elems=1 << 21):
    """-> (idx int64, sq float32). NaN / inf in q are accepted: the result is whatever the key order gives (a NaN distance sorts above +inf);
    the caller turns a distance that is not finite into 'no correspondence'."""
    tgt = np.ascontiguousarray(tgt, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    nt, nq = len(tgt), len(q)
    assert nt >= 1 and tgt.shape[1] == 3 and q.shape[1] == 3
    idx = np.empty(nq, np.int64)
    sq = np.empty(nq, np.float32)
    ids = np.arange(nt, dtype=np.uint64)
    step = max(1, block_elems // nt)
    for a in range(0, nq, step):
        d = _sqdist_block(tgt, q[a:a + step])
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]
        k = key.min(axis=1)
        idx[a:a + step] = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        sq[a:a + step] = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, sq


def tie_count(tgt, q, sq, block_elems=1 << 21):
    """how many target points lie at exactly the minimum distance `sq` of each query"""
    tgt = np.ascontiguousarray(tgt, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    out = np.empty(len(q), np.int64)
    step = max(1, block_elems // len(tgt))
    for a in range(0, len(q), step):
        out[a:a + step] = (_sqdist_block(tgt, q[a:a + step]) == sq[a:a + step, None]).sum(axis=1)
    return out


def keep(idx, sq, max_dist=MAX_DIST_DEFAULT):
    thr = min(float(max_dist), MAX_DIST_CLAMP) ** 2
    with np.errstate(invalid="ignore"):
        return np.where(sq.astype(np.float64) < thr, idx, -1)   # strict (fast_gicp_impl.hpp:139); NaN and +inf compare false


def correspondences(tgt, src, T, max_dist=MAX_DIST_DEFAULT):
    idx, sq = nearest(tgt, transform_f32(src, T))
    return keep(idx, sq, max_dist)


def fitness(sq, max_range=NO_POINT_IN_RANGE):
    d = np.asarray(sq, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = d[d <= max_range]                                     # inclusive; NaN and (at the default range) +inf stay out
    return math.fsum(d.tolist()) / len(d) if len(d) else NO_POINT_IN_RANGE


def search(tgt, src, T, max_dist=MAX_DIST_DEFAULT):
    """one brute force for both answers of a pose -> (correspondences, nearest squared distances)"""
    idx, sq = nearest(tgt, transform_f32(src, T))
    return keep(idx, sq, max_dist), sq


# ---------------------------------------------------------------------------------------------------
# the clouds of the edge suite
# ---------------------------------------------------------------------------------------------------
SCALE = np.array([30.0, 30.0, 3.0])   # the anisotropic Gaussian of the existing nearest-point tests


def rigid(axis, angle_deg, t):
    """rotation by angle_deg about `axis` (Rodrigues) and the translation t, as a 4x4"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def pose_7deg_04m():
    t = np.array([0.3, -0.2, 0.1732050807568877])   # |t| = 0.4
    return rigid([0.2, -0.3, 1.0], 7.0, t)


def translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def gauss(n, seed):
    return (np.random.default_rng(seed).normal(size=(n, 3)) * SCALE).astype(np.float32)


SELF_SIZES = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8191, 8193, 32768, 32769)   # ends of rows, tiles, super tiles; both sort routes
SELF_BRUTE_FORCE_MAX = 8193


def self_cloud(n):
    """anisotropic Gaussian with n // 8 points rounded to integers (ties, a few duplicates) and n // 16 points copied onto other indices
    (duplicates at every size from 16 up) -> (cloud, the first index holding each point's coordinates)"""
    rng = np.random.default_rng(1000 + n)
    p = (rng.normal(size=(n, 3)) * SCALE).astype(np.float32)
    m = n // 8
    if m:
        sel = rng.choice(n, m, replace=False)
        p[sel] = np.rint(p[sel]) + np.float32(0.0)   # (+ 0: no -0.0, so equal coordinates are equal bits)
    if n // 16:
        to, frm = rng.choice(n, (2, n // 16), replace=False)
        p[to] = p[frm]
    _, first, inv = np.unique(p, axis=0, return_index=True, return_inverse=True)
    return p, first[np.asarray(inv).reshape(-1)].astype(np.int64)


def lattice(seed=16):
    g = np.arange(16, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


LATTICE_M = 1500   # queries per kind


def lattice_queries(seed=17):
    """-> dict kind -> queries: the lattice points themselves, then LATTICE_M each of cell centres (8 nearest points at distance^2 0.75 exactly),
    face centres (4 at 0.5) and edge midpoints (2 at 0.25) of cells drawn from ALL 16^3 base corners -- a cell on the upper boundary has fewer."""
    rng = np.random.default_rng(seed)
    out = {"points": lattice(seed=99)}   # (the same points in another order)
    for kind, half_axes in (("centres", 3), ("faces", 2), ("edges", 1)):
        base = rng.integers(0, 16, size=(LATTICE_M, 3)).astype(np.float32)
        for i in range(LATTICE_M):
            ax = rng.permutation(3)[:half_axes]
            base[i, ax] += 0.5
        out[kind] = base
    return out


LATTICE_WAYS = {"centres": 8, "faces": 4, "edges": 2}


def lattice_case():
    q = lattice_queries()
    return lattice(), np.concatenate([q["points"], q["centres"], q["faces"], q["edges"]])


def plane_case():
    rng = np.random.default_rng(21)
    def cloud(n):
        p = (rng.normal(size=(n, 3)) * SCALE).astype(np.float32)
        p[:, 2] = 1.25
        return p
    tgt, src = cloud(4097), cloud(2000)
    src[1000:, 2] += rng.normal(size=1000).astype(np.float32)   # half of the queries in the plane (every box has zero thickness), half off it
    return tgt, src


def line_case():
    rng = np.random.default_rng(22)
    tgt = np.zeros((4097, 3), np.float32)
    tgt[:, 0] = (rng.normal(size=4097) * 30.0).astype(np.float32)
    src = np.zeros((2000, 3), np.float32)
    src[:, 0] = (rng.normal(size=2000) * 30.0).astype(np.float32)
    src[1000:, 1:] = (rng.normal(size=(1000, 2)) * 2.0).astype(np.float32)
    return tgt, src


def identical_case():
    tgt = np.tile(np.array([[3.25, -7.5, 1.125]], np.float32), (1000, 1))
    src = np.concatenate([tgt[:300], gauss(300, 23)])
    return tgt, src


def offset_case():
    """the lattice 4,096 away from the origin on every axis (fp32 ulp 4.9e-4: distances are quantised), queries jittered by 0.3"""
    tgt = lattice() + np.float32(4096.0)
    src = (lattice(seed=98).astype(np.float64) + 4096.0 + np.random.default_rng(24).uniform(-0.3, 0.3, size=(4096, 3))).astype(np.float32)
    return tgt, src


def clusters_case():
    """2,048 + 2,049 points 1e4 apart, interleaved in index; queries in each cluster, midway, and at 1e6 (every bound is huge there and
    only the low mantissa bits order the candidates)"""
    rng = np.random.default_rng(25)
    far = np.array([1e4, 0.0, 0.0])
    tgt = np.empty((4097, 3), np.float32)
    tgt[0::2] = (rng.normal(size=(2049, 3)) * SCALE).astype(np.float32)
    tgt[1::2] = (rng.normal(size=(2048, 3)) * SCALE + far).astype(np.float32)
    src = np.concatenate([rng.normal(size=(800, 3)) * SCALE, rng.normal(size=(800, 3)) * SCALE + far,
                          rng.normal(size=(400, 3)) * SCALE + far / 2, rng.normal(size=(400, 3)) * SCALE + np.array([1e6, 0.0, 0.0]),
                          rng.normal(size=(400, 3)) * SCALE + np.array([-5e5, 7e5, 1e6])]).astype(np.float32)
    return tgt, src


BAD_ROWS = {20: [np.nan, 0.0, 0.0], 21: [np.inf, 0.0, 0.0], 22: [0.0, -np.inf, 1.0], 23: [1.0, 2.0, np.nan], 64: [1e30, 0.0, 0.0], 65: [0.0, 0.0, -1e30],
            66: [np.nan, np.nan, np.nan], 130: [np.inf, -np.inf, 0.0]}
NEG_ZERO_ROWS = (24, 131)


def bad_case():
    """finite target; a source with NaN, +-inf and 1e30 rows (no correspondence, outside the fitness mean) and two rows of -0.0 (a query like any other)"""
    tgt = gauss(4097, 26)
    tgt[7] = 0.0
    src = gauss(200, 27)
    for i, row in BAD_ROWS.items():
        src[i] = row
    for i in NEG_ZERO_ROWS:
        src[i] = [-0.0, -0.0, -0.0]
    return tgt, src


STRUCTURED = {"lattice": lattice_case, "plane": plane_case, "line": line_case, "identical": identical_case, "offset": offset_case,
              "clusters": clusters_case, "bad": bad_case}


def twin_case():
    """-> (target A, target B, source, P). A: point 5 moved 1e3 away, point 900 at P. B: A with point 5 at P as well (the lower-index twin).
    200 queries within 1e-3 of P, the first eight ON P (distance 0 to both twins: the bound of their box then EQUALS the seed's distance);
    no other target point within 0.5 of P."""
    rng = np.random.default_rng(31)
    P = np.array([2.5, -1.25, 0.75], np.float32)
    A = gauss(5000, 32)
    A = A[np.abs(A - P).max(axis=1) > 0.5][:4000].copy()
    A[5] = [1e3, 1e3, 1e3]
    A[900] = P
    B = A.copy()
    B[5] = P
    src = (P.astype(np.float64) + rng.uniform(-1e-3, 1e-3, size=(200, 3))).astype(np.float32)
    src[:8] = P
    return A, B, src, P


THRESHOLD_MAX_DISTS = (0.5, float(np.nextafter(0.5, 1.0)), MAX_DIST_DEFAULT)


def threshold_case():
    """one target point at the origin and 63 far away; queries on the x axis at 0.5 and one fp32 step to either side"""
    tgt = np.zeros((64, 3), np.float32)
    tgt[1:] = gauss(63, 33) + np.float32(500.0)
    h = np.float32(0.5)
    src = np.zeros((3, 3), np.float32)
    src[:, 0] = [h, np.nextafter(h, np.float32(0)), np.nextafter(h, np.float32(1))]
    return tgt, src


REDUCE_SIZES = (1, 1023, 1024, 1025, 4095, 4096, 4097, 8193)


def reduce_case(n):
    """source i at x = k 2^-12 with k = (i % 4093) + 1: every squared distance to the origin (k^2 2^-24, k^2 < 2^24) is exact in fp32 and
    every partial sum exact in fp64 -> (source, k, the exact fitness mean as one correctly rounded division)"""
    k = (np.arange(n, dtype=np.int64) % 4093) + 1
    src = np.zeros((n, 3), np.float32)
    src[:, 0] = (k.astype(np.float64) * 2.0 ** -12).astype(np.float32)
    total = int((k * k).sum())
    assert total < 2 ** 53
    return src, k, (total * 2.0 ** -24) / n
