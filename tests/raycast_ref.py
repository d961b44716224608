"""The contract of fvh_*_cast_rays_source / _cast_rays_cloud (include/fast_vgicp_hip.h: ray casting into the target voxel map), restated
operation by operation in plain Python.

Python floats are IEEE doubles and Python has no fused multiply-add, so every + - * / below is one correctly rounded fp64 operation, in the
association written; the float32 roundings go through numpy.float32. The map is what the voxel getters return, as
tests/mapscore_ref.records_of arranges it. cast() returns the per-ray rows, the struct's counts and the counters the tests use to show that a
scene exercises every rule: clamped_low / clamped_high / interior (where the closest approach of a regular candidate fell), passed_through
(regular candidates whose m2 was above max_m2), singular (candidates whose record was singular for the ray) and ties (steps of used rays
where the smallest tMax was shared by two axes).

Also here, because the CPU and the GPU tests share it: the ray scene (ray_scene) over mapscore_ref.plane_scene's map."""
import math

import numpy as np

from tests.clearrays_ref import pose_parts, ray_setup, rounding_is_stable, transform_point  # noqa: F401  (rounding_is_stable: for the tests)
from tests.mapscore_ref import mahalanobis2, model_records, plane_scene, records_of, wrap_scene  # noqa: F401  (for the tests)
from tests.mapscore_ref import POSE, SPD, _centre

INF = float("inf")
NAN = float("nan")
COUNTERS = ("clamped_low", "clamped_high", "interior", "passed_through", "singular", "ties")
COUNTS = ("n_rays", "n_used", "n_hit", "n_hit_at_origin", "n_cells")


def bilinear(u, v, adj):
    a00, a01, a02, a11, a12, a22 = adj
    return (((u[0] * v[0]) * a00 + (u[1] * v[1]) * a11) + (u[2] * v[2]) * a22) + ((((u[0] * v[1] + u[1] * v[0]) * a01) + ((u[0] * v[2] + u[2] * v[0]) * a02)) + ((u[1] * v[2] + u[2] * v[1]) * a12))


def closest_approach(e, dm, lo, hi, c6):
    """the point of x(s) = e + s dm, s in [lo, hi], with the smallest squared Mahalanobis distance under c6 -> (s, m2, what): what is
    'singular', 'low', 'high' or 'interior'"""
    cxx, cxy, cxz, cyy, cyz, czz = c6
    a00 = cyy * czz - cyz * cyz
    a01 = cxz * cyz - cxy * czz
    a02 = cxy * cyz - cxz * cyy
    a11 = cxx * czz - cxz * cxz
    a12 = cxy * cxz - cxx * cyz
    a22 = cxx * cyy - cxy * cxy
    det = (cxx * a00 + cxy * a01) + cxz * a02
    adj = (a00, a01, a02, a11, a12, a22)
    with np.errstate(all="ignore"):
        den = bilinear(dm, dm, adj)
        num = bilinear(dm, e, adj)
    if not (det > 0.0) or not math.isfinite(det) or not (den > 0.0) or not math.isfinite(den) or not math.isfinite(num):
        return lo, INF, "singular"
    sstar = (-num) / den
    if sstar < lo:
        s, what = lo, "low"
    elif sstar > hi:
        s, what = hi, "high"
    else:
        s, what = sstar, "interior"
    x = (e[0] + s * dm[0], e[1] + s * dm[1], e[2] + s * dm[2])
    return s, mahalanobis2(x, c6), what


def walk_intervals(a, b):
    """the cells a ray from grid coordinate a to b visits, in order, with their parameter intervals: [(cell, t_in, t_out, tie)] -- the walk of
    clearrays_ref.walk with t_end = 1.0; tie: the step OUT of the cell had two axes at the smallest tMax"""
    c = [math.floor(v) for v in a]
    e = [math.floor(v) for v in b]
    d = [b[k] - a[k] for k in range(3)]
    s = [1 if v > 0.0 else (-1 if v < 0.0 else 0) for v in d]
    t_delta = [1.0 / abs(v) if v != 0.0 else INF for v in d]
    t_max = []
    for k in range(3):
        if d[k] > 0.0:
            t_max.append((float(c[k] + 1) - a[k]) / d[k])
        elif d[k] < 0.0:
            t_max.append((a[k] - float(c[k])) / (-d[k]))
        else:
            t_max.append(INF)
    n_steps = abs(e[0] - c[0]) + abs(e[1] - c[1]) + abs(e[2] - c[2])
    t_in, steps, out = 0.0, 0, []
    while t_in < 1.0:
        last = steps == n_steps
        if t_max[0] <= t_max[1] and t_max[0] <= t_max[2]:
            k = 0
        elif t_max[1] <= t_max[2]:
            k = 1
        else:
            k = 2
        t_next = t_max[k]
        t_out = 1.0 if (last or not t_next < 1.0) else t_next
        tie = (not last) and t_next < INF and sum(1 for v in t_max if v == t_next) > 1
        out.append(((c[0], c[1], c[2]), t_in, t_out, tie))
        if last:
            break
        t_in = t_next
        c[k] += s[k]
        t_max[k] += t_delta[k]
        steps += 1
    return out


def cast(records, res, points, T=None, origin=None, min_range=0.0, max_range=100.0, min_points=1, max_m2=INF):
    """records: records_of(...). points: (n, 3) float32 endpoints in the scan frame. -> dict: hit (int32), cell (n, 3) int32, range, m2
    (float64), the struct's counts and the coverage counters"""
    R, t = pose_parts(T)
    o32 = transform_point(R, t, (0.0, 0.0, 0.0) if origin is None else [float(v) for v in origin])
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    hit = np.full(n, -1, np.int32)
    cell = np.zeros((n, 3), np.int32)
    rng = np.full(n, NAN, np.float64)
    m2s = np.full(n, NAN, np.float64)
    cnt = dict.fromkeys(COUNTERS, 0)
    n_used = n_hit = n_origin = n_cells = 0
    for i, row in enumerate(pts):
        p = [float(v) for v in row]
        if not all(math.isfinite(v) for v in p):
            continue
        p32 = transform_point(R, t, p)
        ray = ray_setup(o32, p32, res, 0.0, max_range, 0.0)  # (min_range skips nothing here)
        if ray is None:
            continue
        a, b, _ = ray
        dm = [p32[k] - o32[k] for k in range(3)]
        r = math.sqrt((dm[0] * dm[0] + dm[1] * dm[1]) + dm[2] * dm[2])
        t_lo = min_range / r
        n_used += 1
        hit[i], rng[i], m2s[i] = 0, INF, INF
        cells = walk_intervals(a, b)
        for j, (c, t_in, t_out, tie) in enumerate(cells):
            n_cells += 1
            if not t_out > t_lo:
                cnt["ties"] += 1 if tie else 0
                continue
            rec = records.get(c)
            if rec is not None and not (min_points > 1 and rec[0] < min_points):
                lo = t_in if t_in > t_lo else t_lo
                e = (o32[0] - rec[1][0], o32[1] - rec[1][1], o32[2] - rec[1][2])
                s, m2, what = closest_approach(e, dm, lo, t_out, rec[2])
                if what == "singular":
                    cnt["singular"] += 1
                else:
                    cnt[{"low": "clamped_low", "high": "clamped_high", "interior": "interior"}[what]] += 1
                if m2 <= max_m2:
                    hit[i], cell[i], rng[i], m2s[i] = 1, c, s * r, m2
                    n_hit += 1
                    n_origin += 1 if c == cells[0][0] else 0
                    break
                if what != "singular":
                    cnt["passed_through"] += 1
            cnt["ties"] += 1 if tie else 0
    out = dict(hit=hit, cell=cell, range=rng, m2=m2s, n_rays=n, n_used=n_used, n_hit=n_hit, n_hit_at_origin=n_origin, n_cells=n_cells)
    out.update(cnt)
    return out


# ---- the ray scene ---------------------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = 14  # rows of ray_scene's endpoints that are made by hand
ORIGIN_GRID = np.array([4.0 + 17.0 / 32.0, 4.0 + 17.0 / 32.0, 6.0 + 9.0 / 32.0])  # the sensor in grid coordinates: above the plane, x and y the same way off their cell's edge
ORIGIN_INSIDE = np.array([3.0 + 17.0 / 32.0, 4.0 + 17.0 / 32.0, 9.0 / 32.0])      # ... inside plane voxel (3, 4, 0): ray_scene(inside=True), for n_hit_at_origin
TIGHT_CELL = (12, 2, 0)
NUM_VOXELS = 101  # plane_scene's 100 and the tight one
MAX_RANGE_VOXELS = 24.0  # ray_scene's max_range, in voxels


def _metric(g, res):
    return (np.asarray(g, np.float64) + 0.5) * res  # the metric point whose grid coordinate x / res - 0.5 is g


def ray_scene(res=1.0, n=1000, seed=0, pose=True, inside=False):
    """-> plane_scene's map plus dict(origin (3,) float64 in the scan frame, scan (n, 3) float32 endpoints in the scan frame, targets (n, 3):
    where the pose puts them, pose, max_range). The sensor sits above the 8 x 8 ground plane at grid coordinate ORIGIN_GRID; all finite
    endpoints are odd multiples of res / 32 in the map frame (never on a cell face), and with pose = POSE (or identity, pose=False) every
    product and sum of R p + t is exact. Rows 0 .. 13 are made by hand (below); the others end around and below the plane. inside: the sensor
    sits inside plane voxel (3, 4, 0) instead (the hand-made rows then mean nothing in particular)."""
    sc = plane_scene(res, 12, seed)
    # one voxel more than plane_scene has: eight points a sixteenth of a cell around the centre of cell (12, 2, 0) with SPD / 64 -- so
    # tight under every voxel type (at res 0.5 the additive records of the plane are wide enough to catch every ray that enters their cell)
    # that row 13, which crosses the cell a third of a cell off the mean, is passed through at max_m2 = 9
    tight = _centre(TIGHT_CELL, res) + np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * res / 16.0
    sc["map_points"] = np.concatenate([sc["map_points"], tight.astype(np.float32)])
    sc["map_covs"] = np.concatenate([sc["map_covs"], np.repeat(SPD[None] / 64.0, 8, axis=0)])
    rng = np.random.default_rng(seed)
    a = ORIGIN_INSIDE if inside else ORIGIN_GRID
    g = np.zeros((max(n, SPECIAL_ROWS), 3), np.float64)  # endpoints in grid coordinates
    g[0] = a + np.array([0.0, 0.0, -7.5])                      # axis-parallel: straight down through plane voxel (4, 4, 0), past its mean (interior)
    g[1] = a + np.array([-3.5, -3.5, -6.5])                    # the diagonal: x and y reach their cell faces together at every crossing (the tMax tie)
    g[2] = a + np.array([0.25, -0.125, 0.375])                 # ends in the origin's own cell (empty: no hit, one cell)
    g[3] = np.array([11.0 + 13.0 / 32.0, -3.0 / 32.0, -11.0 / 32.0])              # through the flat (singular) voxel (10, 0, 0), ending beyond it
    g[4] = np.array([11.0 + 13.0 / 32.0, 3.0 + 11.0 / 32.0, -11.0 / 32.0])        # through the single-point voxel (10, 3, 0): gone with min_points = 3
    g[5] = a + np.array([2.0, -3.0, 5.0])                      # upwards: misses everything
    g[6:11] = a + np.array([1.0, 1.0, -7.0])                   # rows 6 .. 10 become NaN, inf, r == 0, r > max_range and the index limit
    g[8] = a
    g[9] = a + np.array([0.0, MAX_RANGE_VOXELS + 1.0, 0.0])
    g[10] = np.array([float((1 << 20) - 4096) + 0.5, a[1], a[2]])  # cell 2^20 - 4096: the first index that is not ok
    g[11] = np.array([15.0 + 19.0 / 32.0, 6.0 + 21.0 / 32.0, 21.0 / 32.0])  # shallow, in through the far half of the top face of (14, 6, 0), moving away from its mean: clamped low
    g[12] = np.array([3.0 + 15.0 / 32.0, 4.0 + 17.0 / 32.0, 25.0 / 32.0])   # ends inside plane voxel (3, 4, 0) above its mean: clamped high
    g[13] = np.array([13.0 + 21.0 / 32.0, 1.0 + 31.0 / 32.0, -3.0 / 32.0])  # through the TIGHT voxel (12, 2, 0), a third of a cell off its mean: a regular record passed through
    if n > SPECIAL_ROWS:
        m = n - SPECIAL_ROWS
        cells = np.stack([rng.integers(-2, 10, m), rng.integers(-2, 10, m), rng.integers(-2, 3, m)], axis=1)
        g[SPECIAL_ROWS:] = cells + 0.5 + (2 * rng.integers(-8, 8, (m, 3)) + 1) / 32.0  # odd multiples of 1 / 32, inside the cell
    targets = _metric(g, res)
    o_map = _metric(a, res)
    T = POSE.copy() if pose else np.eye(4)
    R, t = T[:3, :3], T[:3, 3]
    scan = (targets - t) @ R  # R^T (q - t), exact
    origin = R.T @ (o_map - t)
    scan[6, 0] = np.nan
    scan[7, 2] = -np.inf
    targets[6:8] = np.nan
    sc.update(origin=origin, origin_map=o_map, scan=scan[:n].astype(np.float32), targets=targets[:n].astype(np.float32), pose=T, max_range=MAX_RANGE_VOXELS * res)
    return sc


def wrap_rays(w):
    """rays into a mapscore_ref.wrap_scene: from a sensor twenty cells above its first voxel to a point inside the cell of every voxel, a little
    past the mean, and to one inside the absent cell -> (endpoints float32, origin, max_range); identity pose, res 1, everything dyadic"""
    cells = np.concatenate([w["voxels"], w["absent"][None]]).astype(np.float64)
    origin = _metric(cells[0] + np.array([17.0 / 32.0, 17.0 / 32.0, 20.0 + 9.0 / 32.0]), 1.0)
    pts = _metric(cells + 0.5 + np.array([3.0 / 32.0, -5.0 / 32.0, -7.0 / 32.0]), 1.0)
    return pts.astype(np.float32), origin, 2048.0


def analytic_plane(res=1.0, n=500, seed=0, tilted=False):
    """A dense plane sampled into NDT-style records at `res`, and n oblique rays from 4.7 m above it. The plane is z = 1.62 res -- level, an
    eighth of a cell above the floor of its layer of cells, so that a range taken at the ENTRY of the hit cell would be most of a voxel short --
    or, tilted, z = 0.25 x + 0.125 y + 2, which also leaves slivers of the plane in the corners of cells.
    -> dict(records, origin, scan, ranges: the analytic range of every ray to the plane)"""
    rng = np.random.default_rng(seed)
    gx, gy, z0 = (0.25, 0.125, 2.0) if tilted else (0.0, 0.0, 1.62 * res)
    k = (np.arange(int(round(192 / res))) + 0.5) * res / 8.0 - 12.0  # a lattice an eighth of a cell apart, never on a cell face: 64 samples per full cell
    xy = np.stack(np.meshgrid(k, k, indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.column_stack([xy, gx * xy[:, 0] + gy * xy[:, 1] + z0])
    cells = np.floor(pts / res - 0.5).astype(np.int64)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    cells, pts = cells[order], pts[order]
    starts = np.flatnonzero(np.r_[True, (np.diff(cells, axis=0) != 0).any(axis=1)])
    rec = {}
    for lo, hi in zip(starts, np.r_[starts[1:], len(pts)]):
        if hi - lo < 6:
            continue
        p = pts[lo:hi]
        mean = p.mean(axis=0)
        d = p - mean
        cov = d.T @ d / (hi - lo)
        w, v = np.linalg.eigh(cov)
        w = np.maximum(w, 1e-3 * w.max())
        cov = ((v * w) @ v.T).astype(np.float32)
        m32 = mean.astype(np.float32)
        rec[tuple(int(x) for x in cells[lo])] = (int(hi - lo), tuple(float(x) for x in m32), (float(cov[0, 0]), float(cov[0, 1]), float(cov[0, 2]), float(cov[1, 1]), float(cov[1, 2]), float(cov[2, 2])))
    origin = np.array([0.3, -0.2, z0 + gx * 0.3 - gy * 0.2 + 4.7])
    foot = np.column_stack([rng.uniform(-6.0, 6.0, (n, 2)), np.zeros(n)])
    foot[:, 2] = gx * foot[:, 0] + gy * foot[:, 1] + z0
    d = foot - origin
    scan = (origin + 1.25 * d).astype(np.float32)  # the endpoint lies behind the plane
    o32 = origin.astype(np.float32).astype(np.float64)
    dd = scan.astype(np.float64) - o32
    nrm = np.array([gx, gy, -1.0])
    s = -(o32 @ nrm + z0) / (dd @ nrm)  # o + s d on the plane
    return dict(records=rec, origin=o32, scan=scan, ranges=s * np.linalg.norm(dd, axis=1))
