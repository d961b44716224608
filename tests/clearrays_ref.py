"""The contract of fvh_*_clear_rays_* (include/fast_vgicp_hip.h: free-space carving), restated operation by operation in plain Python.

Python floats are IEEE doubles and Python has no fused multiply-add, so every + - * / below is one correctly rounded fp64 operation, in the
association written; the float32 roundings go through numpy.float32. The map is an exported snapshot {coords, sums, ages, ...}: clear_rays()
returns the snapshot the device must hold afterwards (same rows minus the removed ones, survivors untouched) and the two counts."""
import math

import numpy as np

LIM = (1 << 20) - 4096  # voxel_index_ok: |floor| < 2^20 - 4096
INF = float("inf")


def _f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(v))


def transform_point(R, t, p):
    """(float)(R p + t) per axis: ((r0 x + r1 y) + r2 z) + t in fp64, rounded once"""
    return tuple(_f32(((R[a][0] * p[0] + R[a][1] * p[1]) + R[a][2] * p[2]) + t[a]) for a in range(3))


def pose_parts(T):
    T = np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4)
    return [[float(T[a, j]) for j in range(3)] for a in range(3)], [float(T[a, 3]) for a in range(3)]


def rounding_is_stable(T, points, origin=None):
    """True when no (float)(R p + t) of `points` (and of the origin) can depend on HOW the fp64 sum is formed -- the kernel's compiler may
    contract products into sums, which moves the fp64 value by a few 2^-53 of the largest term: the float32 rounding must be the same 2^-48
    of the terms' magnitude to either side. (With a pose whose products and sums are exact -- identity, dyadic translations -- it always is.)"""
    R, t = pose_parts(T)
    rows = [tuple(float(v) for v in p) for p in np.asarray(points, np.float32).reshape(-1, 3)]
    rows.append((0.0, 0.0, 0.0) if origin is None else tuple(float(v) for v in origin))
    for p in rows:
        if not all(math.isfinite(v) for v in p):
            continue
        for a in range(3):
            q = ((R[a][0] * p[0] + R[a][1] * p[1]) + R[a][2] * p[2]) + t[a]
            m = (abs(R[a][0] * p[0]) + abs(R[a][1] * p[1]) + abs(R[a][2] * p[2]) + abs(t[a])) * 2.0 ** -48
            if not (_f32(q - m) == _f32(q) == _f32(q + m)):
                return False
    return True


def _floor(v):
    return float(math.floor(v)) if math.isfinite(v) else v


def _index_ok(f):
    return all(abs(v) < LIM for v in f)  # False for NaN


def ray_setup(o32, p32, res, min_range, max_range, end_margin):
    """o32, p32: the float32 origin and endpoint in the map frame (as Python floats). -> None for a skipped ray, else (a, b, t_end):
    the grid coordinates of the two ends and where the walk stops"""
    a = [v / res - 0.5 for v in o32]
    b = [v / res - 0.5 for v in p32]
    dm = [p32[k] - o32[k] for k in range(3)]
    with np.errstate(all="ignore"):
        s = (dm[0] * dm[0] + dm[1] * dm[1]) + dm[2] * dm[2]
    r = math.sqrt(s) if s >= 0.0 else float("nan")
    if r == 0.0 or r < min_range or r > max_range:
        return None
    if not _index_ok([_floor(v) for v in a]) or not _index_ok([_floor(v) for v in b]):
        return None
    return a, b, 1.0 - end_margin / r


def walk(a, b, t_end):
    """the cells a ray from grid coordinate a to b crosses before t_end, in order (Amanatides-Woo, one axis per step, at most N + 1 cells)"""
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
    while True:
        if not t_in < t_end:
            break
        out.append((c[0], c[1], c[2]))
        if steps == n_steps:
            break
        if t_max[0] <= t_max[1] and t_max[0] <= t_max[2]:
            k = 0
        elif t_max[1] <= t_max[2]:
            k = 1
        else:
            k = 2
        t_in = t_max[k]
        c[k] += s[k]
        t_max[k] += t_delta[k]
        steps += 1
    return out


def clear_rays(snapshot, points, T=None, origin=None, min_range=0.0, max_range=100.0, end_margin=0.0, min_misses=1):
    """-> (the snapshot after the call, voxels removed, rays used). points: (n, 3) float32 in the scan frame."""
    res = float(snapshot["resolution"])
    R, t = pose_parts(T)
    o32 = transform_point(R, t, (0.0, 0.0, 0.0) if origin is None else [float(v) for v in origin])
    coords = np.asarray(snapshot["coords"], np.int32).reshape(-1, 3)
    index = {(int(c[0]), int(c[1]), int(c[2])): i for i, c in enumerate(coords)}
    misses = [0] * len(coords)
    hit = [False] * len(coords)
    used = 0
    for row in np.asarray(points, np.float32).reshape(-1, 3):
        p = [float(v) for v in row]
        if not all(math.isfinite(v) for v in p):
            continue
        ray = ray_setup(o32, transform_point(R, t, p), res, min_range, max_range, end_margin)
        if ray is None:
            continue
        used += 1
        a, b, t_end = ray
        i = index.get(tuple(math.floor(v) for v in b))
        if i is not None:
            hit[i] = True
        for cell in walk(a, b, t_end):
            i = index.get(cell)
            if i is not None:
                misses[i] += 1
    keep = np.array([not (misses[i] >= min_misses and not hit[i]) for i in range(len(coords))], bool).reshape(-1)
    out = dict(snapshot)
    out["coords"] = coords[keep]
    out["sums"] = np.asarray(snapshot["sums"], np.float64).reshape(-1, 10)[keep]
    out["ages"] = np.asarray(snapshot["ages"], np.uint32).reshape(-1)[keep]
    out["num_voxels"] = int(keep.sum())
    return out, int(len(coords) - keep.sum()), used
