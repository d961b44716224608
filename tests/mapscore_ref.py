"""The contract of fvh_*_score_source / _score_cloud (include/fast_vgicp_hip.h: scoring a posed scan against the target voxel map), restated
operation by operation in plain Python.

Python floats are IEEE doubles and Python has no fused multiply-add, so every + - * / below is one correctly rounded fp64 operation, in the
association written; the float32 roundings go through numpy.float32. The map is what the voxel getters return: coords (V, 3) int, num_points
(V,), float32 means (V, 3) and float32 covariances (V, 3, 3). score() returns per-point rows and the counts; the three sums are math.fsum of
the per-point terms (the device adds them in a fixed tree: the tests hold it to the any-order summation bound).

Also here, because the CPU and the GPU tests share them: the synthetic scene (plane_scene) and numpy models of the three voxel types'
records (model_records), so that a scene can be shown to exercise every rule of the contract without a GPU."""
import math

import numpy as np

from tests.clearrays_ref import _index_ok, pose_parts, rounding_is_stable, transform_point  # noqa: F401  (rounding_is_stable: for the tests)

INF = float("inf")
NAN = float("nan")
DIRECT27, DIRECT7, DIRECT1 = 0, 1, 2  # fvh_neighbor_search

OFFSETS = {
    DIRECT1: [(0, 0, 0)],
    DIRECT7: [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
    DIRECT27: [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)],
}
COORD_BIAS = 1 << 20


def _coord_in_range(c):
    return all(0 <= v + COORD_BIAS < (1 << 21) for v in c)


def mahalanobis2(d, c6):
    """d: 3 Python floats; c6: (cxx, cxy, cxz, cyy, cyz, czz) Python floats. -> m2, +inf for a record that is not positive or not finite"""
    dx, dy, dz = d
    cxx, cxy, cxz, cyy, cyz, czz = c6
    a00 = cyy * czz - cyz * cyz
    a01 = cxz * cyz - cxy * czz
    a02 = cxy * cyz - cxz * cyy
    a11 = cxx * czz - cxz * cxz
    a12 = cxy * cxz - cxx * cyz
    a22 = cxx * cyy - cxy * cxy
    det = (cxx * a00 + cxy * a01) + cxz * a02
    q = (((dx * dx) * a00 + (dy * dy) * a11) + (dz * dz) * a22) + 2.0 * ((((dx * dy) * a01) + ((dx * dz) * a02)) + ((dy * dz) * a12))
    if not (det > 0.0) or not math.isfinite(det) or not math.isfinite(q):
        return INF
    m2 = q / det
    return 0.0 if m2 < 0.0 else m2


def score_of(score_scale, m2):
    return 0.0 if not (m2 < INF) else math.exp((-0.5 * score_scale) * m2)


def records_of(coords, num_points, means, covs):
    """the getters' arrays as {cell: (num_points, mean as 3 Python floats, c6 as 6 Python floats)}"""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    means = np.asarray(means, np.float32).reshape(-1, 3)
    covs = np.asarray(covs, np.float32).reshape(-1, 3, 3)
    out = {}
    for c, n, m, v in zip(coords.tolist(), np.asarray(num_points).reshape(-1).tolist(), means, covs):
        out[tuple(c)] = (int(n), tuple(float(x) for x in m), (float(v[0, 0]), float(v[0, 1]), float(v[0, 2]), float(v[1, 1]), float(v[1, 2]), float(v[2, 2])))
    return out


def score(records, res, points, T=None, neighbors=DIRECT7, min_points=1, max_m2=INF, score_scale=1.0):
    """records: records_of(...). points: (n, 3) float32 in the scan frame. -> dict: found, best (int32), best_m2 (float64), terms (n, 3), ties,
    singular_hits and the struct's fields (the sums by math.fsum)"""
    R, t = pose_parts(T)
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    found = np.full(n, -1, np.int32)
    best = np.full(n, -1, np.int32)
    best_m2 = np.full(n, NAN, np.float64)
    terms = np.zeros((n, 3), np.float64)
    n_used = n_in_voxel = n_near = n_explained = ties = singular_hits = 0
    offs = OFFSETS[neighbors]
    own = offs.index((0, 0, 0))
    for i, row in enumerate(pts):
        p = [float(v) for v in row]
        if not all(math.isfinite(v) for v in p):
            continue
        q = transform_point(R, t, p)
        f = [v / res - 0.5 for v in q]
        if not all(math.isfinite(v) for v in f):
            continue
        c = [float(math.floor(v)) for v in f]
        if not _index_ok(c):
            continue
        c = [int(v) for v in c]
        n_used += 1
        k, b, bm, in_own, all_sum, at_best = 0, -1, INF, False, 0.0, 0
        for o, (dx, dy, dz) in enumerate(offs):
            cell = (c[0] + dx, c[1] + dy, c[2] + dz)
            if not _coord_in_range(cell):
                continue
            rec = records.get(cell)
            if rec is None or (min_points > 1 and rec[0] < min_points):
                continue
            m2 = mahalanobis2((q[0] - rec[1][0], q[1] - rec[1][1], q[2] - rec[1][2]), rec[2])
            k += 1
            in_own = in_own or o == own
            singular_hits += 1 if m2 == INF else 0
            if b < 0 or m2 < bm:
                b, bm, at_best = o, m2, 1
            elif m2 == bm:
                at_best += 1
            all_sum = all_sum + score_of(score_scale, m2)
        found[i], best[i], best_m2[i] = k, b, bm
        n_in_voxel += 1 if in_own else 0
        if k > 0:
            n_near += 1
            ties += 1 if (at_best > 1 and bm < INF) else 0
            terms[i, 1] = score_of(score_scale, bm)
            if bm < INF and bm <= max_m2:  # (+inf explains nothing, whatever max_m2 is)
                n_explained += 1
                terms[i, 0] = bm
        terms[i, 2] = all_sum
    return dict(found=found, best=best, best_m2=best_m2, terms=terms, ties=ties, singular_hits=singular_hits, n_points=n, n_used=n_used, n_in_voxel=n_in_voxel, n_near=n_near,
                n_explained=n_explained, sum_best_m2=math.fsum(terms[:, 0].tolist()), sum_score_max=math.fsum(terms[:, 1].tolist()), sum_score_all=math.fsum(terms[:, 2].tolist()))


def sum_bounds(terms, extra=(0, 8, 8)):
    """what the device's three sums may differ from math.fsum by: (n + extra) * 2^-53 * sum |term| -- any order of n additions; the 8 of the
    score sums covers the device's and libm's exp, each within 1 ulp, taken twice over"""
    t = np.abs(np.asarray(terms, np.float64).reshape(-1, 3))
    return [(len(t) + extra[k]) * 2.0 ** -53 * math.fsum(t[:, k].tolist()) for k in range(3)]


# ---- the synthetic scene ------------------------------------------------------------------------------------------------------------------
SPD = np.array([[0.03125, 0.0078125, 0.0], [0.0078125, 0.0625, 0.00390625], [0.0, 0.00390625, 0.046875]])  # float32-exact
FLAT = np.diag([0.0625, 0.0625, 0.0])                                                                    # a REG_NONE coplanar patch: det == 0
# scan frame -> map frame: a quarter turn about z and a dyadic shift -- every product and sum of R p + t is exact
POSE = np.array([[0.0, -1.0, 0.0, 2.0], [1.0, 0.0, 0.0, -3.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
SPECIAL_ROWS = 12  # rows of plane_scene's scan that are made by hand


def _centre(c, res):
    return (np.asarray(c, np.float64) + 1.0) * res  # floor(x / res - 0.5) puts it in voxel c


def plane_scene(res=1.0, n=1000, seed=0):
    """-> dict(res, map_points (m, 3) float32, map_covs (m, 3, 3) float64, scan (n, 3) float32 in the scan frame, targets (n, 3) float32: where
    POSE puts the scan, pose). Map: an 8 x 8 ground plane of voxels (x, y, 0) with eight points each (cube corners), a second storey of SINGLE-point voxels over
    half of it, a flat (singular) eight-point voxel, a single-point voxel, and the same voxel twice either side of an empty cell. All
    coordinates are multiples of res / 16 and none of the scan's is 0 in the map frame. Scan rows 0 .. 11 are made by hand (below), the others are drawn around the plane."""
    rng = np.random.default_rng(seed)
    pts, covs = [], []

    def voxel(c, k, cov, spread=True):
        ctr = _centre(c, res)
        quad = np.array([[sx, sy, sz] for sx in (-0.25, 0.25) for sy in (-0.25, 0.25) for sz in (-0.25, 0.25)]) * res if spread else np.zeros((8, 3))  # cube corners: they sum to zero
        for j in range(k):
            pts.append(ctr + quad[j])
            covs.append(cov)

    for x in range(8):
        for y in range(8):
            voxel((x, y, 0), 8, SPD)
            if (x + y) % 2 == 0:
                voxel((x, y, 1), 1, SPD, spread=False)
    voxel((10, 0, 0), 8, FLAT, spread=False)   # eight times the same point with a flat covariance: singular for every voxel type (NDT: zero scatter)
    voxel((10, 3, 0), 1, FLAT, spread=False)   # ... and once: gone with min_points = 3
    voxel((12, 6, 0), 8, SPD)                  # the tie: the same voxel twice, two cells apart, the cell between them empty. Point counts
    voxel((14, 6, 0), 8, SPD)                  # of 8 keep every mean exact, so the two records differ by the shift alone
    targets = np.zeros((max(n, SPECIAL_ROWS), 3), np.float64)
    targets[0] = _centre((3, 4, 0), res) + np.array([0.125, -0.125, 0.0]) * res   # inside a plane voxel
    targets[1] = _centre((13, 6, 0), res)                                          # midway between the twin voxels: d and -d, the tie
    targets[2] = _centre((10, 0, 0), res) + np.array([0.125, 0.0, 0.0]) * res      # in the flat voxel
    targets[3] = _centre((10, 3, 0), res)                                          # in the single-point voxel
    targets[4] = (np.array([4.0, 4.0, 0.0]) + 0.5) * res                           # exactly on the corner of voxels: floor() decides, c = (4, 4, 0)
    targets[5] = _centre((3, 3, 2), res)                                           # above the second storey: near only through -z
    targets[6] = _centre((40, 40, 40), res)                                        # far from everything: used, nothing found
    targets[7] = _centre((3, 4, 0), res) + np.array([0.0, 0.0, 0.375]) * res       # off the plane inside its voxel: a large m2 (not explained)
    targets[8] = _centre((-1, 3, 0), res) + np.array([0.125, 0.0, 0.0]) * res                                          # beside the plane: near through +x only
    targets[9:12] = _centre((5, 5, 0), res)                                        # rows 9 .. 11 become NaN, +inf, and a cell beyond the index range
    if n > SPECIAL_ROWS:
        m = n - SPECIAL_ROWS
        cells = np.stack([rng.integers(-2, 10, m), rng.integers(-2, 10, m), rng.integers(-1, 4, m)], axis=1)
        targets[SPECIAL_ROWS:] = (cells + 1.0) * res + (2 * rng.integers(-3, 3, (m, 3)) + 1) / 16.0 * res  # odd multiples of res / 16: never 0
    R, t = POSE[:3, :3], POSE[:3, 3]
    scan = (targets - t) @ R  # R^T (q - t), exact
    scan[9, 0] = np.nan
    scan[10, 1] = np.inf
    targets[11] = np.array([float((1 << 20) - 4096), 5.0, 5.0]) * res + res  # c_x = 2^20 - 4096: the first index that is not ok
    scan[11] = R.T @ (targets[11] - t)
    targets[9:11] = np.nan
    return dict(res=res, map_points=np.array(pts, np.float32), map_covs=np.array(covs, np.float64), scan=scan[:n].astype(np.float32), targets=targets[:n].astype(np.float32), pose=POSE.copy())


def model_records(kind, res, points, covs):
    """numpy models of the voxel records a build of (points, covs) leaves: 'additive' (mean of points, mean of covariances), 'multiplicative'
    ((sum C^-1)^-1 and its mean), 'ndt' (scatter of the points, eigenvalues raised to 1e-3 of the largest). For the CPU tests: exact where sums
    are exact (the additive type on this module's scenes), a close model elsewhere -- the GPU tests take the records from the device."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    covs = np.asarray(covs, np.float64).reshape(-1, 3, 3)
    cells = np.floor(points / res - 0.5).astype(np.int64)
    groups = {}
    for i, c in enumerate(cells.tolist()):
        groups.setdefault(tuple(c), []).append(i)
    out = {}
    for c, idx in groups.items():
        p, C = points[idx], covs[idx]
        with np.errstate(all="ignore"):
            if kind == "additive":
                mean, cov = p.mean(axis=0), C.mean(axis=0)
            elif kind == "multiplicative":
                try:
                    Ci = np.linalg.inv(C)
                    cov = np.linalg.inv(Ci.sum(axis=0))
                    mean = cov @ np.einsum("nij,nj->i", Ci, p)
                except np.linalg.LinAlgError:
                    mean, cov = p.mean(axis=0), np.full((3, 3), np.nan)
            else:
                mean = p.mean(axis=0)
                d = p - mean
                cov = d.T @ d / len(idx)
                w, v = np.linalg.eigh(cov)
                w = np.maximum(w, 1e-3 * w.max())
                cov = (v * w) @ v.T
        m32, c32 = mean.astype(np.float32), cov.astype(np.float32)
        out[c] = (len(idx), tuple(float(x) for x in m32), (float(c32[0, 0]), float(c32[0, 1]), float(c32[0, 2]), float(c32[1, 1]), float(c32[1, 2]), float(c32[2, 2])))
    return out


def wrap_scene(capacity, res=1.0):
    """Voxels (one point each) that make probe sequences of a `capacity`-slot table cross its end: four whose home slot is the LAST one (they
    take slots capacity - 1, 0, 1, 2), two whose home is slot 0 (pushed further on), a dozen others -- and a fifth cell with the last home slot
    that stays EMPTY, so that the lookup of an absent key wraps too. Cells are three apart: no voxel is another's neighbour.
    -> dict(map_points, map_covs, scan (identity pose), absent (the empty cell), stats = table_sim.fill_table of the voxels)"""
    from tests import table_sim
    cands = np.array([(x, y, z) for z in (0, 3) for y in range(0, 90, 3) for x in range(0, 1500, 3)], np.int64)
    home = table_sim.hash_slot(table_sim.pack_key(cands), capacity)
    last, first = cands[home == capacity - 1], cands[home == 0]
    other = cands[(home > 8) & (home < capacity - 8)]
    assert len(last) >= 5 and len(first) >= 2 and len(other) >= 12, (capacity, len(last), len(first))
    voxels = np.concatenate([last[:4], first[:2], other[:12]])
    absent = last[4]
    pts = _centre(voxels, res)
    scan = np.concatenate([pts, pts + np.array([0.125, -0.125, 0.25]) * res, _centre(absent, res)[None], _centre(absent, res)[None] + 0.25 * res])
    return dict(res=res, voxels=voxels, map_points=pts.astype(np.float32), map_covs=np.repeat(SPD[None], len(pts), axis=0), scan=scan.astype(np.float32), absent=absent,
                stats=table_sim.fill_table(voxels, capacity))
