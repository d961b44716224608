"""The contract of the incremental target voxel map (include/fast_vgicp_hip.h: fvh_vgicp_map_*), restated in numpy.

An inserted point is p' = (float)(T p) and its covariance C' = (float)(R C R^T), both formed in fp64 and rounded to float32 once; the map
is then the map a batch build (set_target_cloud + set_target_covariances + create_target_voxelmap) makes of all inserted p', C'.
The voxel of a point is floor(p' / res - 0.5) per axis (fp64 of the float value); the centre of voxel c is (c + 1) * res."""
import numpy as np


def transform_cloud(P, C, T):
    """P (N, 3) float32, C (N, 3, 3) float32, T 4x4 -> (P', C') float32, products in fp64, rounded once."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    P64 = np.asarray(P, np.float32).astype(np.float64)
    C64 = np.asarray(C, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        Pp = (P64 @ R.T + t).astype(np.float32)
        Cp = (R @ C64 @ R.T).astype(np.float32)
    # the engine keeps the upper triangle of a covariance (xx xy xz yy yz zz): mirror it, so that every consumer sees one matrix
    iu = np.triu_indices(3)
    Cs = np.zeros_like(Cp)
    Cs[:, iu[0], iu[1]] = Cp[:, iu[0], iu[1]]
    Cs[:, iu[1], iu[0]] = Cp[:, iu[0], iu[1]]
    return Pp, Cs


def voxel_coords(Pp, res):
    """voxel coordinate of float32 points (rows with a non-finite / out-of-range coordinate: `ok` False)"""
    with np.errstate(invalid="ignore"):
        f = np.floor(np.asarray(Pp, np.float32).astype(np.float64) / res - 0.5)
        ok = np.all(np.abs(f) < (1 << 20) - 4096, axis=1)  # NaN compares False
    c = np.zeros(f.shape, np.int64)
    c[ok] = f[ok].astype(np.int64)
    return c, ok


def face_margin(P, T, res):
    """smallest distance, in voxels, of a transformed point (fp64) to a voxel face"""
    T = np.asarray(T, np.float64)
    q = np.asarray(P, np.float32).astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    fr = (q / res - 0.5) % 1.0
    return float(np.minimum(fr, 1.0 - fr).min())


def safe_pose(P, T, res_list, margin=1e-6, step=(1.0e-4, 2.0e-4, 3.0e-4), tries=64):
    """T, or T moved by the smallest multiple of the fixed `step` (metres) for which no transformed point lies within `margin` voxels of a
    voxel face at any resolution of `res_list`: a last-bit difference between two fp64 products then cannot move a point across a face"""
    T = np.array(T, np.float64)
    for k in range(tries):
        Tk = T.copy()
        Tk[:3, 3] += k * np.asarray(step)
        if all(face_margin(P, Tk, r) > margin for r in res_list):
            return Tk, k
    raise AssertionError("no pose within %d steps keeps every point %g voxels off the faces" % (tries, margin))


def voxel_centres(coords, res):
    return (np.asarray(coords, np.float64) + 1.0) * res


def prune_keep(coords, res, center, radius):
    """the distance rule of fvh_vgicp_map_prune: keep voxels whose centre is within `radius` of `center`; also the smallest |distance - radius|"""
    d = np.linalg.norm(voxel_centres(coords, res) - np.asarray(center, np.float64), axis=1)
    return d <= radius, float(np.abs(d - radius).min()) if len(d) else np.inf


def sorted_map(voxelmap):
    """(coords, num_points, means, covs) of a getter, rows in lexicographic coordinate order"""
    coords, num, means, covs = (np.asarray(a) for a in voxelmap)
    o = np.lexsort(coords.T[::-1]) if len(coords) else np.zeros(0, np.int64)
    return coords[o], num[o], means[o], covs[o]


def map_spread(a, b):
    """two maps with the same voxels: the largest differences of means and covariances in units of (1) the float32 spacing of the entry and
    (2) the voxel's scale (largest |mean| component; largest covariance diagonal)"""
    ca, na, ma, va = sorted_map(a)
    cb, nb, mb, vb = sorted_map(b)
    assert ca.shape == cb.shape and np.array_equal(ca, cb), "voxel coordinate sets differ (%d vs %d voxels)" % (len(ca), len(cb))
    assert np.array_equal(na, nb), "num_points differ in %d voxels" % int((na != nb).sum())
    out = {}
    for name, x, y, scale in (("mean", ma, mb, np.abs(mb).max(axis=1)[:, None]), ("cov", va.reshape(-1, 9), vb.reshape(-1, 9), np.abs(np.diagonal(vb, axis1=1, axis2=2)).max(axis=1)[:, None])):
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        d = np.abs(x64 - y64)
        ulp = np.spacing(np.maximum(np.abs(x), np.abs(y)).astype(np.float32)).astype(np.float64)
        out[name + "_ulps"] = float((d / ulp).max()) if d.size else 0.0
        out[name + "_rel_scale"] = float((d / np.maximum(scale, 1e-300)).max()) if d.size else 0.0
        # what is left once one float32 spacing of the entry is allowed, relative to the voxel's scale
        out[name + "_excess"] = float((np.maximum(d - ulp, 0.0) / np.maximum(scale, 1e-300)).max()) if d.size else 0.0
    return out
