"""Independent numpy restatement of the oracle's core formulas (test infrastructure only): a second,
differently-written implementation so that the C++ oracle is not its own judge (SURVEY 8c 'oracle plan')."""
import numpy as np


def regularize(C, reg):
    if reg == 0:
        return C
    if reg == 4:
        Ci = np.linalg.inv(C + 1e-3 * np.eye(3))
        return np.linalg.inv(Ci / np.linalg.norm(Ci))
    w, V = np.linalg.eigh(C)
    if reg == 3:
        d = np.array([1e-3, 1.0, 1.0])
    elif reg == 1:
        d = np.maximum(w, 1e-3)
    else:
        d = np.maximum(w / w[2], 1e-3)
    return (V * d) @ V.T


def covariances(xyz, idx, reg):
    p = xyz.astype(np.float64)
    out = np.empty((len(p), 3, 3))
    for i in range(len(p)):
        nb = p[idx[i]]
        d = nb - nb.mean(axis=0)
        out[i] = regularize(d.T @ d / idx.shape[1], reg)
    return out


def voxelmap(xyz, covs, res):
    p = xyz.astype(np.float64)
    keys = np.floor(p / res - 0.5).astype(np.int64)
    vm = {}
    for k, pt, c in zip(map(tuple, keys), p, covs):
        n, m, cc = vm.get(k, (0, np.zeros(3), np.zeros((3, 3))))
        vm[k] = (n + 1, m + pt, cc + c)
    return {k: (n, m / n, c / n) for k, (n, m, c) in vm.items()}


def skew(x):
    return np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])


def inv3(A):
    """3x3 inverse written out as adjugate / determinant (rows of the cofactor matrix are cross products of the rows of A): works in any
    dtype, np.longdouble included, where np.linalg.inv does not"""
    r0, r1, r2 = A
    cof = np.array([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)])
    return cof.T / (r0 @ cof[0])


def _jacobian(q, dtype):
    return np.hstack([skew(q).astype(dtype), -np.eye(3, dtype=dtype)])


def _transformed(pts, T, res, dtype):
    T = np.asarray(T, dtype)
    R, t = T[:3, :3], T[:3, 3]
    with np.errstate(invalid="ignore"):  # (non-finite points)
        q = np.asarray(pts).astype(dtype) @ R.T + t
        f = np.floor(q / dtype(res) - dtype(0.5))
    # a non-finite or absurdly far point has no voxel (and no integer coordinate): it is given one nobody can hold
    ok = np.isfinite(f).all(axis=1) & (np.abs(np.where(np.isfinite(f), f, 0)) < 2.0 ** 40).all(axis=1)
    coords = np.where(ok[:, None], np.where(np.isfinite(f), f, 0), 2.0 ** 40).astype(np.int64)
    return R, q, coords


def linearize(src, src_covs, vm, res, offsets, T, dtype=np.float64):
    """VGICP sums at pose T: every (source point, occupied neighbour voxel) pair, weight sqrt(points in the voxel),
    M = (C_voxel + R C_point R^T)^-1. -> err, H, b, number of pairs. dtype: np.float64 or np.longdouble (tolerance measurements)."""
    R, q, coords = _transformed(src, T, res, dtype)
    covs = np.asarray(src_covs).astype(dtype)
    H = np.zeros((6, 6), dtype); b = np.zeros(6, dtype); err = dtype(0); nc = 0
    for i in range(len(q)):
        for o in offsets:
            v = vm.get(tuple(coords[i] + o))
            if v is None:
                continue
            n, mu, Cb = v
            M = inv3(np.asarray(Cb).astype(dtype) + R @ covs[i] @ R.T)
            e = np.asarray(mu).astype(dtype) - q[i]
            w = np.sqrt(dtype(n))
            J = _jacobian(q[i], dtype)
            err += w * (e @ M @ e)
            H += w * (J.T @ M @ J)
            b += w * (J.T @ M @ e)
            nc += 1
    return err, H, b, nc


def ndt_linearize(src, src_records, vm, res, offsets, T, d2d, dtype=np.float64):
    """NDT sums at pose T over a target map `vm` {coord: (n, mean, cov)}. P2D (d2d False): the elements are the points `src`, M = C_voxel^-1.
    D2D: the elements are the source voxels `src_records` (a sequence of (n, mean, cov); `src` is not used): the voxel's mean stands for the
    point and M = (C_voxel + R C_source R^T)^-1. Every pair is weighted by the Cauchy kernel res^2 / (res^2 + |e|^2); target voxels of at most
    6 points are looked up -- they count as correspondences -- but contribute nothing. -> err, H, b, number of correspondences."""
    if d2d:
        pts = np.array([np.asarray(r[1]) for r in src_records]).reshape(-1, 3)
        scov = [np.asarray(r[2]).astype(dtype) for r in src_records]
    else:
        pts = src
    R, q, coords = _transformed(pts, T, res, dtype)
    k2 = dtype(res) * dtype(res)
    H = np.zeros((6, 6), dtype); b = np.zeros(6, dtype); err = dtype(0); nc = 0
    for i in range(len(q)):
        for o in offsets:
            v = vm.get(tuple(coords[i] + o))
            if v is None:
                continue
            nc += 1
            n, mu, Cb = v
            if n <= 6:
                continue
            Cb = np.asarray(Cb).astype(dtype)
            M = inv3(Cb + R @ scov[i] @ R.T) if d2d else inv3(Cb)
            e = np.asarray(mu).astype(dtype) - q[i]
            w = k2 / (k2 + e @ e)
            J = _jacobian(q[i], dtype)
            err += w * (e @ M @ e)
            H += w * (J.T @ M @ J)
            b += w * (J.T @ M @ e)
    return err, H, b, nc
