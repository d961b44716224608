"""The contract of the incremental NDT target map (include/fast_vgicp_hip.h: fvh_ndt_map_*), restated in numpy.

An inserted point is p' = (float)(T p), formed in fp64 and rounded to float32 once; its voxel is floor(p' / res - 0.5) per axis (fp64 of the
float value); a voxel holds the fp64 sums of the ten terms {p'x, p'y, p'z, p'x p'x, p'x p'y, p'x p'z, p'y p'y, p'y p'z, p'z p'z, 1} of its
points, the products being fp64 products of the float values. The map is then the map a batch build (set_target_cloud(all p') +
create_target_voxelmap) makes: mean = sum p / n, C = (sum p p^T - mean sum p^T) / n, MIN_EIG regularisation.
safe_pose, voxel_coords, prune_keep, sorted_map: tests/incmap_ref.py (the VGICP contract has the same geometry)."""
import numpy as np

from tests.incmap_ref import face_margin, prune_keep, safe_pose, sorted_map, voxel_coords  # noqa: F401  (one place to import the contract from)

EPS = 2.0 ** -53  # unit roundoff of fp64


def transform_points(P, T):
    """P (N, 3) float32, T 4x4 -> P' float32: R p + t in fp64, rounded once."""
    T = np.asarray(T, np.float64)
    P64 = np.asarray(P, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (P64 @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def point_terms(Pp):
    """(N, 10) fp64: the ten terms a point adds to its voxel"""
    q = np.asarray(Pp, np.float32).astype(np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z, np.ones(len(q))], axis=1)


def voxel_sums(Pp, res):
    """Per-voxel fp64 sums of float32 points, rows in ascending packed-key order (z-major, then y, then x: the order of a snapshot).
    -> dict(coords (V, 3) int32, sums (V, 10), abs_sums (V, 10): the same sums over |term|, delta (V,): see voxel_delta)"""
    c, ok = voxel_coords(Pp, res)
    q = np.asarray(Pp, np.float32).astype(np.float64)[ok]
    terms = point_terms(np.asarray(Pp, np.float32)[ok])
    uniq, inv = np.unique(c[ok], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.lexsort((uniq[:, 0], uniq[:, 1], uniq[:, 2]))
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    inv, uniq = rank[inv], uniq[order]
    sums, abs_sums, r2max = np.zeros((len(uniq), 10)), np.zeros((len(uniq), 10)), np.zeros(len(uniq))
    np.add.at(sums, inv, terms)
    np.add.at(abs_sums, inv, np.abs(terms))
    np.maximum.at(r2max, inv, (q * q).sum(axis=1))
    return dict(coords=uniq.astype(np.int32), sums=sums, abs_sums=abs_sums, delta=voxel_delta(sums[:, 9], r2max))


def voxel_delta(n, r2max):
    """delta_v = 8 n_v 2^-53 max |p'|^2: the bound on a RAW covariance entry (sum pp^T - mean sum p^T) / n when the order of the fp64 sums
    changes. Every summation order is within (n - 1) 2^-53 sum|x| of exact, so two orders differ by twice that: 2 n 2^-53 (n r2max) / n =
    2 n 2^-53 r2max per entry of sum pp^T / n; the cancellation against mean sum p^T / n (|mean| |sum p| / n <= r2max, formed from sums with the
    same relative error) adds the same again: 4 n 2^-53 r2max to first order. The contract's constant is 8: a factor 2 over that count for the
    roundings of the products and quotients themselves and the second-order terms."""
    return 8.0 * np.asarray(n, np.float64) * EPS * np.asarray(r2max, np.float64)


def sum_order_bound(n, abs_sums):
    """|one summation order - another| per entry: 2 (n - 1) 2^-53 sum|x|"""
    return 2.0 * np.maximum(np.asarray(n, np.float64) - 1.0, 0.0)[:, None] * EPS * abs_sums


def map_delta(coords, Pp, res):
    """delta_v for the voxels `coords` (any order) of the float32 cloud Pp"""
    ref = voxel_sums(Pp, res)
    index = {tuple(c): i for i, c in enumerate(ref["coords"])}
    return np.array([ref["delta"][index[tuple(c)]] for c in np.asarray(coords)])
