"""The contract of fvh_vgicp_target_from_map / fvh_ndt_target_from_map (include/fast_vgicp_hip.h), restated in numpy.

The handle's target cloud becomes one point per voxel of the live incremental map that holds at least min_points points: the voxel's float
mean (and, on VGICP handles, its record covariance as the target covariance), rows in ascending packed-key order -- z-major, then y, then
x: the row order of a map export. Everything here comes from the map's EXISTING getters (coords, counts, means, covs) and
tests/mapsnap_ref.key_order; nothing is taken from the call under test."""
import numpy as np

from tests import mapsnap_ref as S


def expected_rows(coords, counts, means, covs=None, min_points=1):
    """-> (rows, points (n, 3) float32, covariances (n, 3, 3) float32 or None): `rows` indexes the getters' arrays"""
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    counts = np.asarray(counts).reshape(-1)
    order = S.key_order(coords)
    rows = order[counts[order] >= max(int(min_points), 1)]  # (a voxel holds at least one point: min_points <= 1 takes all)
    pts = np.ascontiguousarray(np.asarray(means, np.float32).reshape(-1, 3)[rows])
    cov = None if covs is None else np.ascontiguousarray(np.asarray(covs, np.float32).reshape(-1, 3, 3)[rows])
    return rows, pts, cov


def from_voxelmap(vm, min_points=1, with_cov=True):
    """the same from the tuple VGICPCore.get_voxelmap() / NDTCore.get_voxelmap(1) returns"""
    coords, counts, means, covs = vm
    return expected_rows(coords, counts, means, covs if with_cov else None, min_points)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
