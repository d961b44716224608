"""The contract of a map snapshot (include/fast_vgicp_hip.h: fvh_vgicp_voxelmap_export / _import / _merge_from), restated in numpy.

A snapshot is a dict: resolution, mode (0 additive, 2 multiplicative), num_inserts, num_points, num_voxels and per voxel coords (n, 3) int32,
sums (n, 10) float64 = {sum p | sum C^-1 p (3), sum C | sum C^-1 (6: xx xy xz yy yz zz), count}, ages (n,) uint32; rows in ascending
packed-key order."""
import numpy as np

COORD_BIAS = 1 << 20
COORD_LIMIT = COORD_BIAS - 4096  # |c| < this: the range voxel_index_ok gives an inserted point


def packed_key(coords):
    """the engine's voxel key: x in bits 0-20, y in 21-41, z in 42-62, each biased by 2^20 -- ascending keys are z-major, then y, then x"""
    c = np.asarray(coords, np.int64).reshape(-1, 3) + COORD_BIAS
    return (c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)).astype(np.uint64)


def key_order(coords):
    """the permutation that puts rows into snapshot order"""
    return np.argsort(packed_key(coords), kind="stable")


def empty_snapshot(resolution, mode):
    return dict(resolution=float(resolution), mode=int(mode), num_inserts=0, num_points=0, num_voxels=0, coords=np.zeros((0, 3), np.int32), sums=np.zeros((0, 10), np.float64),
                ages=np.zeros(0, np.uint32))


def merge(dst, inc):
    """`inc` added into `dst` as _import / _merge_from do it: union of keys, sums added in fp64 (dst + inc), num_inserts = max, num_points
    summed. Ages follow the stamps: a voxel's stamp is max(dst stamp, new num_inserts - inc age) with dst stamp = dst num_inserts - dst age,
    so the merged age is min(dst age + (new num_inserts - dst num_inserts), inc age): the smaller of the two ages once both count from the
    merged map's insert number (plain min(age, age) when the two maps have seen equally many inserts)."""
    assert dst["resolution"] == inc["resolution"] and dst["mode"] == inc["mode"]
    E = max(dst["num_inserts"], inc["num_inserts"])
    coords = np.concatenate([np.asarray(dst["coords"], np.int32).reshape(-1, 3), np.asarray(inc["coords"], np.int32).reshape(-1, 3)])
    sums_in = np.concatenate([np.asarray(dst["sums"], np.float64).reshape(-1, 10), np.asarray(inc["sums"], np.float64).reshape(-1, 10)])
    ages_in = np.concatenate([np.asarray(dst["ages"], np.int64) + (E - dst["num_inserts"]), np.asarray(inc["ages"], np.int64)])
    keys, first, inv = np.unique(packed_key(coords), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(keys), 10), np.float64)
    np.add.at(sums, inv, sums_in)  # (rows in order: dst's first -- 0 + a + b; with unique keys per map two operands, which commute)
    ages = np.full(len(keys), np.iinfo(np.int64).max)
    np.minimum.at(ages, inv, ages_in)
    return dict(resolution=dst["resolution"], mode=dst["mode"], num_inserts=E, num_points=dst["num_points"] + inc["num_points"], num_voxels=len(keys),
                coords=coords[first].astype(np.int32), sums=sums, ages=ages.astype(np.uint32))


def _full(c6):
    out = np.empty((len(c6), 3, 3), c6.dtype)
    for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[:, r, c] = c6[:, k]
        out[:, c, r] = c6[:, k]
    return out


def additive_records(sums):
    """(num_points int32, means float32, covs float32) of additive voxels: (float32)(sum * (1.0 / count)), the arithmetic of inc_write_record<0>"""
    s = np.asarray(sums, np.float64).reshape(-1, 10)
    inv = 1.0 / s[:, 9]
    return s[:, 9].astype(np.int32), (s[:, :3] * inv[:, None]).astype(np.float32), _full((s[:, 3:9] * inv[:, None]).astype(np.float32))


def multiplicative_records(sums):
    """multiplicative voxels: C = (sum C^-1)^-1, mean = C (sum C^-1 p), in fp64, rounded to float32"""
    s = np.asarray(sums, np.float64).reshape(-1, 10)
    C = np.linalg.inv(_full(s[:, 3:9]))
    return s[:, 9].astype(np.int32), np.einsum("nij,nj->ni", C, s[:, :3]).astype(np.float32), C.astype(np.float32)


def records(snapshot):
    """the getter's tuple (coords, num_points, means, covs) recomputed from a snapshot"""
    f = multiplicative_records if snapshot["mode"] == 2 else additive_records
    return (np.asarray(snapshot["coords"]),) + f(snapshot["sums"])


def same(a, b):
    """two snapshots are byte-equal"""
    return all(a[k] == b[k] for k in ("resolution", "mode", "num_inserts", "num_points", "num_voxels")) and all(
        np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
        for k in ("coords", "sums", "ages"))
