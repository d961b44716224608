"""The contract of a posed map merge (include/fast_vgicp_hip.h: fvh_*_posed_merge_from / fvh_*_transform_map), restated in numpy,
and the inputs the CPU and GPU tests of it share.

A snapshot row {coords, sums[10], age} of a map seen from pose T = (R, t) becomes, in fp64 (n = sums[9]; the six stored entries of a
symmetric matrix are its upper triangle xx xy xz yy yz zz):
    additive       (snapshot mode 0): sp' = R sp + n t          SC' = R SC R^T
    multiplicative (mode 2)         : A'  = R A R^T             b'  = R b + A' t
    NDT sums       (mode 3), u = R sp: sp' = u + n t            S'  = R S R^T + u t^T + t u^T + n t t^T
with every expression associated as _formulas writes it (the kernel writes them the same way: where every product is exact -- R of 0 / +-1,
t of whole numbers -- the two agree to the bit whether or not a product and a sum are fused). The row then goes to the voxel of ITS OWN
float32 mean m' (additive / NDT: (float)(sp' * (1 / n)); multiplicative: (float)(A'^-1 b')): coord = floor((double)m' / res - 0.5), skipped when
|coord| >= 2^20 - 4096.

The bound on |device sum - twin sum| (derived, not measured). u = 2^-53. An entry of R S R^T is two nested dot products of length 3: 2
roundings per product pair and 2 additions each, i.e. at most 8 roundings on any path from an input to the result; the NDT terms add three
products of up to 3 factors (u_r itself carries the 3 roundings of its dot product) and 3 additions, the first moments one dot product of
length 3 (or 6: the multiplicative b') -- every entry is a sum of products with at most 16 roundings on a path, so by the standard bound for
sums of products (Higham, Accuracy and Stability, section 3.1: |fl - exact| <= gamma_k sum |terms|, gamma_k = k u / (1 - k u)) each evaluation
is within 16 u abs_bound of the exact value, abs_bound being the same formulas evaluated with |R|, |t|, |sums|. Fusing a product and a sum
removes a rounding and never adds one. A voxel that k rows land in then receives k fp64 atomic adds in some order, on top of what it held:
at most k more roundings of a partial sum bounded by the voxel's abs_bound (|what it held| + the rows' abs_bounds). The contract's
constant is gamma = 64 + k: four times the count for the evaluation, plus the adds. Device and twin are each within gamma u abs_bound of the
exact value, hence within 2 gamma u abs_bound of each other."""
import numpy as np

from tests import mapsnap_ref as S

EPS = 2.0 ** -53
GAMMA0 = 64.0


def _formulas(R, t, s, mode):
    """(N, 10) transformed sums of rows s under (R, t); mode: the snapshot's (0, 2, 3)"""
    n = s[:, 9]
    a = [s[:, 0], s[:, 1], s[:, 2]]
    Sm = [[s[:, 3], s[:, 4], s[:, 5]], [s[:, 4], s[:, 6], s[:, 7]], [s[:, 5], s[:, 7], s[:, 8]]]
    u = [(R[r, 0] * a[0] + R[r, 1] * a[1]) + R[r, 2] * a[2] for r in range(3)]
    M = [[(R[r, 0] * Sm[0][c] + R[r, 1] * Sm[1][c]) + R[r, 2] * Sm[2][c] for c in range(3)] for r in range(3)]
    Q = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(r, 3):
            Q[r][c] = (M[r][0] * R[c, 0] + M[r][1] * R[c, 1]) + M[r][2] * R[c, 2]
            Q[c][r] = Q[r][c]
    if mode == 2:
        o = [((u[r] + Q[r][0] * t[0]) + Q[r][1] * t[1]) + Q[r][2] * t[2] for r in range(3)]
    else:
        o = [u[r] + n * t[r] for r in range(3)]
    if mode == 3:
        for r in range(3):
            for c in range(r, 3):
                Q[r][c] = ((Q[r][c] + u[r] * t[c]) + t[r] * u[c]) + (n * t[r]) * t[c]
    return np.stack(o + [Q[0][0], Q[0][1], Q[0][2], Q[1][1], Q[1][2], Q[2][2], n], axis=1)


def row_means(sums, mode):
    """the float32 mean the record arithmetic gives each row of sums on its own"""
    s = np.asarray(sums, np.float64).reshape(-1, 10)
    if len(s) == 0:
        return np.zeros((0, 3), np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if mode == 2:
            return S.multiplicative_records(s)[1]
        return (s[:, :3] * (1.0 / s[:, 9])[:, None]).astype(np.float32)


def transform_rows(snapshot, T, guard=1.0):
    """-> (coords (N, 3) int32, sums (N, 10), ages (N,), skipped_mask (N,), abs_bound (N, 10), near_face (N,)).
    coords of a skipped row are 0. near_face: (double)m' / res - 0.5 lies within guard * 4 * 2^-23 * max(1, |m'|) / res of an integer on
    some axis -- a last-bit difference in the float mean could move such a row to the neighbouring voxel."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    res, mode = float(snapshot["resolution"]), int(snapshot["mode"])
    s = np.asarray(snapshot["sums"], np.float64).reshape(-1, 10)
    ages = np.asarray(snapshot["ages"], np.uint32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        out = _formulas(R, t, s, mode)
        bound = _formulas(np.abs(R), np.abs(t), np.abs(s), mode)
        m = row_means(out, mode).astype(np.float64)
        x = m / res - 0.5
        f = np.floor(x)
        ok = np.all(np.abs(f) < S.COORD_LIMIT, axis=1)  # NaN compares False
        dist = np.abs(x - np.round(x))
        lim = guard * 4.0 * 2.0 ** -23 * np.maximum(1.0, np.linalg.norm(m, axis=1)) / res
        near = ok & np.any(dist <= lim[:, None], axis=1)
    coords = np.zeros((len(s), 3), np.int32)
    coords[ok] = f[ok].astype(np.int32)
    return coords, out, ages, ~ok, bound, near


def posed_merge(dst, inc, T):
    """`inc` seen from pose T added into `dst` -> (merged snapshot, info). info: rows_skipped, skipped_points, and per merged voxel `landed`
    (rows of inc that arrived in it) and `abs_bound` (|what dst held| + the arrived rows' abs_bounds), near_face (rows of inc)."""
    assert dst["resolution"] == inc["resolution"] and dst["mode"] == inc["mode"]
    coords, sums, ages, skipped, bound, near = transform_rows(inc, T)
    keep = ~skipped
    moved = dict(inc, coords=coords[keep], sums=sums[keep], ages=ages[keep], num_voxels=int(keep.sum()))
    out = S.merge(dst, moved)
    keys = S.packed_key(out["coords"])
    landed = np.zeros(len(keys), np.int64)
    ab = np.zeros((len(keys), 10))
    at = np.searchsorted(keys, S.packed_key(np.asarray(dst["coords"]).reshape(-1, 3)))
    ab[at] += np.abs(np.asarray(dst["sums"], np.float64).reshape(-1, 10))
    at = np.searchsorted(keys, S.packed_key(coords[keep]))
    np.add.at(landed, at, 1)
    np.add.at(ab, at, bound[keep])
    return out, dict(rows_skipped=int(skipped.sum()), skipped_points=int(np.asarray(inc["sums"]).reshape(-1, 10)[skipped, 9].sum()), landed=landed, abs_bound=ab,
                     near_face=near)


def sums_tolerance(info):
    """2 gamma 2^-53 abs_bound per merged voxel and sum, gamma = 64 + rows landed (the module's docstring derives it)"""
    return 2.0 * (GAMMA0 + info["landed"])[:, None] * EPS * info["abs_bound"]


# ---- the inputs the CPU and GPU tests share --------------------------------------------------------------------------------------------
RES = 1.0
KINDS = {"additive": 0, "ndt": 3, "multiplicative": 2}  # test id -> snapshot mode


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


IDENTITY = np.eye(4)
EXACT = pose(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), [3.0, -2.0, 1.0])  # 90 degrees about z + whole voxels
GENERAL = pose(_rot([1.0, 2.0, 3.0], 35.0), [0.37, -1.21, 0.53])  # tilted axis, non-lattice translation
SECOND = pose(_rot([2.0, -1.0, 1.0], 20.0), [-0.81, 0.443, 0.307])  # what map_transform moves an already merged map by
DIAGONAL = pose(_rot([0.0, 0.0, 1.0], 45.0), [0.1, 0.2, 0.3])
FAR = pose(np.eye(3), [float(1 << 20) * RES, 0.0, 0.0])  # every row beyond the key range
EDGE_SIZES = (0, 1, 255, 256, 257)


def covariances(n, seed):
    """(n, 3, 3) float32 symmetric positive definite covariances, eigenvalues within about [1e-3, 0.05]"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, 3, 3)) * 0.08
    C = (A @ np.transpose(A, (0, 2, 1)) + 1e-3 * np.eye(3)).astype(np.float32)
    iu = np.triu_indices(3)
    C[:, iu[1], iu[0]] = C[:, iu[0], iu[1]]
    return C


def cloud_covariances(P):
    """the covariances the tests give a synthetic cloud"""
    return covariances(len(P), 7)


def voxel_cloud(n_voxels, seed, per_voxel=3):
    """points of exactly n_voxels voxels at RES: distinct cells of a 12 x 12 x 4 block, 1..per_voxel points each within 0.3 voxels of the centre"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(12 * 12 * 4)[:n_voxels]
    c = np.stack([cells % 12 - 6, (cells // 12) % 12 - 6, cells // 144 - 2], axis=1).astype(np.float64)
    k = rng.integers(1, per_voxel + 1, size=n_voxels)
    centre = np.repeat((c + 1.0) * RES, k, axis=0)
    return (centre + rng.uniform(-0.3, 0.3, size=centre.shape) * RES).astype(np.float32)


def lattice_cloud():
    """a dense 14 x 14 x 3 lattice of single-point voxels (the points sit at the voxel centres)"""
    g = np.stack(np.meshgrid(np.arange(-7, 7), np.arange(-7, 7), np.arange(-1, 2), indexing="ij"), axis=-1).reshape(-1, 3)
    return ((g + 1.0) * RES).astype(np.float32)


def numpy_map(P, Cov, mode, T=None, res=RES, inserts=1):
    """the snapshot of a map that received the float32 cloud P (Cov: its float32 covariances, unused for NDT) at pose T in one insert, by the
    numpy restatements of the insert contract (tests/incmap_ref.py, tests/ndtmap_ref.py)"""
    from tests import incmap_ref as I
    from tests import ndtmap_ref as N
    T = np.eye(4) if T is None else T
    Cov = cloud_covariances(P) if Cov is None else Cov
    if mode == 3:
        Pp = N.transform_points(P, T)
        terms = N.point_terms(Pp)
    else:
        Pp, Cp = I.transform_cloud(P, Cov, T)
        p64, c64 = Pp.astype(np.float64), Cp.astype(np.float64)
        six = np.stack([c64[:, 0, 0], c64[:, 0, 1], c64[:, 0, 2], c64[:, 1, 1], c64[:, 1, 2], c64[:, 2, 2]], axis=1)
        if mode == 2:
            Ci = np.linalg.inv(c64)
            six = np.stack([Ci[:, 0, 0], Ci[:, 0, 1], Ci[:, 0, 2], Ci[:, 1, 1], Ci[:, 1, 2], Ci[:, 2, 2]], axis=1)
            p64 = np.einsum("nij,nj->ni", Ci, p64)
        terms = np.concatenate([p64, six, np.ones((len(p64), 1))], axis=1)
    c, ok = I.voxel_coords(Pp, res)
    keys, first, inv = np.unique(S.packed_key(c[ok]), return_index=True, return_inverse=True)
    sums = np.zeros((len(keys), 10))
    np.add.at(sums, inv.reshape(-1), terms[ok])
    return dict(resolution=float(res), mode=int(mode), num_inserts=inserts, num_points=len(P), num_voxels=len(keys), coords=c[ok][first].astype(np.int32), sums=sums,
                ages=np.zeros(len(keys), np.uint32))


def bundled():
    """the bundled pair (target, source) and seeded covariances for both"""
    from tests import util
    tgt, src = util.bundled_pair()
    return dict(tgt=tgt, src=src, Ct=covariances(len(tgt), 11), Cs=covariances(len(src), 12))


def relative():
    """the pose of data/relative.txt (source scan -> target scan), its rotation made orthonormal (the file holds a few digits only)"""
    from tests import util
    T = np.array(util.relative_pose(), np.float64)
    U, _, Vt = np.linalg.svd(T[:3, :3])
    return pose(U @ Vt, T[:3, 3])


SHIFT = pose(np.eye(3), [2.0 * RES, -1.0 * RES, 0.0])  # whole voxels: rows stay apart, a voxel receives at most one
OUTSIDE = pose(np.eye(3), [3000.0 * RES, -2500.0 * RES, 40.0 * RES])  # far outside any bitmap box, inside the key range


def before_shift():
    """the pose at which the bitmap test inserts the source scan into `other`: SHIFT then brings it to relative()"""
    return np.linalg.inv(SHIFT) @ relative()


def guarded_cases():
    """every (name, cloud, covariances, pose the cloud was inserted at, pose of the merge) a GPU test sends through a posed merge or a transform that
    is not the identity: the CPU test asserts that near_face at twice the guard flags none of their rows, the GPU tests re-assert it with the
    single guard on the device's own snapshot"""
    b = bundled()
    out = [("bundled source, general pose", b["src"], b["Cs"], None, GENERAL), ("bundled target, general pose", b["tgt"], b["Ct"], None, GENERAL),
           ("bundled source, exact pose", b["src"], b["Cs"], None, EXACT), ("bundled source, relative pose", b["src"], b["Cs"], None, relative()),
           ("bundled source before the shift, shift", b["src"], b["Cs"], before_shift(), SHIFT), ("5 voxels, far outside", voxel_cloud(5, 77), None, None, OUTSIDE),
           ("lattice, 45 degrees", lattice_cloud(), None, None, DIAGONAL)]
    for n in EDGE_SIZES:
        out.append(("%d voxels, general pose" % n, voxel_cloud(n, 100 + n), None, None, GENERAL))
    return out


AGE_SEEDS = (31, 32, 33)  # `other` of the age test: three inserts of 300 voxels each (their union is what the merge moves: see ages_map)

