"""numpy twin of the three filters of include/fast_vgicp_hip.h (crop_range, remove_statistical_outliers, remove_radius_outliers).

d2(i, j) is fp32 (dx*dx + dy*dy) + dz*dz (numpy does not contract), by chunked brute force; everything else is fp64, as the header
defines it. The twin is the reference of tests/test_gpu_outlier.py and is itself held against an independent fp64 brute force on
lattices (tests/test_outlier_cpu.py), where fp32 is exact."""
import numpy as np

R2_MAX = np.float32(1e37)


def _f32(p):
    return np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 3))


def sq_norm(p):
    p = _f32(p)
    with np.errstate(invalid="ignore", over="ignore"):
        return (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]


def crop(p, min_sq_norm=1e-3, max_sq_norm=np.inf):
    """keep iff x, y, z finite and min <= (double)s <= max; score s"""
    p = _f32(p)
    s = sq_norm(p)
    sd = s.astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(p).all(axis=1) & (min_sq_norm <= sd) & (sd <= max_sq_norm)
    return dict(keep=keep, idx=np.flatnonzero(keep).astype(np.int32), points=p[keep], scores=s, threshold=float(max_sq_norm))


def _sq_rows(p, lo, hi):
    """d2 of rows [lo, hi) against the whole cloud, fp32, fixed association"""
    q = p[lo:hi]
    dx = p[None, :, 0] - q[:, None, 0]
    dy = p[None, :, 1] - q[:, None, 1]
    dz = p[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def radius(p, radius, min_neighbors, chunk=256):
    """keep iff #{j != i : d2(i, j) <= r2} >= min_neighbors, r2 = (float)radius * (float)radius clamped to 1e37; score min(count, min_neighbors)"""
    p = _f32(p)
    n = len(p)
    r = np.float32(radius)
    with np.errstate(over="ignore"):
        r2 = min(r * r, R2_MAX)
    counts = np.zeros(n, np.int64)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        within = _sq_rows(p, lo, hi) <= r2
        counts[lo:hi] = within.sum(axis=1) - within[np.arange(hi - lo), np.arange(lo, hi)]  # j != i by INDEX: duplicates stay neighbours
    keep = counts >= min_neighbors
    return dict(keep=keep, idx=np.flatnonzero(keep).astype(np.int32), points=p[keep], counts=counts,
                scores=np.minimum(counts, min_neighbors).astype(np.float32), threshold=float(min_neighbors))


def nearest_sq(p, kmax, chunk=256):
    """the kmax smallest d2 of every row, ascending (fp32): what the (d2, index)-ordered k-NN returns the distances of -- ties at the
    cut have the same d2 whichever index wins, so the VALUES are unique"""
    p = _f32(p)
    n = len(p)
    kmax = min(kmax, n)
    out = np.empty((n, kmax), np.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d2 = _sq_rows(p, lo, hi)
        part = np.partition(d2, kmax - 1, axis=1)[:, :kmax] if kmax < n else d2
        out[lo:hi] = np.sort(part, axis=1)
    return out


def mean_distances(p, mean_k, nearest=None):
    """d_i = (float)(sum (double)sqrtf(d2) / mean_k) over the mean_k + 1 nearest points (the nearest, at distance 0, adds nothing)"""
    near = nearest_sq(p, mean_k + 1) if nearest is None else nearest[:, :mean_k + 1]
    assert near.shape[1] == mean_k + 1
    return (np.sqrt(near).astype(np.float64).sum(axis=1) / mean_k).astype(np.float32)


def statistical(p, mean_k, stddev_mul, nearest=None):
    p = _f32(p)
    n = len(p)
    assert 1 <= mean_k <= 63 and n > mean_k
    d = mean_distances(p, mean_k, nearest)
    d64 = d.astype(np.float64)
    s1, s2 = d64.sum(), (d64 * d64).sum()
    mu = s1 / n
    var = max(0.0, (s2 - s1 * s1 / n) / (n - 1))
    t = mu + stddev_mul * np.sqrt(var)
    keep = d64 <= t
    margin = float(np.min(np.abs(d64 - t)) / t)
    return dict(keep=keep, idx=np.flatnonzero(keep).astype(np.int32), points=p[keep], scores=d, threshold=float(t), mu=mu, var=var, margin=margin)


# ---- the clouds of the GPU tests (built here so that the CPU tests prove the preconditions on the very same arrays) ----
def cloud_u():
    return np.random.default_rng(7).uniform(-10, 10, (2000, 3)).astype(np.float32)  # the generator's first draw


def cloud_ragged(n, seed=11):
    return np.random.default_rng(seed + n).uniform(-20, 20, (n, 3)).astype(np.float32)


def cloud_lattice(half=4, spacing=0.5):
    """lattice indices -half..half per axis at `spacing` (729 points for +-4): every coordinate, difference and d2 is exact in fp32"""
    g = np.arange(-half, half + 1, dtype=np.float32) * np.float32(spacing)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def cloud_duplicates(n=600, dups=50, seed=3):
    """a random cloud in +-5 m in which `dups` points are exact copies of earlier ones"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    src = rng.choice(n // 2, dups, replace=False)
    dst = n // 2 + rng.choice(n - n // 2, dups, replace=False)
    p[dst] = p[src]
    return p


# Statistical filter on cloud A (first 4,099 rows of the bundled source) and U: the combinations whose smallest relative margin
# |d_i - t| / t is at least 1e-5 -- two orders above one fp32 ulp of a score, so the kept set cannot depend on the last bit of a score
# (cloud, mean_k, stddev_mul, kept)
SOR_TABLE = [("A", 8, 0.5, 3079), ("A", 8, 1.0, 3531), ("A", 8, 2.0, 3941), ("A", 20, 1.0, 3510), ("A", 20, 2.0, 3872), ("A", 50, 1.0, 3491), ("A", 50, 2.0, 3860),
             ("U", 20, 0.5, 1498), ("U", 20, 1.0, 1711), ("U", 50, 0.5, 1506)]
SOR_MIN_MARGIN = 1e-5
RAGGED_MEAN_K = 8
RAGGED_SIZES = [RAGGED_MEAN_K + 1, 63, 64, 65, 257, 1025]


def ragged_stddev_mul(p, mean_k=RAGGED_MEAN_K, nearest=None):
    """the first stddev_mul of {0.5, 1.0, 2.0} that meets the margin precondition on this cloud (None: none does)"""
    for mul in (0.5, 1.0, 2.0):
        if statistical(p, mean_k, mul, nearest)["margin"] >= SOR_MIN_MARGIN:
            return mul
    return None
