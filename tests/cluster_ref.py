"""numpy twin of fvh_voxelgrid_cluster_euclidean (include/fast_vgicp_hip.h): the connected components of the graph
"i ~ j iff i != j and d2(i, j) <= r2", with a size window, numbered by their smallest input index.

d2 is the fp32 (dx*dx + dy*dy) + dz*dz of tests/outlier_ref.py (_sq_rows, chunked brute force), r2 = (float)tolerance * (float)tolerance
clamped to 1e37, as for the radius filter. The components come from a plain union-find (the larger root hooks under the smaller, so a
root is its component's smallest index). Everything the call returns is an integer or a bit copy, so tests/test_gpu_cluster.py holds the
device to EQUALITY with this twin; the twin itself is held against scipy's connected_components on an fp64 adjacency in
tests/test_cluster_cpu.py."""
import numpy as np

from tests import outlier_ref as R


def r2_of(tolerance):
    r = np.float32(tolerance)
    with np.errstate(over="ignore"):
        return min(r * r, R.R2_MAX)


def _find(parent, x):
    """roots of the nodes x (an int array), by pointer chasing"""
    r = parent[x]
    while True:
        nxt = parent[r]
        if np.array_equal(nxt, r):
            return r
        r = nxt


def components(p, tolerance, chunk=256):
    """root[i] = the smallest index of i's component"""
    p = R._f32(p)
    n = len(p)
    r2 = r2_of(tolerance)
    parent = np.arange(n, dtype=np.int64)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        within = R._sq_rows(p, lo, hi) <= r2
        for i in range(lo, hi):
            js = np.flatnonzero(within[i - lo, :i])  # the neighbours at a lower index (j != i by INDEX: an exact duplicate is a neighbour)
            if len(js) == 0:
                continue
            roots = np.unique(np.append(_find(parent, js), _find(parent, np.array([i]))))
            parent[roots] = roots[0]  # every larger root hooks under the smallest
            parent[js] = roots[0]     # (path compression)
    return _find(parent, np.arange(n))


def cluster(p, tolerance, min_size=1, max_size=0):
    """The contract: labels (int32[n], -1 = in no kept component), sizes (int32[num_clusters]), the kept points in input order with their
    indices, scores = (float) size of each input point's component, threshold = min_size."""
    p = R._f32(p)
    n = len(p)
    root = components(p, tolerance)
    comp_size = np.bincount(root, minlength=n)  # indexed by root
    size = comp_size[root] if n else np.zeros(0, np.int64)
    keep = size >= min_size
    if max_size > 0:
        keep &= size <= max_size
    leaders = np.flatnonzero(keep & (root == np.arange(n)))  # ascending: the cluster numbers in order of the smallest input index
    number = np.full(n, -1, np.int64)
    number[leaders] = np.arange(len(leaders))
    labels = np.where(keep, number[root], -1).astype(np.int32) if n else np.zeros(0, np.int32)
    return dict(labels=labels, sizes=comp_size[leaders].astype(np.int32), num_clusters=len(leaders), keep=keep, idx=np.flatnonzero(keep).astype(np.int32),
                points=p[keep], scores=size.astype(np.float32), threshold=float(min_size), largest=int(comp_size.max()) if n else 0, root=root)


def partition(labels):
    """the clustering as a set of frozensets of indices (what a relabelling or a shuffle leaves unchanged); -1 is left out"""
    labels = np.asarray(labels)
    return {frozenset(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels) if c >= 0}


def cloud_helix():
    """(20 cos(s/20), 20 sin(s/20), 0.002 s), s = 0.1 k, k < 3000, rows permuted: neighbours along the curve are 0.1 apart (one component of
    3,000 at tolerance 0.15, 3,000 singletons at 0.09), the turns 0.25 apart: the longest dependent chain of unions the tests hold"""
    s = 0.1 * np.arange(3000, dtype=np.float64)
    p = np.stack([20 * np.cos(s / 20), 20 * np.sin(s / 20), 0.002 * s], axis=1).astype(np.float32)
    return np.ascontiguousarray(p[np.random.default_rng(5).permutation(3000)])


LATTICE_BELOW = float(np.nextafter(np.float32(0.5), np.float32(0)))  # 0.49999997

# (cloud, tolerance, min, max, clusters, kept points, largest component)
TABLE = [("A", 0.3, 1, 0, 34, 4099, 3388), ("A", 0.5, 1, 0, 6, 4099, 3405), ("A", 0.5, 10, 0, 5, 4098, 3405), ("A", 0.5, 10, 500, 4, 693, 3405),
         ("A", 1.0, 5, 0, 1, 4099, 4099), ("U", 0.8, 2, 0, 340, 817, 8), ("U", 1.2, 2, 0, 333, 1625, 75), ("U", 1.6, 2, 0, 43, 1936, 1751),
         ("lattice", 0.5, 1, 0, 1, 729, 729), ("lattice", LATTICE_BELOW, 1, 0, 729, 729, 1), ("dup", 1e-6, 2, 0, 50, 100, 2),
         ("ragged257", 4.0, 1, 0, 150, 257, 8), ("ragged257", 8.0, 2, 0, 3, 256, 251), ("ragged1025", 4.0, 1, 0, 51, 1025, 901), ("ragged1025", 8.0, 2, 0, 1, 1025, 1025),
         ("helix", 0.15, 1, 0, 1, 3000, 3000), ("helix", 0.09, 1, 0, 3000, 3000, 1)]
# the tile edges: (n, clusters at tolerance 4.0 min 1, clusters at tolerance 8.0 min 2)
EDGE_SIZES = [(1, None, None), (2, None, None), (9, None, None), (63, 56, 11), (64, 60, 10), (65, 60, 13)]


def named_cloud(name, cloud_a=None):
    if name == "A":
        assert cloud_a is not None
        return cloud_a
    if name == "U":
        return R.cloud_u()
    if name == "lattice":
        return R.cloud_lattice()
    if name == "dup":
        return R.cloud_duplicates()
    if name == "helix":
        return cloud_helix()
    assert name.startswith("ragged")
    return R.cloud_ragged(int(name[6:]))
