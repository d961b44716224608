"""numpy twin of fvh_voxelgrid_segment_plane (include/fast_vgicp_hip.h, "plane segmentation by RANSAC").

mix32 and the sample indices are Python integers; a hypothesis's plane, the axis test and the count test are np.float64 with the
associations the header writes down (numpy does not contract). The tests contain no division and no square root, so
tests/test_gpu_plane.py holds the device to EQUALITY with this twin on every count, the winner, the kept indices and the kept points.
The refit here is the twin's OWN fp64 route (np.linalg.eigh); the device's refit is compared with it at 1e-9, and the device's final
labelling is reproduced exactly from the coefficients the device returned (label_with)."""
import math

import numpy as np

from tests import outlier_ref as R

KEEP_OUTLIERS, REFINE = 1, 2
SLAB = 256  # PLANE_SLAB of kernels_plane.hpp: points a workgroup of the sweep stages
M32 = 0xFFFFFFFF
GOLD = 0x9E3779B9


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def seed_word(seed):
    seed &= 0xFFFFFFFFFFFFFFFF
    return mix32((seed & M32) ^ mix32((seed >> 32) ^ GOLD))


def sample_indices(seed, H, n):
    """int64[H, 3]: the input indices of every hypothesis"""
    s0 = seed_word(seed)
    out = np.zeros((H, 3), np.int64)
    for h in range(H):
        for j in range(3):
            out[h, j] = (mix32(s0 + GOLD * (3 * h + j + 1)) * n) >> 32
    return out


def hypotheses(p, H, seed, axis=None, eps_angle=0.0):
    p = R._f32(p)
    n = len(p)
    idx = sample_indices(seed, H, n)
    if n == 0:
        z = np.zeros(H)
        return dict(idx=idx, a=z, b=z, c=z, nn=z, q=np.zeros((H, 3)), valid=np.zeros(H, bool), ratio=z)
    p64 = p.astype(np.float64)
    q, p1, p2 = p64[idx[:, 0]], p64[idx[:, 1]], p64[idx[:, 2]]
    e1, e2 = p1 - q, p2 - q
    a = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    b = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    c = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    nn = (a * a + b * b) + c * c
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & (nn != 0.0)
    ratio = np.zeros(H)
    if axis is not None:
        ax, ay, az = (float(v) for v in axis)
        aa = (ax * ax + ay * ay) + az * az
        ce = math.cos(eps_angle)
        c2 = ce * ce
        dot = (a * ax + b * ay) + c * az
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(valid, dot * dot / (nn * aa), 0.0)  # (for the margin test only: how far each hypothesis is from c2)
        valid = valid & (dot * dot >= (c2 * nn) * aa)
    return dict(idx=idx, a=a, b=b, c=c, nn=nn, q=q, valid=valid, ratio=ratio)


def signed(p64, hyp, h):
    """s_i of hypothesis h for every point"""
    u = p64 - hyp["q"][h]
    return (hyp["a"][h] * u[:, 0] + hyp["b"][h] * u[:, 1]) + hyp["c"][h] * u[:, 2]


def counts_of(p, hyp, t, chunk=64):
    """int32[H]: count_h, -1 for an invalid hypothesis"""
    p64 = R._f32(p).astype(np.float64)
    H = len(hyp["valid"])
    t2 = float(t) * float(t)
    out = np.full(H, -1, np.int32)
    for lo in range(0, H, chunk):
        hs = lo + np.flatnonzero(hyp["valid"][lo:lo + chunk])
        if len(hs) == 0:
            continue
        ux = p64[None, :, 0] - hyp["q"][hs, 0][:, None]
        uy = p64[None, :, 1] - hyp["q"][hs, 1][:, None]
        uz = p64[None, :, 2] - hyp["q"][hs, 2][:, None]
        s = (hyp["a"][hs][:, None] * ux + hyp["b"][hs][:, None] * uy) + hyp["c"][hs][:, None] * uz
        out[hs] = (s * s <= (t2 * hyp["nn"][hs])[:, None]).sum(axis=1)
    return out


def fix_sign(co):
    co = np.array(co, np.float64)
    d = co[3]
    first = next((v for v in co[:3] if v != 0.0), 0.0)
    if d < 0.0 or (d == 0.0 and first < 0.0):
        co = -co
    return co


def label_with(p, co, t):
    """the final labelling of a refit call under the coefficients it returned"""
    p64 = R._f32(p).astype(np.float64)
    a, b, c, d = (np.float64(v) for v in co)
    s = ((a * p64[:, 0] + b * p64[:, 1]) + c * p64[:, 2]) + d
    t2 = np.float64(float(t) * float(t))
    return s * s <= t2 * ((a * a + b * b) + c * c)


def refit(p, inl, q):
    """the twin's own least-squares plane of the points p[inl], moments about q; also the eigenvalues (ascending)"""
    u = R._f32(p).astype(np.float64)[inl] - q
    m = len(u)
    mu = u.sum(axis=0) / m
    C = (u.T @ u) / m - np.outer(mu, mu)
    w, V = np.linalg.eigh(C)
    v = V[:, 0]
    centre = q + mu
    return fix_sign([v[0], v[1], v[2], -((v[0] * centre[0] + v[1] * centre[1]) + v[2] * centre[2])]), w


def segment(p, t, H=256, seed=0, axis=None, eps_angle=0.0, flags=0):
    """The contract. counts, winner, sample, valid (number), count_winner, coefficients, inlier (bool[n]), num_inliers, keep, idx, points,
    scores (float32[n]), threshold; with REFINE also eig (the covariance's eigenvalues) and refit (whether it ran)."""
    p = R._f32(p)
    n = len(p)
    p64 = p.astype(np.float64)
    hyp = hypotheses(p, H, seed, axis, eps_angle)
    counts = counts_of(p, hyp, t)
    out = dict(counts=counts, valid=int(hyp["valid"].sum()), hyp=hyp, threshold=float(t), refit=False, eig=None)
    if out["valid"] == 0:
        inl = np.zeros(n, bool)
        out.update(winner=-1, sample=np.zeros(3, np.int32), count_winner=0, coefficients=np.zeros(4), scores=np.full(n, np.inf, np.float32))
    else:
        w = int(np.argmax(counts))  # the first of the largest: ties to the smallest h
        s = signed(p64, hyp, w)
        nn = hyp["nn"][w]
        inl = s * s <= (float(t) * float(t)) * nn
        assert int(inl.sum()) == counts[w]
        norm = np.sqrt(nn)
        an, bn, cn = hyp["a"][w] / norm, hyp["b"][w] / norm, hyp["c"][w] / norm
        q = hyp["q"][w]
        co = fix_sign([an, bn, cn, -((an * q[0] + bn * q[1]) + cn * q[2])])
        out.update(winner=w, sample=hyp["idx"][w].astype(np.int32), count_winner=int(counts[w]), scores=(np.abs(s) / norm).astype(np.float32))
        if (flags & REFINE) and counts[w] >= 3:
            co, eig = refit(p, inl, q)
            inl = label_with(p, co, t)
            out.update(refit=True, eig=eig)
        out.update(coefficients=co)
    keep = ~inl if (flags & KEEP_OUTLIERS) else inl
    out.update(inlier=inl, num_inliers=int(inl.sum()), keep=keep, idx=np.flatnonzero(keep).astype(np.int32), points=p[keep])
    return out


# ---- the clouds of the GPU tests (built here so that the CPU tests prove the preconditions on the very same arrays) ----
def cloud_slabs():
    """lattice points, multiples of 1/4: a ground slab at z = 0 (1,600 points), a shelf at z = 2 (400), a wall at x = 5 (600), and 400
    points of clutter at z >= 1/2; rows shuffled. Every expression of the contract is exact in fp64 on it."""
    rng = np.random.default_rng(31)
    g = np.stack(np.meshgrid(np.arange(-20, 20), np.arange(-20, 20), indexing="ij"), axis=-1).reshape(-1, 2) * 0.25
    ground = np.column_stack([g, np.zeros(len(g))])
    s = np.stack(np.meshgrid(np.arange(0, 20), np.arange(0, 20), indexing="ij"), axis=-1).reshape(-1, 2) * 0.25
    shelf = np.column_stack([s, np.full(len(s), 2.0)])
    w = np.stack(np.meshgrid(np.arange(-15, 15), np.arange(2, 22), indexing="ij"), axis=-1).reshape(-1, 2) * 0.25
    wall = np.column_stack([np.full(len(w), 5.0), w])
    clutter = np.column_stack([rng.integers(-20, 20, 400), rng.integers(-20, 20, 400), rng.integers(2, 24, 400)]) * 0.25
    p = np.concatenate([ground, shelf, wall, clutter]).astype(np.float32)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def cloud_wall():
    """a wall (x = 3, 1,200 points) with more points than the ground (z = -1.5, 700 points), jittered by +-1 cm, and 300 points of clutter:
    the unconstrained winner is the wall, the axis (0, 0, 1) constraint makes it the ground"""
    rng = np.random.default_rng(32)
    wall = np.column_stack([3.0 + rng.uniform(-0.01, 0.01, 1200), rng.uniform(-6, 6, 1200), rng.uniform(-1.5, 3, 1200)])
    ground = np.column_stack([rng.uniform(-6, 3, 700), rng.uniform(-6, 6, 700), -1.5 + rng.uniform(-0.01, 0.01, 700)])
    clutter = rng.uniform(-6, 6, (300, 3))
    p = np.concatenate([wall, ground, clutter]).astype(np.float32)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def cloud_two_planes():
    """two parallel lattice planes of 20 x 20 points, z = 0 and z = 3, and nothing else: every hypothesis inside one plane counts 400"""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), axis=-1).reshape(-1, 2) * 0.25
    p = np.concatenate([np.column_stack([g, np.zeros(400)]), np.column_stack([g, np.full(400, 3.0)])]).astype(np.float32)
    return np.ascontiguousarray(p[np.random.default_rng(33).permutation(800)])


def cloud_collinear(n=300):
    """lattice points on one line: every cross product is exactly zero"""
    k = np.random.default_rng(34).permutation(n).astype(np.float64)
    return np.ascontiguousarray(np.column_stack([0.25 * k, 0.5 * k, -0.75 * k + 1.0]).astype(np.float32))


def cloud_all_duplicates(n=200):
    return np.ascontiguousarray(np.tile(np.array([[1.25, -2.5, 0.75]], np.float32), (n, 1)))


def named_cloud(name, cloud_a=None):
    if name == "A":
        assert cloud_a is not None
        return cloud_a
    if name.startswith("wall") and name != "wall":  # "wall<n>": the first n rows of the wall cloud (the size edges)
        return np.ascontiguousarray(cloud_wall()[:int(name[4:])])
    return {"slabs": cloud_slabs, "wall": cloud_wall, "two": cloud_two_planes, "collinear": cloud_collinear, "dup": cloud_all_duplicates, "U": R.cloud_u}[name]()


Z = (0.0, 0.0, 1.0)
DEG10 = math.radians(10.0)

# (cloud, distance_threshold, H, seed, axis: None or "Z" = (0, 0, 1) within 10 degrees, flags -> valid hypotheses, winner, count_winner, num_inliers)
TABLE = [ ("A", 0.1, 64, 7, None, 0, 64, 23, 1768, 1768), ("A", 0.1, 64, 7, "Z", 0, 4, 14, 893, 893), ("A", 0.1, 256, 7, None, 0, 256, 23, 1768, 1768), ("A", 0.1, 256, 7, "Z", 0, 18, 14, 893, 893), ("A", 0.1, 256, 7, None, 2, 256, 23, 1768, 1756), ("A", 0.1, 256, 7, "Z", 3, 18, 14, 893, 886), ("A", 0.05, 1000, 11, None, 1, 1000, 747, 1510, 1510), ("slabs", 0.3, 64, 3, None, 0, 64, 0, 1600, 1600), ("slabs", 0.3, 100, 3, "Z", 2, 18, 0, 1600, 1600), ("wall", 0.05, 64, 3, None, 0, 64, 5, 1207, 1207), ("wall", 0.05, 64, 3, "Z", 0, 2, 61, 527, 527), ("wall", 0.05, 64, 3, None, 2, 64, 5, 1207, 1205), ("wall", 0.05, 64, 3, "Z", 3, 2, 61, 527, 726), ("two", 0.1, 65, 5, None, 0, 64, 4, 400, 400), ("two", 0.1, 63, 5, None, 2, 62, 4, 400, 400), ("U", 0.5, 1, 1, None, 0, 1, 0, 125, 125), ("U", 0.5, 63, 1, None, 1, 63, 31, 167, 167), ("U", 0.5, 1000, 1, "Z", 2, 22, 712, 126, 122), ("wall65", 0.05, 16384, 9, None, 0, 15638, 1, 42, 42), ("wall65", 0.05, 16384, 9, "Z", 2, 889, 6152, 20, 19), ("collinear", 0.1, 64, 3, None, 2, 0, -1, 0, 0), ("dup", 0.1, 64, 3, None, 0, 0, -1, 0, 0)]
# the size edges: the first n rows of the wall cloud (PLANE_SLAB - 1, PLANE_SLAB, PLANE_SLAB + 1 among them)
EDGE_N = [0, 1, 2, 3, 4, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1]
