"""fp64 numpy twin of fvh_voxelgrid_deskew (include/fast_vgicp_hip.h has the contract), and the generators its tests share.

    xi_j = log(T[j]^-1 T[j+1]),  j(x) = largest j with tau[j] <= x clamped to [0, K-2],  s = (x - tau[j]) / (tau[j+1] - tau[j]),
    T(x) = T[j] exp(s xi_j),     p' = float32( T(t_ref)^-1 T((double)t) (double)p )

Knot poses are (K, 4, 4) in the usual row-major numpy indexing. Rotation-first exponential: exp(w, v) = {exp(w), V(w) v}."""
import numpy as np

SWEEP = 0.1  # seconds


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _abc(th):
    """a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3; the series below 1e-10 rad"""
    th = np.asarray(th, np.float64)
    small = th < 1e-10
    t = np.where(small, 1.0, th)
    sh, ch = np.sin(0.5 * t), np.cos(0.5 * t)
    sn = 2.0 * sh * ch
    a = np.where(small, 1.0, sn / t)
    b = np.where(small, 0.5, 2.0 * sh * sh / (t * t))
    c = np.where(small, 1.0 / 6.0, (t - sn) / (t * t * t))
    return a, b, c


def se3_exp(w, v):
    """4x4 of the twist (w, v)"""
    w, v = np.asarray(w, np.float64), np.asarray(v, np.float64)
    a, b, c = _abc(np.sqrt(w @ w))
    K = hat(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    T[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    return T


def se3_log(M):
    """(w, v) with se3_exp(w, v) == M; the rotation through the unit quaternion, so that angles up to pi are well conditioned"""
    R, t = np.asarray(M, np.float64)[:3, :3], np.asarray(M, np.float64)[:3, 3]
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2.0
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2.0
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2.0
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2.0
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    if q[0] < 0:
        q = -q
    nv = np.sqrt(q[1:] @ q[1:])
    th = 2.0 * np.arctan2(nv, q[0])
    w = (2.0 / q[0] if nv < 1e-12 else th / nv) * q[1:]
    d = 1.0 / 12.0 if th < 1e-5 else (1.0 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / (th * th)
    K = hat(w)
    v = t - 0.5 * (K @ t) + d * (K @ (K @ t))
    return w, v


def rigid_inv(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def twists(knot_poses):
    """(K-1, 3) rotation parts and (K-1, 3) translation parts of xi_j"""
    T = np.asarray(knot_poses, np.float64)
    wv = [se3_log(rigid_inv(T[j]) @ T[j + 1]) for j in range(len(T) - 1)]
    return np.array([x[0] for x in wv]), np.array([x[1] for x in wv])


def segment(tau, x):
    """the largest j with tau[j] <= x, clamped to [0, K-2]"""
    tau = np.asarray(tau, np.float64)
    return np.clip(np.searchsorted(tau, x, side="right") - 1, 0, len(tau) - 2)


def pose_at(tau, knot_poses, x, wv=None):
    """T(x), 4x4"""
    tau, T = np.asarray(tau, np.float64), np.asarray(knot_poses, np.float64)
    w, v = twists(T) if wv is None else wv
    j = int(segment(tau, x))
    s = (x - tau[j]) / (tau[j + 1] - tau[j])
    return T[j] @ se3_exp(s * w[j], s * v[j])


def _moved(p64, x, tau, T, w, v, left):
    """left @ T(x_i) @ p_i per point, fp64; left: 4x4"""
    j = segment(tau, np.where(np.isfinite(x), x, tau[0]))
    s = (x - tau[j]) / (tau[j + 1] - tau[j])
    ww, uu = s[:, None] * w[j], s[:, None] * v[j]
    a, b, c = _abc(np.sqrt((ww * ww).sum(axis=1)))
    k1, l1 = np.cross(ww, p64), np.cross(ww, uu)
    k2, l2 = np.cross(ww, k1), np.cross(ww, l1)
    q = (p64 + a[:, None] * k1 + b[:, None] * k2) + (uu + b[:, None] * l1 + c[:, None] * l2)
    A = np.einsum("ab,nbc->nac", left, T[j])  # left @ T[j] per point
    return np.einsum("nab,nb->na", A[:, :3, :3], q) + A[:, :3, 3]


def deskew(p, t, knot_times, knot_poses, t_ref=None):
    """(fp64 result, its float32 cast); rows with a non-finite coordinate or time are NaN"""
    tau, T = np.asarray(knot_times, np.float64), np.asarray(knot_poses, np.float64)
    p32, t32 = np.asarray(p, np.float32).reshape(-1, 3), np.asarray(t, np.float32).reshape(-1)
    t_ref = float(tau[-1] if t_ref is None else t_ref)
    w, v = twists(T)
    bad = ~(np.isfinite(p32).all(axis=1) & np.isfinite(t32))
    p64, x = np.where(bad[:, None], 0.0, p32.astype(np.float64)), np.where(bad, tau[0], t32.astype(np.float64))
    out = _moved(p64, x, tau, T, w, v, rigid_inv(pose_at(tau, T, t_ref, (w, v))))
    out[bad] = np.nan
    return out, out.astype(np.float32)


def skew(p, t, knot_times, knot_poses, t_ref=None):
    """The inverse map: q_i = T(t_i)^-1 T(t_ref) p_i in fp64 -- what a sensor moving along the trajectory records of the rigid cloud p
    (given in the sensor frame of t_ref). deskew(float32(skew(p))) recovers p."""
    tau, T = np.asarray(knot_times, np.float64), np.asarray(knot_poses, np.float64)
    p64, x = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(t, np.float32).reshape(-1).astype(np.float64)
    t_ref = float(tau[-1] if t_ref is None else t_ref)
    w, v = twists(T)
    world = p64 @ pose_at(tau, T, t_ref, (w, v))[:3, :3].T + pose_at(tau, T, t_ref, (w, v))[:3, 3]
    # T(x)^-1 = exp(-s xi_j) T[j]^-1: the same evaluation with the twist negated, applied to T[j]^-1 world
    j = segment(tau, x)
    s = (x - tau[j]) / (tau[j + 1] - tau[j])
    Tj_inv = np.array([rigid_inv(Tk) for Tk in T])[j]
    local = np.einsum("nab,nb->na", Tj_inv[:, :3, :3], world) + Tj_inv[:, :3, 3]
    ww, uu = -s[:, None] * w[j], -s[:, None] * v[j]
    a, b, c = _abc(np.sqrt((ww * ww).sum(axis=1)))
    k1, l1 = np.cross(ww, local), np.cross(ww, uu)
    k2, l2 = np.cross(ww, k1), np.cross(ww, l1)
    return (local + a[:, None] * k1 + b[:, None] * k2) + (uu + b[:, None] * l1 + c[:, None] * l2)


def deskew_quat(p, t, knot_times, knot_poses, t_ref=None):
    """The same map in another fp64 formulation (half-angle quaternion rotation, V as a matrix): what two correct fp64 evaluations differ by"""
    tau, T = np.asarray(knot_times, np.float64), np.asarray(knot_poses, np.float64)
    p64, x = np.asarray(p, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(t, np.float32).reshape(-1).astype(np.float64)
    t_ref = float(tau[-1] if t_ref is None else t_ref)
    w, v = twists(T)
    left = np.linalg.inv(pose_at(tau, T, t_ref, (w, v)))
    j = segment(tau, x)
    s = (x - tau[j]) / (tau[j + 1] - tau[j])
    ww, uu = s[:, None] * w[j], s[:, None] * v[j]
    th = np.sqrt((ww * ww).sum(axis=1))
    small = th < 1e-10
    ts = np.where(small, 1.0, th)
    qv = ww * np.where(small, 0.5, np.sin(0.5 * ts) / ts)[:, None]
    qw = np.where(small, 1.0, np.cos(0.5 * ts))
    tt = 2.0 * np.cross(qv, p64)
    rp = p64 + qw[:, None] * tt + np.cross(qv, tt)
    b = np.where(small, 0.5, (1.0 - np.cos(ts)) / (ts * ts))
    c = np.where(small, 1.0 / 6.0, (ts - np.sin(ts)) / (ts * ts * ts))
    K = np.zeros((len(p64), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ww[:, 2], ww[:, 1], ww[:, 2], -ww[:, 0], -ww[:, 1], ww[:, 0]
    V = np.eye(3)[None] + b[:, None, None] * K + c[:, None, None] * (K @ K)
    q = rp + np.einsum("nab,nb->na", V, uu)
    world = np.einsum("nab,nb->na", T[j][:, :3, :3], q) + T[j][:, :3, 3]
    return world @ left[:3, :3].T + left[:3, 3]


def scale(p, knot_poses):
    """M of the tolerance: 1 + max |p| + 2 max |knot translation|"""
    p = np.asarray(p, np.float64)
    return 1.0 + float(np.abs(p[np.isfinite(p)]).max(initial=0.0)) + 2.0 * float(np.abs(np.asarray(knot_poses, np.float64)[:, :3, 3]).max())


def tolerance(ref64, p, knot_poses):
    """per coordinate: half an ulp of the float32 result plus 1e-12 M of fp64 evaluation-order noise"""
    return 0.5 * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64) + 1e-12 * scale(p, knot_poses)


# ---- generators ----
def azimuth_times(p):
    """a spinning sensor: t = (atan2(y, x) + pi) / 2 pi * 0.1 s, float32"""
    p = np.asarray(p, np.float64)
    return ((np.arctan2(p[:, 1], p[:, 0]) + np.pi) / (2.0 * np.pi) * SWEEP).astype(np.float32)


def random_trajectory(K, seed=0, trans=1.5, rot=0.06, sweep=SWEEP):
    """(knot times (K,), knot poses (K, 4, 4)): about `trans` metres and `rot` radians over the sweep, uneven knot spacing, a start pose
    away from the identity"""
    rng = np.random.default_rng(seed)
    gaps = rng.uniform(0.5, 1.5, K - 1)
    tau = np.concatenate([[0.0], np.cumsum(gaps) / gaps.sum() * sweep])
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    direction = rng.normal(size=3)
    direction /= np.linalg.norm(direction)
    T = [se3_exp(0.3 * rng.normal(size=3), rng.normal(size=3))]
    for j in range(K - 1):
        f = (tau[j + 1] - tau[j]) / sweep
        w = f * rot * (axis + 0.3 * rng.normal(size=3))
        v = f * trans * (direction + 0.3 * rng.normal(size=3))
        T.append(T[-1] @ se3_exp(w, v))
    return tau, np.array(T)


def identity_trajectory(K, sweep=SWEEP):
    return np.linspace(0.0, sweep, K), np.tile(np.eye(4), (K, 1, 1))


def cloud_lattice(m=9, step=0.5):
    """m^3 points on a lattice centred at the origin (coordinates exact in float32), the origin itself included"""
    g = (np.arange(m) - m // 2) * step
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
