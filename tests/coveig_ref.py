"""Plain references for the third numerical core -- the k-NN covariances (kernels_cov.hpp: cov_from_neighbors_kernel<5|8>,
cov_from_neighbors_regather_kernel) and the eigen solver / regulariser under every covariance (dev_math.hpp: sym_eig3, regularize_cov).
numpy and the standard library only: no engine code, no oracle call.

  exact_cov      the covariance of each neighbour list in exact rational arithmetic, rounded once to fp64
  reg_reference  the five regularisations as matrix functions (numpy.linalg.eigh), fp64
  jacobi_twin    the device's cyclic Jacobi restated with IEEE operations: same thresholds, rotation order, sweep cap, ascending sort
  MATRICES       the matrices the solver is held on through capi.debug_regularize (tests/test_gpu_cov_edges.py, part a)
  CLOUDS         the clouds + neighbour lists the three covariance kernels are held on (part b); every cloud is at most 2,000 points

The solver bound. Per matrix S with s = |S|max and eps = 2^-52 the solver is held to
    |V diag(w) V^T - S|max <= K eps s,   |V^T V - I|max <= K eps,   |w - eigvalsh(S)|max <= K eps s,   w ascending, all finite.
K = 4 x the worst of those three figures (in units of eps s / eps) that jacobi_twin -- the same algorithm in correctly rounded IEEE
arithmetic -- shows over the whole MATRICES list: tests/test_coveig_ref_cpu.py recomputes it and pins K_TWIN_MEASURED. The factor 4 is for
the device's Newton-refined seeds (reciprocal, square root, reciprocal square root: about 1 ulp, not correctly rounded) and fma contraction.
    measured worst of the twin over MATRICES: 11.68 (eigenvalues, scale_1e-100_1e100), at most 4 sweeps on every family -> K = 4 x 11.7 = 46.8
    measured worst of the DEVICE over the same list (MI355X), same units: reconstruction 7.10, orthogonality 6.00, eigenvalues 11.68

The solver's domain: finite symmetric matrices with 1e-100 <= |S|max <= 1e100, or S = 0. Below about 1e-134 the sweep loop leaves early
(off <= 1e-300 holds before anything is diagonal); that is outside the domain and not tested.
"""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS = range(5)
METHODS = (NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS)
METHOD_NAMES = ("NONE", "MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE", "FROBENIUS")

K_TWIN_MEASURED = 11.7  # worst residual of jacobi_twin over MATRICES, units of eps (test_coveig_ref_cpu.py: test_twin_meets_the_bound...)
K = 4.0 * K_TWIN_MEASURED
STORAGE_REL = 2e-7  # the project's figure for a covariance stored in fp32
PLANE_STORAGE_REL = 1.2e-7  # ... and the storage term of tests/util.py: cov_error_bound


# ---------------------------------------------------------------------------------------------
# exact covariances
# ---------------------------------------------------------------------------------------------
def _exact_ints(points_f32):
    """(integer coordinates X with p = X / D, D): every float is an exact rational; one common power-of-two denominator"""
    p = np.asarray(points_f32, dtype=np.float32)
    fr = [[Fraction(float(v)) for v in row] for row in p]
    D = 1
    for row in fr:
        for f in row:
            D = max(D, f.denominator)  # (all denominators are powers of two: the largest is the common one)
    return [[f.numerator * (D // f.denominator) for f in row] for row in fr], D


def exact_mean_cov(points_f32, idx):
    """Mean (m, 3) and covariance (m, 3, 3) of the points each row of `idx` lists (a repeated index counts as often as it is listed), in exact
    rational arithmetic -- cov = (k sum p p^T - sum p sum p^T) / k^2 over fractions.Fraction -- rounded ONCE to fp64."""
    X, D = _exact_ints(points_f32)
    idx = np.asarray(idx)
    m, k = idx.shape
    mean = np.empty((m, 3))
    cov = np.empty((m, 3, 3))
    den_m, den_c = k * D, k * k * D * D
    for r in range(m):
        rows = [X[j] for j in idx[r]]
        s = [sum(q[a] for q in rows) for a in range(3)]
        for a in range(3):
            mean[r, a] = float(Fraction(s[a], den_m))
            for b in range(a, 3):
                sab = sum(q[a] * q[b] for q in rows)
                cov[r, a, b] = cov[r, b, a] = float(Fraction(k * sab - s[a] * s[b], den_c))
    return mean, cov


def exact_cov(points_f32, idx):
    return exact_mean_cov(points_f32, idx)[1]


# ---------------------------------------------------------------------------------------------
# the regularisations as matrix functions
# ---------------------------------------------------------------------------------------------
def reg_reference(C, method):
    """regularize_cov(method) of (m, 3, 3) symmetric fp64 matrices. NONE: the identity. FROBENIUS: the formula in fp64 -- A = C + 1e-3 I,
    A^-1 normalised to Frobenius norm 1, inverted: that is A |A^-1|_F, and |A^-1|_F^2 = sum 1 / mu_i^2 over the eigenvalues of A (evaluated
    so because two literal inversions lose cond(A) eps each and say nothing from cond(A) = 1e8 on). MIN_EIG / NORMALIZED_MIN_EIG: the matrix functions V max(w, 1e-3) V^T and
    V max(w / w_max, 1e-3) V^T through numpy.linalg.eigh (well defined at eigenvalue ties; on the zero matrix 0 / 0 counts as below the
    floor: 1e-3 I). PLANE: I - 0.999 n n^T with n the eigenvector of the smallest eigenvalue."""
    C = np.asarray(C, np.float64)
    if method == NONE:
        return C.copy()
    if method == FROBENIUS:
        A = C + 1e-3 * np.eye(3)
        with np.errstate(divide="ignore"):
            return A * np.sqrt((1.0 / np.linalg.eigvalsh(A) ** 2).sum(axis=1))[:, None, None]
    w, V = np.linalg.eigh(C)
    if method == PLANE:
        n = V[:, :, 0]
        return np.eye(3)[None] - 0.999 * n[:, :, None] * n[:, None, :]
    if method == MIN_EIG:
        d = np.maximum(w, 1e-3)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.fmax(w / w[:, 2:3], 1e-3)  # (fmax: a NaN ratio -- the zero matrix -- gives the floor)
    return np.einsum("mij,mj,mkj->mik", V, d, V)


def frobenius_condition(C):
    """How much FROBENIUS amplifies a relative perturbation of C, per matrix: R = A |A^-1|_F with A = C + 1e-3 I, so a change dC moves R by
    |dC| |A^-1|_F + |A| d|A^-1|_F <= |dC| |A^-1|_F (1 + |A| / mu_min(A)); relative to |R| ~ |A| |A^-1|_F that is (|dC| / |C|) (1 + |C|max / mu_min(A))
    at most. 1 for tiny or well-conditioned matrices, |C|max / 1e-3 for a rank-deficient one."""
    C = np.asarray(C, np.float64)
    mu = np.linalg.eigvalsh(C)[:, 0] + 1e-3
    return 1.0 + np.abs(C).max(axis=(1, 2)) / np.maximum(mu, 1e-300)


# ---------------------------------------------------------------------------------------------
# the device's Jacobi in IEEE arithmetic
# ---------------------------------------------------------------------------------------------
SWEEP_CAP = 12


def jacobi_twin(S, sweep_cap=SWEEP_CAP, stats=None):
    """sym_eig3 of dev_math.hpp on (m, 3, 3) matrices with every reciprocal, square root and reciprocal square root an IEEE operation:
    cyclic rotations (0,1), (0,2), (1,2); a rotation skipped for |apq| <= 1e-290; t = 0.5 / theta for |theta| > 1e100; at most 12 sweeps, ended
    by off <= 1e-300 or off <= 1e-32 diag; ascending 3-element sorting network. -> (w (m, 3), V (m, 3, 3) eigenvectors in the columns,
    sweeps (m,) = sweeps that rotated); `stats`, a dict, receives how many rotations took the huge-theta branch and how many were skipped on a
    non-zero element"""
    S = np.asarray(S, np.float64)
    m = len(S)
    a = {(0, 0): S[:, 0, 0].copy(), (0, 1): S[:, 0, 1].copy(), (0, 2): S[:, 0, 2].copy(), (1, 1): S[:, 1, 1].copy(), (1, 2): S[:, 1, 2].copy(), (2, 2): S[:, 2, 2].copy()}
    v = np.tile(np.eye(3), (m, 1, 1))
    sweeps = np.zeros(m, int)
    active = np.ones(m, bool)

    def key(i, j):
        return (i, j) if i <= j else (j, i)

    with np.errstate(all="ignore"):
        for _ in range(sweep_cap):
            off = a[0, 1] * a[0, 1] + a[0, 2] * a[0, 2] + a[1, 2] * a[1, 2]
            diag = a[0, 0] * a[0, 0] + a[1, 1] * a[1, 1] + a[2, 2] * a[2, 2]
            active &= ~((off <= 1e-300) | (off <= 1e-32 * diag))
            if not active.any():
                break
            sweeps += active
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = a[p, q]
                rot = active & (np.abs(apq) > 1e-290)
                safe = np.where(rot, apq, 1.0)
                theta = (a[q, q] - a[p, p]) / (2.0 * safe)
                big = ~(np.abs(theta) <= 1e100)
                rr = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(big, 0.5 / theta, np.where(theta >= 0, rr, -rr))
                if stats is not None:
                    stats["huge_theta"] = stats.get("huge_theta", 0) + int((rot & big).sum())
                    stats["skipped"] = stats.get("skipped", 0) + int((active & ~rot & (apq != 0)).sum())
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = a[p, p] - t * apq, a[q, q] + t * apq
                rp, rq = a[key(r, p)], a[key(r, q)]
                arp, arq = c * rp - s * rq, s * rp + c * rq
                a[p, p] = np.where(rot, app, a[p, p])
                a[q, q] = np.where(rot, aqq, a[q, q])
                a[p, q] = np.where(rot, 0.0, apq)
                a[key(r, p)] = np.where(rot, arp, rp)
                a[key(r, q)] = np.where(rot, arq, rq)
                vp, vq = v[:, :, p].copy(), v[:, :, q].copy()
                v[:, :, p] = np.where(rot[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                v[:, :, q] = np.where(rot[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    e = np.stack([a[0, 0], a[1, 1], a[2, 2]], axis=1)
    order = np.tile(np.arange(3), (m, 1))
    for i, j in ((0, 1), (1, 2), (0, 1)):  # the device's network: swap on a strict >
        sw = e[:, i] > e[:, j]
        e[sw, i], e[sw, j] = e[sw, j], e[sw, i]
        order[sw, i], order[sw, j] = order[sw, j], order[sw, i]
    V = np.take_along_axis(v, order[:, None, :], axis=2)
    return e, V, sweeps


def eig_residuals(S, w, V):
    """The three figures of the solver bound per matrix, in units of eps s (reconstruction, eigenvalues) and eps (orthogonality); on the zero
    matrix anything but an exact answer is inf. -> dict of (m,) arrays + `ascending` and `finite` (bool)"""
    S, w, V = (np.asarray(x, np.float64) for x in (S, w, V))
    s = np.abs(S).max(axis=(1, 2))
    with np.errstate(all="ignore"):
        rec = np.abs(np.einsum("mij,mj,mkj->mik", V, w, V) - S).max(axis=(1, 2))
        orth = np.abs(np.einsum("mji,mjk->mik", V, V) - np.eye(3)).max(axis=(1, 2)) / EPS
        ev = np.abs(w - np.linalg.eigvalsh(S)).max(axis=1)

        def units(x):
            return np.where(s > 0, x / (EPS * np.where(s > 0, s, 1.0)), np.where(x == 0, 0.0, np.inf))
        out = dict(reconstruction=units(rec), orthogonality=orth, eigenvalues=units(ev))
    out["ascending"] = (w[:, 0] <= w[:, 1]) & (w[:, 1] <= w[:, 2])
    out["finite"] = np.isfinite(w).all(axis=1) & np.isfinite(V).all(axis=(1, 2))
    for k_ in ("reconstruction", "orthogonality", "eigenvalues"):
        out[k_] = np.where(np.isfinite(out[k_]), out[k_], np.inf)
    return out


def plane_tie_violations(R, S, tol, lam_tol=1e-9):
    """PLANE where the two smallest eigenvalues of S tie (the smallest eigenvector is not defined): the result must still be symmetric and finite
    with the spectrum {1e-3, 1, 1} to `tol`, and its own smallest eigenvector n must lie in the tied eigenspace: n^T S n <= lambda_1(S) + 1e-9 lambda_max.
    -> (m,) bool, True where one of these fails"""
    R, S = np.asarray(R, np.float64), np.asarray(S, np.float64)
    bad = ~np.isfinite(R).all(axis=(1, 2))
    Rf = np.where(bad[:, None, None], np.eye(3), R)
    bad |= np.abs(Rf - Rf.transpose(0, 2, 1)).max(axis=(1, 2)) > 0
    wr, Vr = np.linalg.eigh(0.5 * (Rf + Rf.transpose(0, 2, 1)))
    bad |= np.abs(wr - np.array([1e-3, 1.0, 1.0])).max(axis=1) > tol
    ws = np.linalg.eigvalsh(S)
    n = Vr[:, :, 0]
    q = np.einsum("mi,mij,mj->m", n, S, n)
    bad |= q > ws[:, 1] + lam_tol * np.abs(ws).max(axis=1)
    return bad


# ---------------------------------------------------------------------------------------------
# MATRICES: what the solver is held on
# ---------------------------------------------------------------------------------------------
PER_FAMILY = 2048


def _rand_q(rng, m):
    q, r = np.linalg.qr(rng.normal(size=(m, 3, 3)))
    return q * np.sign(np.einsum("mii->mi", r))[:, None, :]


def _qdq(q, d):
    A = np.einsum("mij,mj,mkj->mik", q, d, q)
    return 0.5 * (A + A.transpose(0, 2, 1))


def _spd(rng, m):
    g = rng.normal(size=(m, 3, 3))
    return np.einsum("mij,mkj->mik", g, g)


def _logu(rng, lo, hi, m):
    return 10.0 ** rng.uniform(lo, hi, size=m)


def _build_matrices():
    rng = np.random.default_rng(20260)
    m = PER_FAMILY
    fam = {}
    fam["spd"] = _spd(rng, m)
    a = rng.uniform(0, 16, m)
    b = rng.uniform(a, 16)
    b[: m // 8] = 16.0  # the full 1 ... 1e-16
    fam["graded"] = _qdq(_rand_q(rng, m), np.stack([np.ones(m), 10.0 ** -a, 10.0 ** -b], axis=1))
    u, v = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    fam["rank1"] = u[:, :, None] * u[:, None, :]
    fam["rank2"] = fam["rank1"] + v[:, :, None] * v[:, None, :]
    x = np.where(rng.random(m) < 0.5, rng.uniform(0, 1, m), rng.uniform(1, 3, m))
    fam["tie"] = _qdq(_rand_q(rng, m), np.stack([np.ones(m), np.ones(m), x], axis=1))
    fam["scaled_identity"] = _logu(rng, -12, 12, m)[:, None, None] * np.eye(3)
    fam["near_tie"] = _qdq(_rand_q(rng, m), np.stack([np.ones(m), np.full(m, 1.0 + 1e-13), np.where(rng.random(m) < 0.5, rng.uniform(0, 0.9, m), rng.uniform(1.1, 3, m))], axis=1))
    fixed = np.zeros((m, 3, 3))  # the zero matrix, the identity, diagonal matrices: no rotation at all
    fixed[1] = np.eye(3)
    d = rng.uniform(0, 2, size=(m, 3)) * _logu(rng, -6, 6, m)[:, None]
    d[2: m // 4, rng.integers(0, 3)] = 0.0
    fixed[2:, [0, 1, 2], [0, 1, 2]] = d[2:]
    fam["zero_identity_diagonal"] = fixed
    ap = np.zeros((m, 3, 3))  # one exactly zero off-diagonal pair: the axis-aligned plane / a block-diagonal matrix
    g2 = rng.normal(size=(m, 2, 2))
    ap[:, :2, :2] = np.einsum("mij,mkj->mik", g2, g2)
    ap[:, 2, 2] = np.where(rng.random(m) < 0.5, 0.0, rng.uniform(0, 2, m))
    perm = np.array([[0, 1, 2], [0, 2, 1], [2, 1, 0]])[rng.integers(0, 3, m)]
    fam["axis_plane"] = np.take_along_axis(np.take_along_axis(ap, perm[:, :, None], axis=1), perm[:, None, :], axis=2)

    def beside(tiny):  # a tiny off-diagonal beside one of 0.3
        A = np.zeros((m, 3, 3))
        A[:, [0, 1, 2], [0, 1, 2]] = rng.uniform(0.5, 3.0, size=(m, 3)) + np.array([0.0, 3.0, 6.0]) * (rng.random(m) < 0.5)[:, None]
        where = rng.integers(0, 3, m)  # which pair is the tiny one
        pairs = np.array([[0, 1], [0, 2], [1, 2]])
        other = pairs[(where + 1 + rng.integers(0, 2, m)) % 3]
        tp = pairs[where]
        sgn = np.where(rng.random(m) < 0.5, -1.0, 1.0)
        A[np.arange(m), tp[:, 0], tp[:, 1]] = A[np.arange(m), tp[:, 1], tp[:, 0]] = sgn * tiny
        A[np.arange(m), other[:, 0], other[:, 1]] = A[np.arange(m), other[:, 1], other[:, 0]] = 0.3
        return A
    fam["huge_theta"] = beside(_logu(rng, -280, -100, m))  # the only way into the |theta| > 1e100 branch
    fam["skipped_rotation"] = beside(_logu(rng, -305, -291, m))  # |apq| <= 1e-290: the rotation is skipped
    def scaled(lo, hi):  # |S|max = the scale: the ends of the range are the ends of the domain
        A = _spd(rng, m)
        sc = _logu(rng, lo, hi, m)
        sc[:2] = 10.0 ** lo, 10.0 ** hi
        return A / np.abs(A).max(axis=(1, 2))[:, None, None] * sc[:, None, None]
    fam["scale_1e-100_1e100"] = np.clip(scaled(-100, 100), -1e100, 1e100)
    fam["scale_1e-12_1e12"] = scaled(-12, 12)
    return fam


MATRICES = _build_matrices()  # family name -> (PER_FAMILY, 3, 3)


# ---------------------------------------------------------------------------------------------
# CLOUDS: what the covariance kernels are held on
# ---------------------------------------------------------------------------------------------
KS = (1, 2, 3, 4, 5, 7, 19, 20, 21, 31, 32, 33, 63, 64)
NS = (1, 3, 63, 64, 65, 257, 2000)
SCALES = (1e-3, 1.0, 1e3)
OFFSETS = (0.0, 50.0, 1e4)
SHAPES = ("blob", "line", "tilted_plane", "axis_plane", "lattice", "coincident", "repeat")


def _shape_points(shape, n, rng):
    if shape == "line":
        return rng.uniform(-2, 2, size=(n, 1)) * np.array([[0.48, -0.6, 0.64]])
    if shape == "tilted_plane":
        return rng.uniform(-2, 2, size=(n, 1)) * np.array([[0.6, 0.0, 0.8]]) + rng.uniform(-2, 2, size=(n, 1)) * np.array([[0.28, 0.96, -0.21]])
    if shape == "axis_plane":
        p = rng.uniform(-2, 2, size=(n, 3))
        p[:, 2] = 0.5
        return p
    if shape == "lattice":
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
        assert n <= len(g)
        return 0.25 * g[rng.permutation(len(g))[:n]].astype(np.float64) - 1.0
    return rng.normal(size=(n, 3))  # blob (and the clouds whose LISTS are the special thing)


def _window_lists(n, k, rng):
    """k neighbour indices per point from a window of the cloud around it, distinct while k <= the window; longer lists go round again"""
    win = min(n, 128)
    cols = []
    while sum(c.shape[1] for c in cols) < k:
        cols.append(np.argsort(rng.random((n, win)), axis=1))
    off = np.concatenate(cols, axis=1)[:, :k]
    return ((np.arange(n)[:, None] + off) % n).astype(np.int32)


def _knn_lists(pts, k):
    d = ((pts[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


def _make_cloud(name, shape, n, k, scale, offset, seed):
    rng = np.random.default_rng(seed)
    base = _shape_points(shape, n, rng)
    pts = (offset + scale * base).astype(np.float32)
    if shape == "lattice":
        idx = _knn_lists(pts, k) if k <= n else _window_lists(n, k, rng)
    elif shape == "coincident":
        idx = np.repeat(rng.integers(0, n, size=(n, 1)), k, axis=1).astype(np.int32)  # k times one point
    else:
        idx = _window_lists(n, k, rng)
        if shape == "repeat":
            idx[:, : (k + 1) // 2] = idx[:, :1]  # half the slots repeat one index
    # PLANE is defined by the smallest eigenvector: where the construction ties the two smallest eigenvalues (fewer than three distinct
    # points, collinear points, symmetric lattice neighbourhoods, a blob squeezed onto the fp32 grid of a far offset) only the tie
    # properties hold; everywhere else every point is held to the gap-aware bound
    quantised = offset != 0.0 and scale / offset < 1e-6
    distinct = min(n, k) if shape != "coincident" else 1
    if shape == "repeat":
        distinct = min(n, k - (k + 1) // 2 + 1)
    may_tie = shape in ("line", "coincident", "lattice") or distinct < 3 or quantised
    return dict(name=name, shape=shape, n=n, k=k, scale=scale, offset=offset, pts=pts, idx=idx, may_tie=may_tie, coincident=shape == "coincident" or n == 1)


def _build_clouds():
    out = []
    seed = 1000
    for n in NS:  # every k at every n, on a blob at lidar range
        for k in KS:
            seed += 1
            out.append(_make_cloud("blob_n%d_k%d" % (n, k), "blob", n, k, 1.0, 50.0, seed))
    ks = (5, 20, 33, 3, 64, 7, 21, 2, 32, 19, 63, 4, 31, 1)
    j = 0
    for shape in SHAPES:  # every shape at every scale and offset; k walks through the list
        for scale in SCALES:
            for offset in OFFSETS:
                seed += 1
                k = ks[j % len(ks)]
                j += 1
                out.append(_make_cloud("%s_s%g_o%g_k%d" % (shape, scale, offset, k), shape, 257, k, scale, offset, seed))
    return out


CLOUDS = _build_clouds()


# ---------------------------------------------------------------------------------------------
# the checks of part b, shared by the GPU test (the kernels' output) and the CPU test (a model of the kernels, with and without a defect)
# ---------------------------------------------------------------------------------------------
def cloud_reference(cloud):
    """(raw exact covariance, {method: reference}) of a CLOUDS entry, computed once"""
    if "_ref" not in cloud:
        raw = exact_cov(cloud["pts"], cloud["idx"])
        cloud["_ref"] = (raw, {m: reg_reference(raw, m) for m in METHODS})
    return cloud["_ref"]


def plane_error_bound(got, ref, raw, input_rel, storage_rel):
    """tests/util.py: cov_error_bound(gaps="01"), restated here so that this module stays free of the engine's helpers (the GPU test checks the two agree)"""
    got, ref, raw = (np.asarray(x, np.float64) for x in (got, ref, raw))
    w = np.linalg.eigvalsh(raw)
    lam = np.maximum(np.abs(w).max(axis=1), 1e-300)
    gap = w[:, 1] - w[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.where(gap > 1e-14 * lam, 8.0 * input_rel * lam / gap, np.inf)
    scale = np.abs(ref).max(axis=(1, 2))
    return np.abs(got - ref).max(axis=(1, 2)), (storage_rel + amp) * scale, amp >= 0.5


def cloud_violations(cloud, method, got):
    """Points of a CLOUDS entry at which `got` (n, 3, 3), the fp32-stored covariances of `method`, miss their check -> (bad (n,) bool, worst
    error in units of its bound). NONE / MIN_EIG / NORMALIZED_MIN_EIG: |got - ref|max <= 2e-7 |ref|max on every point (FROBENIUS: times its
    condition number at the 1e-13 input precision of the fp64 sums); coincident neighbours under NONE: exactly 0; PLANE: the gap-aware bound with
    input_rel = 1e-13, no point excused unless the cloud ties by construction, where the tie properties hold instead; everything finite."""
    raw, refs = cloud_reference(cloud)
    ref = refs[method]
    got = np.asarray(got, np.float64)
    finite = np.isfinite(got).all(axis=(1, 2))
    g = np.where(finite[:, None, None], got, 0.0)
    if method == PLANE:
        err, bound, degenerate = plane_error_bound(g, ref, raw, 1e-13, PLANE_STORAGE_REL)
        bad = ~finite | (~degenerate & (err > bound))
        if degenerate.any():
            if not cloud["may_tie"]:
                bad |= degenerate
            else:
                bad[degenerate] |= plane_tie_violations(g[degenerate], raw[degenerate], STORAGE_REL)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(degenerate, 0.0, err / bound)
        return bad, float(rel.max())
    scale = np.abs(ref).max(axis=(1, 2))
    err = np.abs(g - ref).max(axis=(1, 2))
    bound = STORAGE_REL * scale
    if method == FROBENIUS:
        bound = bound + 8.0 * 1e-13 * frobenius_condition(raw) * scale
    if method == NONE and cloud["coincident"]:
        bound = np.zeros_like(bound)
    bad = ~finite | (err > bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(err == 0, 0.0, err / bound)
    return bad, float(rel.max())


def kernel_model(pts, idx, method, drop_centring=False, mask_one_more=False, plane_swapped=False):
    """What the covariance kernels compute, in numpy: fp64 mean of the listed fp32 points, centred fp64 sums, 1 / k, the regularisation through
    jacobi_twin, one rounding to fp32. The switches are the defects tests/test_coveig_ref_cpu.py plants: the sums taken uncentred, the last
    slot of every list masked out (still divided by k), PLANE's floor on the largest eigenvalue instead of the smallest."""
    p = np.asarray(pts, np.float32).astype(np.float64)[np.asarray(idx)]  # (n, k, 3)
    k = p.shape[1]
    if mask_one_more:
        p = p[:, : k - 1]
    mean = p.sum(axis=1) / k
    d = p if drop_centring else p - mean[:, None, :]
    C = np.einsum("nka,nkb->nab", d, d) * (1.0 / k)
    if method == NONE:
        R = C
    elif method == FROBENIUS:
        R = reg_reference(C, FROBENIUS)
    else:
        w, V, _ = jacobi_twin(C)
        if method == PLANE:
            dd = np.tile(np.array([1.0, 1.0, 1e-3]) if plane_swapped else np.array([1e-3, 1.0, 1.0]), (len(C), 1))
        elif method == MIN_EIG:
            dd = np.maximum(w, 1e-3)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                dd = np.fmax(w / w[:, 2:3], 1e-3)
        R = np.einsum("mij,mj,mkj->mik", V, dd, V)
    return R.astype(np.float32)
