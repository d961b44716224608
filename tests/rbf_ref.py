"""A plain numpy reference of the RBF covariance (kernels_cov.hpp: cov_rbf1_kernel + cov_rbf_finish_kernel), the clouds the RBF
tests share, and the bound they hold the engine to. numpy only: no engine code, no oracle call.

  rbf_reference     the formula in fp64: W = sum w, m = sum w d / W, C = sum w d d^T / W - m m^T with d = p - x and
                    w = exp(-kernel_width |d|^2). Only the neighbour SET is decided in fp32, exactly as the engine and the oracle
                    decide it: sq = (dx*dx + dy*dy) + dz*dz in float, kept iff sq <= float(max_dist) * float(max_dist).
  rbf_emulate_fp32  the kernel's arithmetic restated in numpy float32: lane l adds the candidates at position l of every tile of
                    the Morton-sorted cloud in ascending tile order, the 64 lane totals meet in fp64, rbf_cov_from_sums, fp32 storage.
                    (Tiles the kernel culls hold no in-radius candidate: every term they would add is 0.f, so sweeping them all is the
                    same sum.) Not bit-exact -- numpy's float exp is not the device's, and the compiler may fuse a multiply-add --
                    but the same number of roundings in the same places: it says what fp32 sums of this shape cost.
  rbf_bound         |got - ref|max <= 5e-5 (|ref|max + |m|^2) + 1e-12 per query.
  CASES             every cloud / parameter pair of tests/test_gpu_rbf.py, so that tests/test_rbf_ref_cpu.py can check on the
                    reference side that the bound holds for fp32 sums and still sees ONE wrong candidate.
"""
import numpy as np

REL = 5e-5          # the project's figure for these fp32 sums (test_covariances_rbf_match_oracle, test_c3_rbf_covariances)
ABS = 1e-12
PAD = np.float32(3.0e18)         # load_candidate: the coordinates of a slot past the end of the cloud
MAX_DIST_SQ_CAP = np.float32(1e37)  # calc_cov_rbf: the fp32 max_dist^2 stays below the padding's squared distance (2.7e37)


def max_dist_sq_f32(max_dist):
    with np.errstate(over="ignore"):
        md = np.float32(max_dist)
        return np.float32(md * md)


def _sq_f32(c, q):
    """fp32 (dx*dx + dy*dy) + dz*dz of candidates c (m, 3) against queries q (k, 3) -> (k, m); every product and sum rounds to float"""
    dx = c[None, :, 0] - q[:, None, 0]
    dy = c[None, :, 1] - q[:, None, 1]
    dz = c[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def rbf_reference(pts_f32, kernel_width, max_dist, queries=None, chunk=4096, q_chunk=1024, want_pairs=False):
    """(W, m, C) in fp64 for the points `queries` (original indices; default: all): W (q,), m (q, 3) the weighted mean OFFSET from the
    query, C (q, 3, 3) the raw covariance. want_pairs: also the (query row, candidate index) pairs inside the radius."""
    pts = np.ascontiguousarray(pts_f32, np.float32)
    assert pts.ndim == 2 and pts.shape[1] == 3
    n = len(pts)
    queries = np.arange(n) if queries is None else np.asarray(queries, np.int64)
    nq = len(queries)
    md2 = max_dist_sq_f32(max_dist)
    p64 = pts.astype(np.float64)
    S = np.zeros((10, nq))
    pairs = []
    for q0 in range(0, nq, q_chunk):
        qi = queries[q0:q0 + q_chunk]
        for c0 in range(0, n, chunk):
            sq = _sq_f32(pts[c0:c0 + chunk], pts[qi])
            r, c = np.nonzero(sq <= md2)
            if not len(r):
                continue
            w = np.exp(-float(kernel_width) * sq[r, c].astype(np.float64))
            d = p64[c0 + c] - p64[qi[r]]  # exact: a difference of two floats in fp64 (the oracle's (double)p - x)
            terms = (w, w * d[:, 0], w * d[:, 1], w * d[:, 2], w * d[:, 0] * d[:, 0], w * d[:, 0] * d[:, 1], w * d[:, 0] * d[:, 2],
                     w * d[:, 1] * d[:, 1], w * d[:, 1] * d[:, 2], w * d[:, 2] * d[:, 2])
            for k, t in enumerate(terms):
                S[k, q0:q0 + len(qi)] += np.bincount(r, weights=t, minlength=len(qi))
            if want_pairs:
                pairs.append(np.stack([q0 + r, c0 + c], 1))
    W, m, C = _cov_from_sums(S)
    if want_pairs:
        return W, m, C, (np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64))
    return W, m, C


def _cov_from_sums(S):
    """rbf_cov_from_sums (and the oracle's last line): m = S_d / W, C = S_dd / W - m m^T, fp64"""
    W = S[0]
    iw = 1.0 / W
    m = (S[1:4] * iw).T
    C = np.empty((S.shape[1], 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = S[4 + k] * iw - m[:, a] * m[:, b]
    return W, m, C


def rbf_emulate_fp32(pts_f32, kernel_width, max_dist, queries, order, drop_tile=None):
    """The kernel's sums in numpy float32 -> (W, m, C32): C32 (q, 3, 3) float32 as get_covariances returns it (method NONE).
    order: the Morton order (original index per sorted position; any permutation states the same arithmetic).
    drop_tile = (query, tile): the MUTANT -- that tile of the sorted cloud is left out of that query's sums (query: an original index)."""
    pts = np.ascontiguousarray(pts_f32, np.float32)
    n = len(pts)
    order = np.asarray(order, np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "order must be a permutation"
    queries = np.asarray(queries, np.int64)
    nq = len(queries)
    ntiles = (n + 63) // 64
    sp = np.full((ntiles * 64, 3), PAD, np.float32)  # load_candidate's far-away slots behind the last point
    sp[:n] = pts[order]
    q = pts[queries]
    kw = np.float32(kernel_width)
    md2 = np.minimum(max_dist_sq_f32(max_dist), MAX_DIST_SQ_CAP)
    acc = np.zeros((10, nq, 64), np.float32)  # ten sums per (query, lane)
    drop_row = None
    if drop_tile is not None:
        drop_row = np.nonzero(queries == drop_tile[0])[0]
        assert len(drop_row), "the mutant's query is not among the queries"
    with np.errstate(over="ignore", under="ignore"):
        for t in range(ntiles):
            c = sp[t * 64:(t + 1) * 64]
            dx = c[None, :, 0] - q[:, None, 0]
            dy = c[None, :, 1] - q[:, None, 1]
            dz = c[None, :, 2] - q[:, None, 2]
            sq = (dx * dx + dy * dy) + dz * dz
            w = np.where(sq > md2, np.float32(0), np.exp(-kw * sq)).astype(np.float32)
            if drop_row is not None and t == drop_tile[1]:
                w[drop_row] = 0
            if not w.any():
                continue  # (adds 0.f to every sum)
            wx, wy, wz = w * dx, w * dy, w * dz
            for k, term in enumerate((w, wx, wy, wz, wx * dx, wx * dy, wx * dz, wy * dy, wy * dz, wz * dz)):
                acc[k] += term
    W, m, C = _cov_from_sums(acc.astype(np.float64).sum(axis=2))  # wave_sum: the 64 lane totals in fp64
    return W, m, C.astype(np.float32)


def rbf_bound(ref_C, ref_m):
    """per query: 5e-5 (|ref|max + |m|^2) + 1e-12. The kernel forms XX / W - mx^2: a query at the edge of its neighbourhood loses
    |m|^2 / |C| digits by construction, so the error of the sums scales with the second MOMENT, not with the covariance."""
    return REL * (np.abs(ref_C).max(axis=(1, 2)) + (np.asarray(ref_m) ** 2).sum(axis=1)) + ABS


def rbf_error(got_C, ref_C):
    return np.abs(np.asarray(got_C, np.float64) - ref_C).max(axis=(1, 2))


def sensitivity(pts_f32, kernel_width, max_dist, W, counts):
    """min over the queries with at least two neighbours of (smallest weight a neighbour can have) / W: the relative change of the sums
    when ONE candidate at the radius is lost or gained. A neighbour is no farther than max_dist and no farther than the diagonal of
    the cloud's bounding box (the only limit when max_dist is 'no limit'). inf if no query has two neighbours."""
    pts = np.asarray(pts_f32, np.float64)
    far_sq = min(float(max_dist) ** 2, float(((pts.max(0) - pts.min(0)) ** 2).sum()))
    sel = np.asarray(counts) >= 2
    return float(np.exp(-float(kernel_width) * far_sq) / np.asarray(W)[sel].max()) if sel.any() else np.inf


# ---------------------------------------------------------------------------------------------------------------------
# the clouds of tests/test_gpu_rbf.py
# ---------------------------------------------------------------------------------------------------------------------
# points per unit volume: W < ~44 at (0.5, 2.5), < ~11 at (0.5, 3.0), < ~290 at (5.0, 0.5) keeps exp(-kw md^2) / W >= 1e-3
DENSITY = {(0.5, 2.5): 1.0, (0.5, 3.0): 0.15, (5.0, 0.5): 16.0}


def uniform_cloud(n, density, seed):
    """n points uniform in the cube that holds them at `density` points per unit volume"""
    side = (n / density) ** (1.0 / 3.0)
    return (np.random.default_rng(seed).uniform(0.0, side, size=(n, 3))).astype(np.float32)


def lattice_cloud(m=12):
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).copy()


def morton_order(pts_f32, bits=10):
    """a Morton order of the cloud on its bounding cube (a stand-in for the engine's on a machine without one: tiles are compact boxes)"""
    pts = np.asarray(pts_f32, np.float64)
    lo = pts.min(0)
    extent = max(float((pts.max(0) - lo).max()), 1e-6)
    q = np.minimum((1 << bits) - 1, ((pts - lo) * ((1 << bits) / extent)).astype(np.int64))
    key = np.zeros(len(pts), np.int64)
    for b in range(bits):
        for a in range(3):
            key |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return np.argsort(key, kind="stable")


def min_pair_distance(pts_f32):
    pts = np.asarray(pts_f32, np.float32)
    best = np.inf
    for c0 in range(0, len(pts), 1024):
        sq = _sq_f32(pts, pts[c0:c0 + 1024]).astype(np.float64)
        sq[np.arange(len(sq)), c0 + np.arange(len(sq))] = np.inf
        best = min(best, sq.min())
    return float(np.sqrt(best))


SIZES = (1, 2, 63, 64, 65, 130, 4095, 4096, 4097, 8191)
N_BIG = 262144 + 64 + 1
OFFSET = np.array([1000.0, -2000.0, 50.0], np.float32)
BELOW_TWO = float(np.nextafter(np.float32(2.0), np.float32(0.0)))


def size_cloud(n):
    if n == 2:
        return np.array([[0, 0, 0], [100, 0, 0]], np.float32)  # far apart: each point alone inside its radius
    return uniform_cloud(n, DENSITY[(0.5, 2.5)], 1000 + n)


def big_cloud():
    return uniform_cloud(N_BIG, DENSITY[(5.0, 0.5)], 77)


def big_queries(order):
    """the first 64 and the last 256 positions of the Morton order, plus 200 random points"""
    order = np.asarray(order, np.int64)
    return np.unique(np.concatenate([order[:64], order[-256:], np.random.default_rng(78).choice(len(order), 200, replace=False)]))


def param_cloud(kw, md):
    return uniform_cloud(4097, DENSITY[(kw, md)], 2000 + int(10 * md))


def wide_cloud():
    return np.random.default_rng(31).uniform(0.0, 2.0, size=(600, 3)).astype(np.float32)  # diagonal 3.47 < max_dist 4


def ragged_cloud():
    return np.random.default_rng(32).uniform(0.0, 1.0, size=(130, 3)).astype(np.float32)


def offset_cloud():
    return param_cloud(0.5, 2.5) + OFFSET  # translated in fp32: the reference sees the same rounded coordinates


def isolated_case():
    pts = param_cloud(0.5, 2.5)
    return pts, 0.5, 0.5 * min_pair_distance(pts)


def cases():
    """name -> (points, kernel_width, max_dist): every cloud and parameter pair the GPU test compares with rbf_reference, but the big one
    (big_cloud: its queries depend on the Morton order) and the isolated one (isolated_case: no query has a neighbour)"""
    out = {}
    for n in SIZES:
        out["size %d" % n] = (size_cloud(n), 0.5, 2.5)
    for kw, md in ((0.5, 2.5), (0.5, 3.0), (5.0, 0.5)):
        out["params (%g, %g)" % (kw, md)] = (param_cloud(kw, md), kw, md)
    out["wide radius"] = (wide_cloud(), 0.02, 4.0)
    for md in (2.0, BELOW_TWO, 3.0):
        for kw in (0.1, 0.0):
            out["lattice kw %g md %.9g" % (kw, md)] = (lattice_cloud(), kw, md)
    out["offset"] = (offset_cloud(), 0.5, 2.5)
    out["ragged no limit kw 0"] = (ragged_cloud(), 0.0, 1e30)
    out["ragged no limit kw 0.5"] = (ragged_cloud(), 0.5, 1e30)
    return out
