"""cov_rbf1_kernel + cov_rbf_finish_kernel against the plain fp64 reference of tests/rbf_ref.py, at the sizes where the box levels
change, on the radius, with nothing inside it, with no radius at all, for every regularisation, on both sides, and on a reused handle.

Raw sums (method NONE) are held to   |got - ref|max <= 5e-5 (|ref|max + |m|^2) + 1e-12   per query (rbf_ref.rbf_bound; what fp32 sums
use of it, and that it still sees one wrong candidate, is checked without a GPU in tests/test_rbf_ref_cpu.py). Regularised covariances
are held to the oracle through util.cov_error_bound(input_rel=5e-5) as in test_gpu_parity.py. Every test prints how much of its bound it
used. All inputs are finite.
Measured on an MI355X when the tests were written: raw sums use 0.0006 .. 0.0027 of the bound (sizes 63 .. 8191: 0.0010 .. 0.0017;
262,209 points: 0.0019; (0.5, 3.0): 0.0027; (5.0, 0.5): 0.0024; lattice: 0.0006 .. 0.0012; no radius limit: 0.0008), the float32
emulation of tests/rbf_ref.py 0.0006 .. 0.0020 on the same clouds; the regularised methods at most 0.0001 of theirs."""
import functools

import numpy as np
import pytest

from tests import rbf_ref as R
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _core(kw, md, **params):
    from fast_gicp_amd import capi
    c = capi.VGICPCore(0)
    if params:
        c.set_engine_params(**params)
    c.set_kernel_params(kw, md)
    return c


def _engine(pts, kw, md, method=0, which="source", core=None):
    """covariances (n, 3, 3) float32 of one cloud on a fresh handle (or on `core`)"""
    c = core or _core(kw, md)
    c.set_kernel_params(kw, md)
    getattr(c, "set_%s_cloud" % which)(pts)
    getattr(c, "calculate_%s_covariances_rbf" % which)(method)
    got = c.get_covariances(which)
    if core is None:
        c.close()
    return got


def _hold_to_reference(name, got, pts, kw, md, queries=None):
    """raw covariances of the engine against rbf_reference, every query against its bound; returns the reference's (W, m, C, pairs)"""
    W, m, C, pairs = R.rbf_reference(pts, kw, md, queries, want_pairs=True)
    got = np.asarray(got, np.float64)
    got = got if queries is None else got[queries]
    assert np.isfinite(got).all(), "%s: %d non-finite covariances" % (name, int((~np.isfinite(got)).any(axis=(1, 2)).sum()))
    ratio = R.rbf_error(got, C) / R.rbf_bound(C, m)
    print("%s: n %d, %d queries, neighbours max %d, W max %.1f: uses %.4f of the bound" % (name, len(pts), len(C), np.bincount(pairs[:, 0]).max(), W.max(), ratio.max()))
    assert ratio.max() <= 1.0, (name, float(ratio.max()), int(np.argmax(ratio)))
    return W, m, C, pairs


@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_where_the_box_levels_change(n):
    """one / two tiles (64 / 65), a ragged last tile whose padded lanes must weigh nothing (63, 65, 130, 4095, 4097, 8191), one / two
    super boxes (4096 / 4097); every query compared. A point alone inside its radius (n = 1; n = 2 far apart) has W = 1 and C = 0 exactly."""
    pts = R.size_cloud(n)
    got = _engine(pts, 0.5, 2.5)
    if n <= 2:
        assert np.array_equal(got, np.zeros((n, 3, 3), np.float32))
    _hold_to_reference("size %d" % n, got, pts, 0.5, 2.5)


def test_second_pass_of_the_super_box_loop():
    """More than 64 super boxes (n > 262,144: the loop over 64 super boxes per ballot takes a second trip, and the sort its 3 x 9-bit
    route): the queries at both ends of the Morton order and 200 random ones, on a sparse cloud (about 8 neighbours)."""
    pts = R.big_cloud()
    c = _core(5.0, 0.5)
    got = _engine(pts, 5.0, 0.5, core=c)
    order, _ = c.debug_spatial_order("source")
    c.close()
    assert np.array_equal(np.sort(order), np.arange(len(pts)))
    q = R.big_queries(order)
    W, m, C, pairs = _hold_to_reference("second pass", got, pts, 5.0, 0.5, q)
    pos = np.empty(len(pts), np.int64)
    pos[order] = np.arange(len(pts))
    assert (pos[pairs[:, 1]] >= 262144).any(), "no compared query has a neighbour behind the first 64 super boxes"
    assert R.sensitivity(pts, 5.0, 0.5, W, np.bincount(pairs[:, 0], minlength=len(q))) >= 1e-3  # (with the engine's order; the stand-in order: test_rbf_ref_cpu)


@pytest.mark.parametrize("kw,md", [(0.5, 2.5), (0.5, 3.0), (5.0, 0.5)])
def test_parameter_pairs(kw, md):
    pts = R.param_cloud(kw, md)
    _hold_to_reference("params (%g, %g)" % (kw, md), _engine(pts, kw, md), pts, kw, md)


def test_radius_larger_than_the_cloud():
    """nothing is culled: every point is a neighbour of every point"""
    pts = R.wide_cloud()
    W, m, C, pairs = _hold_to_reference("wide radius", _engine(pts, 0.02, 4.0), pts, 0.02, 4.0)
    assert len(pairs) == len(pts) ** 2


def test_isolated_queries_are_exactly_zero():
    """a radius below the smallest pair distance: W = 1 (the query itself, sq = 0, weight 1) and C = 0 exactly"""
    pts, kw, md = R.isolated_case()
    got = _engine(pts, kw, md)
    assert np.array_equal(got, np.zeros((len(pts), 3, 3), np.float32)), int(np.any(got != 0, axis=(1, 2)).sum())


@pytest.mark.parametrize("md,interior", [(2.0, 33), (R.BELOW_TWO, 27), (3.0, 123)])
def test_candidates_exactly_on_the_radius(md, interior):
    """A 12 x 12 x 12 integer lattice: sq is exact, so candidates sit ON the radius. sq == max_dist^2 is in (the cut is sq > max_dist_sq),
    with the largest float below 2.0 it is out; sq == 9 comes as (3,0,0) and (2,2,1). A '>=' cut, or a box bound that cuts a touching
    tile, loses neighbours whose weight is far above the bound. With kernel_width = 0 every neighbour weighs 1: the covariance is that
    of the neighbour SET, whose size the reference counts (interior points: 33 / 27 / 123)."""
    pts = R.lattice_cloud()
    for kw in (0.1, 0.0):
        W, m, C, pairs = _hold_to_reference("lattice kw %g md %.9g" % (kw, md), _engine(pts, kw, md), pts, kw, md)
        counts = np.bincount(pairs[:, 0], minlength=len(pts))
        assert counts.max() == interior
        if kw == 0.0:
            assert np.array_equal(W, counts.astype(np.float64))


def test_offset_cloud():
    """the n = 4097 cloud translated by (1000, -2000, 50) in fp32: the kernel sums offsets from the query, not coordinates"""
    pts = R.offset_cloud()
    _hold_to_reference("offset", _engine(pts, 0.5, 2.5), pts, 0.5, 2.5)


@functools.lru_cache(maxsize=None)
def _oracle_regularised(method):
    from oracle import oracle
    return oracle.covariances_rbf(R.param_cloud(0.5, 2.5), 0.5, 2.5, method)


@pytest.mark.parametrize("which", ["source", "target"])
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4])
def test_every_regularisation_on_both_sides(O, method, which):
    """cov_rbf_finish_kernel runs regularize_cov for NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE and FROBENIUS.
    Eigen-based methods: every point against util.cov_error_bound (input error 5e-5, amplified by lambda_max / gap), at most 5 points
    with undefined eigenvectors set aside. FROBENIUS, R = A |A^-1|_F with A = C + 1e-3 I, has no eigenvectors: to first order
    |dR|_2 <= s |dA|_2 (1 + cond A) with s = |A^-1|_F <= 3 |R|max / lambda_max(A) and |dA|_2 <= 3 |dC|max, so
    |dR|max <= 18 |R|max |dC|max / lambda_min(A), |dC|max being the bound of the raw sums; plus fp32 storage."""
    pts = R.param_cloud(0.5, 2.5)
    got = _engine(pts, 0.5, 2.5, method, which).astype(np.float64)
    if method == 0:
        _hold_to_reference("NONE %s" % which, got, pts, 0.5, 2.5)
        return
    ref, raw = _oracle_regularised(method), _oracle_regularised(0)
    if method == 4:
        _, m, C = R.rbf_reference(pts, 0.5, 2.5)
        scale = np.abs(ref).max(axis=(1, 2))
        bound = scale * (1.2e-7 + 18.0 * R.rbf_bound(C, m) / (np.linalg.eigvalsh(raw)[:, 0] + 1e-3))
        err = R.rbf_error(got, ref)
        degenerate = np.zeros(len(pts), bool)
    else:
        err, bound, degenerate = util.cov_error_bound(got, ref, raw, input_rel=5e-5, gaps="01" if method == 3 else "min")
    print("method %d %s: uses %.4f of the bound, %d degenerate" % (method, which, (err / bound)[~degenerate].max(), int(degenerate.sum())))
    assert degenerate.sum() <= 5
    assert np.all(err[~degenerate] <= bound[~degenerate]), float((err / bound)[~degenerate].max())


@pytest.mark.parametrize("estimator", ["rbf", "knn"])
def test_cov_sorted_is_the_same_record_as_cov(estimator):
    """Clouds of coherent_min_points and up get their covariances a second time, in Morton order (CloudDev::cov_sorted), and the cost
    kernel reads that copy. set_source_covariances drops it: the same covariances handed back through the host must give the
    bit-identical linearisation (fixed-order reduction over the same walk)."""
    tgt = R.param_cloud(0.5, 2.5)
    near = np.argsort(((tgt.astype(np.float64) - tgt.astype(np.float64).mean(0)) ** 2).sum(1))[:300]  # a ball in the middle: same density
    src = (tgt[near].astype(np.float64) + np.array([0.05, -0.03, 0.02])).astype(np.float32)
    c = _core(0.5, 2.5, coherent_min_points=1)
    c.set_target_cloud(tgt); c.calculate_target_covariances_rbf(3); c.create_target_voxelmap()
    c.set_source_cloud(src)
    if estimator == "rbf":
        c.calculate_source_covariances_rbf(3)
    else:
        c.find_source_neighbors(20); c.calculate_source_covariances(3)
    T = util.random_pose(np.random.default_rng(3), 0.05, 0.01)
    e, H, b = c.linearize(T)
    assert c.get_num_correspondences() > 100 and e > 0
    cov = c.get_covariances("source")
    c.set_source_covariances(cov)  # fp32 -> fp64 -> fp32: the same records, without the sorted copy
    assert np.array_equal(c.get_covariances("source"), cov)
    e2, H2, b2 = c.linearize(T)
    assert e == e2 and np.array_equal(H, H2) and np.array_equal(b, b2), (e, e2)
    c.close()


def test_scratch_reuse_and_determinism():
    """The ten totals per query live in ONE engine-wide buffer with the cloud's size as its stride: clouds of different sizes in turn,
    and both sides, on one handle. A (4097), B (130), A again, A as the target: A three times to the bit, B as on a fresh handle."""
    A, B = R.param_cloud(0.5, 2.5), R.size_cloud(130)
    c = _core(0.5, 2.5)
    a1 = _engine(A, 0.5, 2.5, core=c)
    b1 = _engine(B, 0.5, 2.5, core=c)
    a2 = _engine(A, 0.5, 2.5, core=c)
    a3 = _engine(A, 0.5, 2.5, which="target", core=c)
    c.close()
    assert np.array_equal(a1, a2) and np.array_equal(a1, a3)
    assert np.array_equal(b1, _engine(B, 0.5, 2.5))


@pytest.mark.parametrize("kw", [0.0, 0.5])
def test_ragged_last_tile_with_no_radius_limit(kw):
    """n = 130 (last tile: 2 points, 62 padded lanes), max_dist = 1e30: max_dist^2 is +inf in fp32. Every point is a neighbour of every
    point; with kernel_width = 0 every covariance is the plain covariance of the cloud about its mean. The padded lanes are far-away
    candidates (3e18): with kernel_width = 0.5 their weight underflows to 0, with kernel_width = 0 only the radius cut keeps them out --
    and sq = 2.7e37 is not above +inf: before calc_cov_rbf clamped max_dist^2 below the padding's distance they entered the sums with
    weight 1 (non-finite covariances for every query)."""
    pts = R.ragged_cloud()
    W, m, C, pairs = _hold_to_reference("ragged no limit kw %g" % kw, _engine(pts, kw, 1e30), pts, kw, 1e30)
    assert len(pairs) == len(pts) ** 2
    if kw == 0.0:
        p = pts.astype(np.float64)
        plain = (p - p.mean(0)).T @ (p - p.mean(0)) / len(p)
        assert np.abs(C - plain).max() <= 1e-13
