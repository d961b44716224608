"""CPU tests: pin the oracle (the fp64 restatement of the reference's CPU FastVGICP) against every
known answer the reference holds for the hot path and against an independent numpy twin."""
import os

import numpy as np
import pytest

from tests import util


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


def test_readme_point_counts(O):
    """README.md:116 'target:17249[pts] source:17518[pts]' -- produced by ApproximateVoxelGrid(0.1) WITHOUT the
    origin filter that HEAD's align.cpp:127-133 added later; with the filter HEAD gives 17,047 / 17,334."""
    t, s = util.bundled_pair(origin_filter=False)
    assert (len(t), len(s)) == (17249, 17518)
    t, s = util.bundled_pair(origin_filter=True)
    assert (len(t), len(s)) == (17047, 17334)


def test_gicp_test_input_counts(O):
    """gicp_test.cpp:55-65: exact VoxelGrid leaf 0.2, no origin filter."""
    t, s = util.bundled_pair(origin_filter=False, leaf=0.2, exact_voxelgrid=True)
    assert (len(t), len(s)) == (7908, 8061)


def _gicp(O):
    g = O.FastVGICP()
    g.set_gicp_mode(True)
    return g


@pytest.mark.parametrize("method", ["VGICP", "NDT", "GICP"])
def test_gicp_test_scenarios(O, method):
    """The reference's only correctness pin (gicp_test.cpp:147-201): forward / backward / swap-and-set-source /
    swap-and-set-target, each within 0.05 m and 1 deg of data/relative.txt and converged."""
    t, s = util.bundled_pair(origin_filter=False, leaf=0.2, exact_voxelgrid=True)
    gt = util.relative_pose()
    make = {"VGICP": (lambda: O.FastVGICP()), "NDT": (lambda: O.NDT()), "GICP": (lambda: _gicp(O))}[method]

    def check(T, conv, label):
        te, re_ = util.pose_error(gt, T)
        assert te < 0.05 and re_ < np.radians(1.0) and conv, label

    reg = make()
    reg.set_target(t); reg.set_source(s)
    r = reg.align(); check(r["T"], r["converged"], "forward")
    reg.set_target(s); reg.set_source(t)
    r = reg.align(); check(np.linalg.inv(r["T"]), r["converged"], "backward")
    reg = make()
    reg.set_source(t); reg.swap(); reg.set_source(s)
    r = reg.align(); check(r["T"], r["converged"], "swap and set source")
    reg = make()
    reg.set_target(s); reg.swap(); reg.set_target(t)
    r = reg.align(); check(r["T"], r["converged"], "swap and set target")


@pytest.mark.parametrize("method", ["VGICP", "NDT"])
def test_gauss_newton_step(O, method):
    """step_gn (lsq_registration_impl.hpp:108-121; selected by lsq_optimizer_type_, :94-104): plain Gauss-Newton -- linearize, H d = -b by LDLT,
    x0 = exp(d) x0, no trial evaluation. On the gicp_test pair it meets the reference's tolerance like LM does, never evaluates the error
    alone, and one GN iteration from a pose IS the numpy solve of that pose's normal equations."""
    t, s = util.bundled_pair(origin_filter=False, leaf=0.2, exact_voxelgrid=True)
    g = O.FastVGICP(search=O.DIRECT7) if method == "VGICP" else O.NDT()
    g.set_optimizer("GN")
    g.set_target(t); g.set_source(s)
    r = g.align()
    te, re_ = util.pose_error(util.relative_pose(), r["T"])
    assert r["converged"] and te < 0.05 and re_ < np.radians(1.0)
    assert r["num_error_evals"] == 0 and r["num_linearize"] == r["iterations"]
    g.set_lm(max_iterations=1)
    r1 = g.align()
    g.prepare()
    e, H, b = g.linearize(np.eye(4))
    d = np.linalg.solve(H, -b)
    assert util.rel_err(r1["T"], O.se3_exp(d)) < 1e-9
    assert util.rel_err(r1["H"], H) < 1e-12


def test_readme_fitness_band(O):
    """README.md:126-128 vgicp fitness 0.204067 (stale revision) -> +-1 % sanity band (SURVEY 6 caveat 3)."""
    t, s = util.bundled_pair(origin_filter=True)
    g = O.FastVGICP()
    g.set_target(t); g.set_source(s)
    r = g.align()
    f = g.fitness()
    assert abs(f - 0.204067) / 0.204067 < 0.01
    # values recorded in SURVEY 8(c)(4) for HEAD preprocessing, res 1.0, DIRECT1
    assert r["iterations"] == 4
    np.testing.assert_allclose(r["T"][:3, 3], [0.498359, 0.117208, -0.029736], atol=2e-6)
    assert abs(f - 0.205022) < 2e-6


def test_readme_fitness_band_fastgicp(O):
    """README.md:122-124 fgicp_st 0.204379 / fgicp_mt 0.204412 -> +-1 % band for the FastGICP (nearest-point) restatement."""
    t, s = util.bundled_pair(origin_filter=True)
    g = _gicp(O)
    g.set_target(t); g.set_source(s)
    r = g.align()
    assert r["converged"]
    assert abs(g.fitness() - 0.204379) / 0.204379 < 0.01


def test_direct27_recorded_values(O):
    t, s = util.bundled_pair(origin_filter=True)
    g = O.FastVGICP(search=O.DIRECT27)
    g.set_target(t); g.set_source(s)
    r = g.align()
    np.testing.assert_allclose(r["T"][:3, 3], [0.503962, 0.074634, -0.025146], atol=2e-6)
    assert abs(g.fitness() - 0.198792) < 2e-6
    coords, num, _, _ = g.get_voxelmap()
    assert len(coords) == 1087 and num.max() == 171 and num.sum() == len(t)


# ---------------------------------------------------------------------------------------------
# independent numpy / scipy twin
# ---------------------------------------------------------------------------------------------
def test_knn_vs_scipy(O):
    from scipy.spatial import cKDTree
    _, s = util.bundled_pair()
    s = s[:4000]
    idx = O.knn(s, 20)
    d, ref = cKDTree(s.astype(np.float64)).query(s.astype(np.float64), k=20)
    # same neighbour sets wherever the 20th/21st distances are not (nearly) tied
    d21 = cKDTree(s.astype(np.float64)).query(s.astype(np.float64), k=21)[0][:, 20]
    clear = (d21 - d[:, 19]) > 1e-5
    same = np.array([set(a) == set(b) for a, b in zip(idx, ref)])
    assert same[clear].all()
    assert (idx[:, 0] == np.arange(len(s))).mean() > 0.99  # self is the nearest neighbour


def test_covariance_and_regularisation_vs_numpy(O):
    from tests import np_twin
    _, s = util.bundled_pair()
    s = s[:3000]
    idx = O.knn(s, 20)
    for reg in (O.NONE, O.PLANE, O.MIN_EIG, O.NORMALIZED_MIN_EIG, O.FROBENIUS):
        got = O.covariances_knn(s, 20, reg, idx=idx)
        ref = np_twin.covariances(s, idx, reg)
        err = np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
        assert np.quantile(err, 0.999) < 1e-7, (reg, err.max())


def test_voxelmap_and_linearize_vs_numpy(O):
    from tests import np_twin
    t, s = util.bundled_pair()
    t, s = t[:5000], s[:5000]
    ct, cs = O.covariances_knn(t, 20, O.PLANE), O.covariances_knn(s, 20, O.PLANE)
    coords, num, means, covs = O.voxelmap_vgicp(t, ct, 1.0)
    vm = np_twin.voxelmap(t, ct, 1.0)
    assert set(map(tuple, coords)) == set(vm)
    for c, n, m, cv in zip(coords, num, means, covs):
        n2, m2, c2 = vm[tuple(c)]
        assert n == n2
        np.testing.assert_allclose(m, m2, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(cv, c2, rtol=1e-12, atol=1e-14)
    for search in (O.DIRECT1, O.DIRECT7, O.DIRECT27):
        g = O.FastVGICP(search=search)
        g.set_target(t); g.set_source(s); g.set_target_covs(ct); g.set_source_covs(cs); g.prepare()
        T = util.random_pose(np.random.default_rng(3), 1.0, 0.3)
        e, H, b = g.linearize(T)
        e2, H2, b2, nc = np_twin.linearize(s, cs, vm, 1.0, O.neighbor_offsets(search), T)
        assert nc == g.num_correspondences()
        assert abs(e - e2) < 1e-10 * abs(e2)
        assert util.rel_err(H, H2) < 1e-10 and util.rel_err(b, b2) < 1e-10


@pytest.mark.parametrize("mode", ["P2D", "D2D"])
def test_ndt_linearize_vs_numpy(O, mode):
    """The NDT sums of the oracle against their numpy twin (np_twin.ndt_linearize: Cauchy weight, voxels of at most 6 points skipped, D2D on
    the source voxels' means and covariances) over the oracle's own voxel records, to the tolerance of the VGICP leg above."""
    from tests import np_twin
    t, s = util.bundled_pair()
    t, s = t[:5000], s[:5000]
    d2d = mode == "D2D"
    for search in (O.DIRECT1, O.DIRECT7):
        g = O.NDT(mode=O.D2D if d2d else O.P2D, search=search)
        g.set_target(t); g.set_source(s); g.prepare()
        vm = util.voxel_dict(*g.get_voxelmap("target"))
        assert sum(1 for v in vm.values() if v[0] > 6) > 20 and sum(1 for v in vm.values() if v[0] <= 6) > 20  # both kinds of voxel take part
        recs = list(zip(*g.get_voxelmap("source")[1:])) if d2d else None
        T = util.random_pose(np.random.default_rng(3), 1.0, 0.3)
        e, H, b = g.linearize(T)
        e2, H2, b2, nc = np_twin.ndt_linearize(s, recs, vm, 1.0, O.neighbor_offsets(search), T, d2d)
        assert nc == g.num_correspondences() and nc > 100
        assert abs(e - e2) < 1e-10 * abs(e2)
        assert util.rel_err(H, H2) < 1e-10 and util.rel_err(b, b2) < 1e-10


def test_se3_exp_vs_scipy(O):
    from scipy.linalg import expm
    rng = np.random.default_rng(0)
    for scale in (1e-7, 1e-3, 0.3, 2.0):
        a = rng.normal(size=6) * scale
        W = np.zeros((4, 4))
        W[:3, :3] = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
        W[:3, 3] = a[3:]
        np.testing.assert_allclose(O.se3_exp(a), expm(W), atol=1e-12)


def test_ndt_voxelmap_vs_numpy(O):
    t, _ = util.bundled_pair()
    t = t[:6000]
    coords, num, means, covs = O.voxelmap_ndt(t, 1.0)
    keys = np.floor(t.astype(np.float64) / 1.0 - 0.5).astype(np.int64)
    for c, n, m, cv in list(zip(coords, num, means, covs))[:200]:
        sel = t[(keys == c).all(axis=1)].astype(np.float64)
        assert len(sel) == n
        np.testing.assert_allclose(m, sel.mean(axis=0), atol=1e-12)
        C = (sel - sel.mean(0)).T @ (sel - sel.mean(0)) / n
        w, V = np.linalg.eigh(C)
        ref = (V * np.maximum(w, 1e-3)) @ V.T
        np.testing.assert_allclose(cv, ref, atol=1e-9)


def test_rbf_covariance_vs_numpy(O):
    _, s = util.bundled_pair()
    s = s[:1500]
    got = O.covariances_rbf(s, 0.5, 2.5, O.NONE)
    p = s.astype(np.float64)
    for i in range(0, len(s), 97):
        d = p - p[i]
        sq = (s[:, 0] - s[i, 0]) ** 2 + (s[:, 1] - s[i, 1]) ** 2 + (s[:, 2] - s[i, 2]) ** 2
        m = sq <= np.float32(2.5) ** 2
        w = np.exp(-0.5 * sq[m].astype(np.float64))
        mu = (w[:, None] * p[m]).sum(0) / w.sum()
        C = ((w[:, None, None] * p[m][:, :, None] * p[m][:, None, :]).sum(0) - np.outer(mu, (w[:, None] * p[m]).sum(0))) / w.sum()
        np.testing.assert_allclose(got[i], C, atol=1e-9 * max(1, np.abs(p[i]).max() ** 2))


def test_product_preprocessing_matches_oracle(O):
    """fast_gicp_amd.preprocess (product host code) against the oracle restatement and the README counts."""
    from fast_gicp_amd import preprocess as P
    t, s = P.bundled_pair(util.DATA)
    ot, os_ = util.bundled_pair()
    assert np.array_equal(t, ot) and np.array_equal(s, os_)
    t2, s2 = P.bundled_pair(util.DATA, origin_filter=False)
    assert (len(t2), len(s2)) == (17249, 17518)


def test_no_overlap_returns_guess_converged(O):
    """H = 0 / lambda = 0 (no correspondences): Eigen::LDLT's pseudo-inverse gives d = 0, the reference accepts delta = I
    and reports the guess as converged (lsq_registration_impl.hpp:111-168). The restated solver must not produce NaN."""
    rng = np.random.default_rng(0)
    tgt = rng.uniform(-5, 5, size=(1500, 3)).astype(np.float32)
    src = (rng.uniform(-5, 5, size=(1200, 3)) + np.array([500.0, 0, 0])).astype(np.float32)
    guess = util.random_pose(np.random.default_rng(1), 1.0, 0.2)
    for g in (O.FastVGICP(search=O.DIRECT7), O.NDT()):
        g.set_target(tgt); g.set_source(src)
        r = g.align(guess)
        assert r["converged"] and np.array_equal(r["T"], guess)
        assert r["num_linearize"] == 1 and r["num_error_evals"] == 1


def test_multiplicative_voxels_against_numpy(O):
    """MultiplicativeGaussianVoxel (fast_vgicp_voxel.hpp:79-103): cov = (sum C_i^-1)^-1, mean = cov * sum C_i^-1 p_i, num_points
    counted as usual -- the oracle's restatement against plain numpy on a small cloud, and the additive mode untouched."""
    tgt, _, _ = util.synthetic_pair(3000, 10, seed=5, extent=10.0)
    covs = O.covariances_knn(tgt, 20, O.PLANE)
    coords, num, means, vc = O.voxelmap_vgicp(tgt, covs, 1.0, O.MULTIPLICATIVE)
    keys = np.floor(tgt.astype(np.float64) / 1.0 - 0.5).astype(np.int64)
    assert int(num.sum()) == len(tgt) and len(np.unique(keys, axis=0)) == len(coords)
    for s in np.random.default_rng(0).integers(0, len(coords), 60):
        m = (keys == coords[s]).all(1)
        ci = np.linalg.inv(covs[m])
        cov = np.linalg.inv(ci.sum(0))
        mean = cov @ np.einsum("nij,nj->i", ci, tgt[m].astype(np.float64))
        assert num[s] == m.sum()
        np.testing.assert_allclose(vc[s], cov, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(means[s], mean, rtol=1e-9, atol=1e-9)
    ca, na, ma, va = O.voxelmap_vgicp(tgt, covs, 1.0, O.ADDITIVE)
    cw, nw, mw, vw = O.voxelmap_vgicp(tgt, covs, 1.0, O.ADDITIVE_WEIGHTED)  # same voxel type in the reference (:137-141)
    assert np.array_equal(ca, cw) and np.array_equal(ma, mw) and np.array_equal(va, vw)
    assert not np.allclose(va, vc)


# ---------------------------------------------------------------------------------------------
# "cuda-compat" leg: the fp32 restatement of the reference's DEVICE path (oracle/cuda_compat.cpp)
# ---------------------------------------------------------------------------------------------
def test_cuda_compat_eigensolver_vs_lapack(O):
    """Eigen's computeDirect (closed form, float) as restated: eigenvalues ascending, orthonormal vectors, A V = V diag(w) to the
    accuracy the method has in float (it is known to be less accurate than an iterative solver: a few 1e-4 of |A| on flat
    point-neighbourhood covariances), and the PLANE / MIN_EIG reconstructions against the fp64 oracle's."""
    rng = np.random.default_rng(5)
    worst_w = worst_res = worst_plane = 0.0
    for trial in range(400):
        B = rng.normal(size=(3, 3)) * rng.uniform(0.02, 2.0, size=3)   # anisotropic, like a planar neighbourhood
        A = (B @ B.T).astype(np.float32).astype(np.float64)
        w, V = O.cc_eig3(A)
        wl = np.linalg.eigvalsh(A)
        assert np.all(np.diff(w) >= -1e-6 * abs(wl).max())
        worst_w = max(worst_w, np.abs(w - wl).max() / abs(wl).max())
        worst_res = max(worst_res, np.abs(A @ V - V * w).max() / abs(wl).max())
        assert np.abs(V.T @ V - np.eye(3)).max() < 2e-3
        gap = (wl[1] - wl[0]) / wl[2]
        if gap > 0.05:  # PLANE only depends on the smallest eigenvector: compare where it is well defined
            worst_plane = max(worst_plane, np.abs(O.cc_regularize(A, O.PLANE) - O.regularize(A, O.PLANE)).max())
    assert worst_w < 2e-5 and worst_res < 5e-4 and worst_plane < 2e-2, (worst_w, worst_res, worst_plane)
    # degenerate inputs take Eigen's branches: all eigenvalues equal -> identity vectors; two equal -> re-orthogonalised pair
    w, V = O.cc_eig3(np.eye(3) * 0.25)
    assert np.allclose(w, 0.25) and np.array_equal(V, np.eye(3))
    w, V = O.cc_eig3(np.diag([1.0, 1.0, 0.01]))
    assert np.allclose(sorted(w), [0.01, 1.0, 1.0], atol=2e-4) and np.abs(V.T @ V - np.eye(3)).max() < 1e-5  # (a double root: the closed form keeps half of float's digits)


def test_cuda_compat_recorded_values(O):
    """SURVEY 8c(4)'s fp32 twin of the reference's CUDA path, recorded when the survey was written (numpy + LAPACK eigh + cKDTree):
    bundled pair, HEAD preprocessing, resolution 1.0 -- DIRECT1: fitness 0.204998, correspondence counts 14,990 -> 16,124 ->
    16,108 -> 16,104; DIRECT27: fitness 0.198996. The restatement here follows the .cu files more closely than that twin did
    (Eigen's closed-form eigen solver instead of LAPACK's, float tree sums): the first count depends on float voxel coordinates
    only and must be exact; the later ones and the fitness may move in the last recorded digits (the survey says so itself)."""
    t, s = util.bundled_pair(origin_filter=True)
    g = O.CudaCompatVGICP(search=O.DIRECT1)
    g.set_target(t); g.set_source(s)
    r = g.align()
    hist = g.corr_history()
    assert r["converged"] and r["iterations"] == 4 and len(hist) == 4
    assert hist[0] == 14990 and all(abs(a - b) <= 2 for a, b in zip(hist, [14990, 16124, 16108, 16104])), hist
    assert abs(g.fitness() - 0.204998) / 0.204998 < 5e-4, g.fitness()
    coords, num, means, covs = g.get_voxelmap()
    assert len(coords) == 1087 and num.max() == 171 and num.sum() == len(t)   # the same voxel set as the fp64 CPU class (Appendix B)
    g27 = O.CudaCompatVGICP(search=O.DIRECT27)
    g27.set_target(t); g27.set_source(s)
    r27 = g27.align()
    assert r27["converged"] and g27.corr_history()[0] == 209669   # Appendix B: N_c at the identity, DIRECT27
    assert abs(g27.fitness() - 0.198996) / 0.198996 < 5e-4, g27.fitness()
    # ... and how far the reference's two paths are from EACH OTHER (fp64 CPU class vs fp32 device path): a few 1e-4 of the pose --
    # the scale every "matches FastVGICP / FastVGICPCuda" tolerance has to be read against
    f = O.FastVGICP(search=O.DIRECT27)
    f.set_target(t); f.set_source(s)
    d = util.rel_err(r27["T"], f.align()["T"])
    assert 1e-5 < d < 1e-3, d


@pytest.mark.parametrize("method", ["VGICP_CUDA", "NDT_CUDA_D2D"])
def test_cuda_compat_gicp_test_scenarios(O, method):
    """gicp_test.cpp:147-201 instantiates exactly these device classes (NDTCuda in its default D2D mode): the float restatement has
    to pass the reference's own test. (P2D is not part of it -- both restatements land 0.059 m from relative.txt there -- and is
    held to the fp64 restatement below instead.)"""
    t, s = util.bundled_pair(origin_filter=False, leaf=0.2, exact_voxelgrid=True)
    gt = util.relative_pose()
    make = {"VGICP_CUDA": (lambda: O.CudaCompatVGICP()), "NDT_CUDA_D2D": (lambda: O.CudaCompatNDT(mode=O.D2D))}[method]

    def check(T, conv, label):
        te, re_ = util.pose_error(gt, T)
        assert te < 0.05 and re_ < np.radians(1.0) and conv, (label, te, re_)

    reg = make()
    reg.set_target(t); reg.set_source(s)
    r = reg.align(); check(r["T"], r["converged"], "forward")
    reg.set_target(s); reg.set_source(t)
    r = reg.align(); check(np.linalg.inv(r["T"]), r["converged"], "backward")
    reg = make()
    reg.set_source(t); reg.swap(); reg.set_source(s)
    r = reg.align(); check(r["T"], r["converged"], "swap and set source")
    reg = make()
    reg.set_target(s); reg.swap(); reg.set_target(t)
    r = reg.align(); check(r["T"], r["converged"], "swap and set target")


def test_cuda_compat_against_the_fp64_formulas(O):
    """The float leg against the fp64 restatements of the SAME formulas at a fixed pose: uncentred float covariances vs centred
    fp64 ones (before regularisation they are the same quantity), float voxel sums vs fp64 ones, float cost terms vs the fp64 NDT
    cost -- differences of float rounding size, nothing structural."""
    t, s = util.bundled_pair(origin_filter=True)
    s = s[:6000]
    g = O.CudaCompatVGICP(reg=O.NONE)          # (NONE: covariance_regularization.cu leaves the matrix alone)
    g.set_target(t); g.set_source(s)
    ref = O.covariances_knn(s, 20, O.NONE)
    got = g.get_covs("source")
    scale = np.abs(ref).max(axis=(1, 2))
    # uncentred float sums lose |p|^2 / |C| digits: points 70 m from the origin with 1e-3 m^2 covariances keep ~3 digits
    r2 = (s.astype(np.float64) ** 2).sum(1)
    assert np.all(np.abs(got - ref).max(axis=(1, 2)) <= 4e-6 * r2 + 1e-6 * scale)
    n = O.CudaCompatNDT(mode=O.D2D)
    n.set_target(t); n.set_source(s); n.prepare()
    f = O.NDT(mode=O.D2D)
    f.set_target(t); f.set_source(s); f.prepare()
    cc, cn, cm, cv = n.get_voxelmap("target")
    fc, fn, fm, fv = f.get_voxelmap("target")
    assert util.voxel_dict(cc, cn) == util.voxel_dict(fc, fn)
    T = util.relative_pose()
    e1, H1, b1 = n.linearize(T)
    e2, H2, b2 = f.linearize(T)
    assert n.num_correspondences() == f.num_correspondences()
    assert abs(e1 - e2) < 2e-3 * abs(e2) and util.rel_err(H1, H2) < 2e-3, (e1, e2, util.rel_err(H1, H2))
    for mode in (O.P2D, O.D2D):  # whole registrations: the float device path against the fp64 restatement of the same formulas
        a, b = O.CudaCompatNDT(mode=mode), O.NDT(mode=mode)
        for g in (a, b):
            g.set_target(t); g.set_source(s)
        ra, rb = a.align(), b.align()
        assert ra["converged"] and rb["converged"] and ra["iterations"] == rb["iterations"]
        assert util.rel_err(ra["T"], rb["T"]) < 1e-3, (mode, util.rel_err(ra["T"], rb["T"]))


def test_cuda_compat_order_spread(O):
    """How far the float device path moves when nothing but the ORDER of its float sums changes: the cuda-compat leg on the same clouds with the
    points permuted. The reference does not fix that order for its voxel sums (atomicAdd in arrival order, gaussian_voxelmap.cu:89-148), so this
    spread is the floor under any "parity with FastVGICPCuda / NDTCuda": measured k-NN covariances ~2e-6, RBF 1e-5 .. 2.3e-4 (the uncentred
    weighted sums over ~100 neighbours at 50 m range), NDT 1e-5 .. 6e-5 of the pose (fitness up to 1e-4 for NDT). The engine's CUDA_COMPAT mode and the oracle leg both take index order, which is why
    tests/test_gpu_cuda_compat.py can hold them to 1e-4 of each other; against the real device code only this spread could be promised."""
    from tests import util
    from fast_gicp_amd import workloads
    rng = np.random.default_rng(0)
    tgt, src = util.bundled_pair()
    for cov_mode, bound in ((0, 2e-5), (1, 1e-3)):
        def run(t, s):
            g = O.CudaCompatVGICP(search=O.DIRECT27, cov_mode=cov_mode)
            g.set_target(t); g.set_source(s)
            return g.align()
        base = run(tgt, src)
        d = [util.rel_err(run(tgt[rng.permutation(len(tgt))], src[rng.permutation(len(src))])["T"], base["T"]) for _ in range(2)]
        print("cuda-compat VGICP cov_mode %d under reordering: pose rel %s" % (cov_mode, ["%.1e" % v for v in d]))
        assert 0 < max(d) < bound, d
    f0 = O.approx_voxelgrid(workloads.lidar_frame(2), 0.25)
    f1 = O.approx_voxelgrid(workloads.lidar_frame(3), 0.25)
    for mode in (O.D2D, O.P2D):
        def run(t, s):
            g = O.CudaCompatNDT(mode=mode, search=O.DIRECT7)
            g.set_target(t); g.set_source(s)
            return g.align()
        base = run(f0, f1)
        d = [util.rel_err(run(f0[rng.permutation(len(f0))], f1[rng.permutation(len(f1))])["T"], base["T"]) for _ in range(2)]
        print("cuda-compat NDT mode %d under reordering: pose rel %s" % (mode, ["%.1e" % v for v in d]))
        assert 0 < max(d) < 3e-4, d
