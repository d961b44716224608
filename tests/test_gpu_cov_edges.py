"""GPU tests: the third numerical core at its edges -- the eigen solver and the regulariser under every covariance (dev_math.hpp: sym_eig3,
regularize_cov) ALONE and in fp64 through fvh_debug_regularize (part a), the three k-NN covariance kernels against exact rational covariances
on caller-given neighbour lists (part b), and the NDT voxel records of degenerate voxels (part c). References: tests/coveig_ref.py.

The fp32 output of the kernels hides any fp64 error below 1e-7, so part a holds the solver to K eps with K = 4 x what the same algorithm in IEEE
arithmetic shows on the same matrices (coveig_ref.K, pinned by tests/test_coveig_ref_cpu.py). MIN_EIG and NORMALIZED_MIN_EIG are matrix functions,
well defined at eigenvalue ties and Lipschitz in C: in part b EVERY point, ties included, is held to the plain fp32-storage bound 2e-7. Only PLANE
depends on an eigenvector; it gets the gap-aware bound of util.cov_error_bound(gaps="01") and, where the two smallest eigenvalues tie by
construction, the properties that survive the tie. FROBENIUS is A |A^-1|_F with A = C + 1e-3 I: NOT Lipschitz -- a relative change of C comes
back times |C|max / mu_min(A) (coveig_ref.frobenius_condition), which its flat bound is multiplied by: 1 + something small for every well-conditioned
matrix, 1e9 for collinear neighbours spread over 1e3. (Two cofactor inversions, the reference's way, lose that factor squared: 0.2 of the result
on the line and plane clouds at scale 1e3 here, which is why regularize_cov forms FROBENIUS from the eigenvalues.)"""
import numpy as np
import pytest

from tests import coveig_ref as R
from tests import util

pytestmark = pytest.mark.gpu

EPS, K = R.EPS, R.K


def _capi():
    from fast_gicp_amd import capi
    return capi


# ---------------------------------------------------------------------------------------------
# a. the solver against numpy, through the hook
# ---------------------------------------------------------------------------------------------
_SOLVED = {}


def _solve(family, method):
    key = (family, method)
    if key not in _SOLVED:
        _SOLVED[key] = _capi().debug_regularize(R.MATRICES[family], method)
    return _SOLVED[key]


@pytest.mark.parametrize("family", list(R.MATRICES))
def test_solver_meets_the_bound_of_its_ieee_twin(family):
    S = R.MATRICES[family]
    w, V, reg = _solve(family, R.NONE)
    r = R.eig_residuals(S, w, V)
    print("device %-24s reconstruction %6.2f orthogonality %6.2f eigenvalues %6.2f   (K = %.1f)" % (family, r["reconstruction"].max(), r["orthogonality"].max(), r["eigenvalues"].max(), K))
    assert r["finite"].all() and r["ascending"].all()
    for what in ("reconstruction", "orthogonality", "eigenvalues"):
        assert np.all(r[what] <= K), (what, float(r[what].max()), int(np.argmax(r[what])))
    assert np.array_equal(reg, S)  # NONE is the identity
    for m in R.METHODS[1:]:  # the decomposition does not depend on the method asked for
        w2, V2, _ = _solve(family, m)
        assert np.array_equal(w2, w) and np.array_equal(V2, V)


@pytest.mark.parametrize("method", [R.MIN_EIG, R.NORMALIZED_MIN_EIG, R.FROBENIUS], ids=["MIN_EIG", "NORMALIZED_MIN_EIG", "FROBENIUS"])
def test_regularisations_match_the_matrix_functions(method):
    worst = {}
    for family, S in R.MATRICES.items():
        _, _, reg = _solve(family, method)
        ref = R.reg_reference(S, method)
        assert np.isfinite(reg).all(), family
        assert np.array_equal(reg, reg.transpose(0, 2, 1)), family
        scale = np.abs(ref).max(axis=(1, 2))
        bound = K * EPS * scale
        told = np.ones(len(S), bool)
        if method == R.FROBENIUS:
            amp = K * EPS * R.frobenius_condition(S)
            bound, told = amp * scale, amp < 0.5  # (beyond: the smallest eigenvalue of C + 1e-3 I is below the rounding of C -- only finite and symmetric)
        err = np.abs(reg - ref).max(axis=(1, 2))
        worst[family] = float((err[told] / bound[told]).max())
        print("device %-20s %-24s worst error / bound %.3f (error %.2f eps |ref|)" % (R.METHOD_NAMES[method], family, worst[family], float((err / (EPS * scale)).max())))
    bad = {f: v for f, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_plane_follows_the_gap_and_survives_ties():
    n_tied = 0
    for family, S in R.MATRICES.items():
        _, _, reg = _solve(family, R.PLANE)
        ref = R.reg_reference(S, R.PLANE)
        assert np.isfinite(reg).all(), family
        err, bound, degenerate = util.cov_error_bound(reg, ref, S, input_rel=K * EPS, gaps="01", storage_rel=K * EPS)
        e2, b2, d2 = R.plane_error_bound(reg, ref, S, K * EPS, K * EPS)  # (the restatement part b uses is the same function)
        assert np.array_equal(err, e2) and np.array_equal(bound, b2) and np.array_equal(degenerate, d2)
        ok = ~degenerate
        print("device PLANE %-24s %4d tied, worst error / bound elsewhere %.3f" % (family, int(degenerate.sum()), float((err[ok] / bound[ok]).max()) if ok.any() else 0.0))
        assert np.all(err[ok] <= bound[ok]), (family, float((err[ok] / bound[ok]).max()))
        if degenerate.any():
            n_tied += int(degenerate.sum())
            assert not R.plane_tie_violations(reg[degenerate], S[degenerate], K * EPS).any(), family
    assert n_tied >= 3 * R.PER_FAMILY  # exact ties, near ties, s I, the zero matrix, rank 1


def test_zero_matrix_under_every_method():
    Z = np.zeros((3, 6))
    I3 = np.eye(3)
    for m, want in ((R.NONE, 0.0 * I3), (R.MIN_EIG, 1e-3 * I3), (R.NORMALIZED_MIN_EIG, 1e-3 * I3)):
        w, V, reg = _capi().debug_regularize(Z, m)
        assert np.array_equal(w, np.zeros((3, 3))) and np.array_equal(V, np.tile(I3, (3, 1, 1)))
        assert np.isfinite(reg).all() and np.array_equal(reg, np.tile(want, (3, 1, 1))), R.METHOD_NAMES[m]
    reg = _capi().debug_regularize(Z, R.FROBENIUS)[2]
    assert np.abs(reg - np.sqrt(3.0) * I3).max() <= K * EPS * np.sqrt(3.0)
    reg = _capi().debug_regularize(Z, R.PLANE)[2]
    assert not R.plane_tie_violations(reg, np.zeros((3, 3, 3)), K * EPS).any()


# ---------------------------------------------------------------------------------------------
# b. the three covariance kernels against exact covariances
# ---------------------------------------------------------------------------------------------
_COVS = {}


def _kernel_covs(cloud):
    """{method: (n, 3, 3) fp32 covariances} of a CLOUDS entry, lists through set_*_neighbors; source and target side take turns"""
    name = cloud["name"]
    if name not in _COVS:
        capi = _capi()
        c = capi.VGICPCore(0)
        side = "source" if R.CLOUDS.index(cloud) % 2 == 0 else "target"
        getattr(c, "set_%s_cloud" % side)(cloud["pts"])
        getattr(c, "set_%s_neighbors" % side)(cloud["k"], cloud["idx"])
        out = {}
        for m in R.METHODS:
            getattr(c, "calculate_%s_covariances" % side)(m)
            out[m] = c.get_covariances(side)
        c.close()
        _COVS[name] = out
    return _COVS[name]


@pytest.mark.parametrize("method", R.METHODS, ids=R.METHOD_NAMES)
def test_knn_covariances_match_exact_covariances_on_every_point(method):
    """k in {1 .. 64} x n in {1 .. 2000} on a blob, and every shape (blob, line, tilted and axis-aligned plane, lattice, coincident neighbours,
    lists repeating an index) at scales 1e-3 / 1 / 1e3 and offsets 0 / 50 / 1e4: no point is excused."""
    failed, worst = [], 0.0
    for cloud in R.CLOUDS:
        got = _kernel_covs(cloud)[method]
        assert got.shape == (cloud["n"], 3, 3)
        bad, rel = R.cloud_violations(cloud, method, got)
        worst = max(worst, rel)
        if bad.any():
            failed.append((cloud["name"], int(bad.sum()), rel))
    print("device %-20s worst error / bound over %d clouds: %.3f" % (R.METHOD_NAMES[method], len(R.CLOUDS), worst))
    assert not failed, failed


def test_more_than_64_neighbours_are_refused():
    capi = _capi()
    c = capi.VGICPCore(0)
    pts = R.CLOUDS[-1]["pts"]
    c.set_source_cloud(pts)
    c.set_source_neighbors(65, R._window_lists(len(pts), 65, np.random.default_rng(1)))
    with pytest.raises(capi.FvhError, match="status 4"):  # FVH_ERR_UNSUPPORTED
        c.calculate_source_covariances(capi.REG_MIN_EIG)
    c.close()


@pytest.mark.parametrize("k", [3, 20, 32, 33])
def test_knn_covariances_in_morton_order(k):
    """With the Morton order present and coherent_min_points lowered the kernels walk the order (`subset`) and leave a second copy along the
    curve (`cov_sorted`), which the VGICP cost reads: the covariances must be the same, and so must the sums of a linearisation."""
    capi = _capi()
    rng = np.random.default_rng(k)
    pts = (rng.normal(size=(1000, 3)) * 3.0 + 20.0).astype(np.float32)
    idx = R._window_lists(1000, k, rng)
    ref = R.reg_reference(R.exact_cov(pts, idx), R.MIN_EIG)
    sums = []
    for coherent in (True, False):
        c = capi.VGICPCore(0)
        c.set_engine_params(coherent_min_points=1 if coherent else 1 << 30)
        c.set_neighbor_search_method(capi.DIRECT7)
        c.set_target_cloud(pts); c.set_target_covariances(np.tile(np.eye(3), (len(pts), 1, 1))); c.create_target_voxelmap()
        c.set_source_cloud(pts)
        c.find_source_neighbors(max(k, 5))  # sorts the cloud
        if coherent:
            order, _ = c.debug_spatial_order("source")
            assert sorted(order) == list(range(1000)) and not np.array_equal(order, np.arange(1000))
        c.set_source_neighbors(k, idx)
        c.calculate_source_covariances(capi.REG_MIN_EIG)
        got = c.get_covariances("source").astype(np.float64)
        assert np.all(np.abs(got - ref).max(axis=(1, 2)) <= R.STORAGE_REL * np.abs(ref).max(axis=(1, 2)))
        T = util.random_pose(np.random.default_rng(3), 0.02, 0.05)
        sums.append(c.linearize(T))
        c.close()
    (e0, H0, b0), (e1, H1, b1) = sums
    assert e0 > 0 and util.sums_close(e0, H0, b0, e1, H1, b1, 1e-10)


# ---------------------------------------------------------------------------------------------
# c. NDT voxel records of degenerate voxels
# ---------------------------------------------------------------------------------------------
def _ndt_voxels(shift):
    """{voxel coordinate: member points} at resolution 1 (voxel c holds [c + 0.5, c + 1.5)): every coordinate has few mantissa bits, so the
    device's uncentred fp64 sums of a one-point or coincident voxel are exact (300 p p^T needs 9 bits more than p p^T)"""
    s = np.float32(shift)
    v = {}
    v["one"] = np.array([[1.0, 1.25, 0.75]])
    v["two"] = np.array([[4.0, 0.75, 1.0], [4.25, 1.0, 1.25]])
    v["collinear"] = np.array([[7.0, 0.75, 0.75], [7.125, 1.0, 0.875], [7.25, 1.25, 1.0]])
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 2) * 0.125 + 0.75
    v["axis_plane"] = np.concatenate([9.0 + g[:, :1], g[:, 1:], np.full((len(g), 1), 1.0)], axis=1)
    v["copies300"] = np.tile(np.array([[13.3125, 0.8125, 1.1875]]), (300, 1))
    return {k_: (p + shift).astype(np.float32) for k_, p in v.items()}


def test_ndt_records_of_degenerate_voxels():
    capi = _capi()
    groups = {}
    for shift in (0.0, 1e4):
        for name, p in _ndt_voxels(shift).items():
            groups["%s@%g" % (name, shift)] = p
    # the 300 copies first: they fill one workgroup of the accumulation (256 points) and spill into the next -> owner and visitor sums
    names = sorted(groups, key=lambda n: (not n.startswith("copies300"), n))
    cloud = np.concatenate([groups[n] for n in names]).astype(np.float32)
    c = capi.NDTCore(0)
    c.set_resolution(1.0)
    c.set_target_cloud(cloud)
    c.create_target_voxelmap()
    coords, num, means, covs = c.get_voxelmap("target")
    c.close()
    got = util.voxel_dict(coords, num, means, covs)
    assert len(got) == len(groups) and int(num.sum()) == len(cloud)
    tiny = np.float32(1e-3) * np.eye(3, dtype=np.float32)
    for name, p in groups.items():
        key = tuple(np.floor(p[0].astype(np.float64) - 0.5).astype(int))
        assert np.all(np.floor(p.astype(np.float64) - 0.5).astype(int) == np.array(key)), name
        n_, mean_, cov_ = got[key]
        assert n_ == len(p), name
        mref, craw = R.exact_mean_cov(p, np.arange(len(p))[None, :])
        ref = R.reg_reference(craw, R.MIN_EIG)[0]
        assert np.all(np.abs(mean_.astype(np.float64) - mref[0]) <= 2.0 ** -24 * (1 + 2.0 ** -20) * np.abs(mref[0])), name  # one fp32 rounding (of an fp64 mean)
        # the device forms sum p p^T - mean sum p from UNCENTRED fp64 sums: the cancellation costs 8 eps |p|^2 at most
        bound = R.STORAGE_REL * np.abs(ref).max() + 8 * EPS * (p.astype(np.float64) ** 2).sum(axis=1).max()
        err = np.abs(cov_.astype(np.float64) - ref).max()
        print("device NDT %-22s error %.3e bound %.3e" % (name, err, bound))
        assert np.isfinite(cov_).all() and err <= bound, (name, err, bound)
        if name.startswith(("one@", "copies300@")):
            assert np.array_equal(cov_, tiny), name
