"""The reference of tests/test_gpu_cov_edges.py (tests/coveig_ref.py) checked without a GPU: the exact covariance against an independent
fp64 computation and the oracle, the IEEE twin of the device's Jacobi against the solver bound at K / 4 -- which is what makes K a bound the
reference alone stays within -- the binding of fvh_debug_regularize, and that the checks of part b see ONE planted error on every cloud."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import coveig_ref as R


def test_exact_cov_agrees_with_fp64_and_with_the_oracle():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(300, 3)).astype(np.float32) * 2.0 + np.float32(3.0)
    idx = R._window_lists(300, 20, rng)
    idx[:, 3] = idx[:, 2]  # a repeated index counts twice
    mean, cov = R.exact_mean_cov(pts, idx)
    p = pts.astype(np.float64)[idx]
    m = p.mean(axis=1)
    d = p - m[:, None, :]
    c64 = np.einsum("nka,nkb->nab", d, d) / 20.0
    assert np.abs(mean - m).max() <= 4 * R.EPS * np.abs(m).max()
    assert np.all(np.abs(cov - c64).max(axis=(1, 2)) <= 64 * R.EPS * np.abs(cov).max(axis=(1, 2)))  # (20 centred terms, well conditioned)
    co = O.covariances_knn(pts, 20, O.NONE, idx=idx)
    assert np.all(np.abs(cov - co).max(axis=(1, 2)) <= 64 * R.EPS * np.abs(cov).max(axis=(1, 2)))
    # exactness where fp64 cannot follow: three points 1e4 out, 2^-10 apart -- every entry of the covariance is a small dyadic rational
    q = (np.float32(1e4) + np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32) * np.float32(2.0 ** -10))
    c = R.exact_cov(q, np.array([[0, 1, 2]]))[0] * 2.0 ** 20
    assert np.array_equal(c, np.array([[2, -2, 0], [-2, 8, 0], [0, 0, 0]]) / 9.0)
    assert np.array_equal(R.exact_cov(pts, np.full((1, 7), 11)), np.zeros((1, 3, 3)))


def test_reg_reference_on_matrices_with_known_answers():
    Z = np.zeros((1, 3, 3))
    assert np.array_equal(R.reg_reference(Z, R.NONE), Z)
    assert np.allclose(R.reg_reference(Z, R.MIN_EIG), 1e-3 * np.eye(3), rtol=0, atol=1e-18)
    got = R.reg_reference(Z, R.NORMALIZED_MIN_EIG)
    assert np.isfinite(got).all() and np.allclose(got, 1e-3 * np.eye(3), rtol=0, atol=1e-18)
    assert np.allclose(R.reg_reference(Z, R.FROBENIUS), np.sqrt(3.0) * np.eye(3), rtol=1e-15)
    D = np.diag([4.0, 1e-5, 2.0])[None]
    assert np.allclose(R.reg_reference(D, R.MIN_EIG), np.diag([4.0, 1e-3, 2.0]), rtol=1e-15, atol=1e-18)
    assert np.allclose(R.reg_reference(D, R.NORMALIZED_MIN_EIG), np.diag([1.0, 1e-3, 0.5]), rtol=1e-15, atol=1e-18)
    assert np.allclose(R.reg_reference(D, R.PLANE), np.diag([1.0, 1e-3, 1.0]), rtol=1e-15, atol=1e-18)
    mu = np.array([4.001, 1.01e-3, 2.001])
    assert np.allclose(R.reg_reference(D, R.FROBENIUS), np.diag(mu * np.sqrt((1 / mu ** 2).sum())), rtol=1e-12)


def test_twin_meets_the_solver_bound_at_a_quarter_of_K_on_the_whole_list():
    """K = 4 x the twin's worst: recomputed here, pinned to the constant the GPU test uses."""
    worst, sweeps, stats = 0.0, 0, {}
    for name, S in R.MATRICES.items():
        assert S.shape == (R.PER_FAMILY, 3, 3) and np.array_equal(S, S.transpose(0, 2, 1)) and np.isfinite(S).all(), name
        s = np.abs(S).max(axis=(1, 2))
        assert np.all((s == 0) | ((s >= 1e-100) & (s <= 1e100))), name  # the solver's stated domain
        st = {}
        w, V, sw = R.jacobi_twin(S, stats=st)
        stats[name] = st
        r = R.eig_residuals(S, w, V)
        assert r["finite"].all() and r["ascending"].all(), name
        fam = max(r[k].max() for k in ("reconstruction", "orthogonality", "eigenvalues"))
        print("%-24s reconstruction %5.2f orthogonality %5.2f eigenvalues %5.2f sweeps %d" % (name, r["reconstruction"].max(), r["orthogonality"].max(), r["eigenvalues"].max(), sw.max()))
        assert fam <= R.K / 4, (name, fam)
        worst, sweeps = max(worst, fam), max(sweeps, int(sw.max()))
    print("worst %.3f (K_TWIN_MEASURED %.3f, K %.1f), sweeps %d" % (worst, R.K_TWIN_MEASURED, R.K, sweeps))
    assert R.K == 4 * R.K_TWIN_MEASURED
    assert 0.85 * R.K_TWIN_MEASURED <= worst <= R.K_TWIN_MEASURED, worst  # (LAPACK's last bits may move it a little from machine to machine)
    assert sweeps <= 4
    # the two families written for a branch reach it, and nothing else does
    assert stats["huge_theta"]["huge_theta"] >= R.PER_FAMILY and stats["skipped_rotation"]["skipped"] >= R.PER_FAMILY
    assert all(st.get("huge_theta", 0) == 0 for n, st in stats.items() if n not in ("huge_theta", "axis_plane"))
    assert stats["zero_identity_diagonal"] == {} and stats["scaled_identity"] == {}  # no rotation at all


def test_twin_is_the_sweep_capped_algorithm():
    """one sweep is not enough: the bound the GPU test holds the device to tells a solver that stops after one sweep from the real one"""
    S = R.MATRICES["spd"]
    w, V, _ = R.jacobi_twin(S, sweep_cap=1)
    r = R.eig_residuals(S, w, V)
    assert (r["reconstruction"] > R.K).mean() > 0.9


def test_clouds_cover_what_the_issue_lists():
    names = {c["name"] for c in R.CLOUDS}
    assert len(names) == len(R.CLOUDS)
    assert {(c["n"], c["k"]) for c in R.CLOUDS if c["name"].startswith("blob_n")} == {(n, k) for n in R.NS for k in R.KS}
    assert {(c["shape"], c["scale"], c["offset"]) for c in R.CLOUDS if not c["name"].startswith("blob_n")} == {(s, a, o) for s in R.SHAPES for a in R.SCALES for o in R.OFFSETS}
    assert {c["k"] for c in R.CLOUDS if not c["name"].startswith("blob_n")} == set(R.KS)
    for c in R.CLOUDS:
        assert c["pts"].dtype == np.float32 and c["pts"].shape == (c["n"], 3) and c["n"] <= 2000
        assert c["idx"].dtype == np.int32 and c["idx"].shape == (c["n"], c["k"]) and c["idx"].min() >= 0 and c["idx"].max() < c["n"]
    # clouds that are what their name says
    raw, _ = R.cloud_reference(next(c for c in R.CLOUDS if c["shape"] == "coincident"))
    assert np.array_equal(raw, np.zeros_like(raw))
    for shape, rank in (("line", 1), ("tilted_plane", 2), ("axis_plane", 2)):
        c = next(c for c in R.CLOUDS if c["shape"] == shape and c["offset"] == 0.0 and c["k"] >= 4)
        w = np.linalg.eigvalsh(R.cloud_reference(c)[0])
        assert np.all(w[:, 3 - rank] > 1e-3 * w[:, 2]) and np.all(np.abs(w[:, : 3 - rank]) <= 1e-12 * w[:, 2:]), shape
    c = next(c for c in R.CLOUDS if c["shape"] == "axis_plane" and c["offset"] == 0.0 and c["scale"] == 1.0)
    raw = R.cloud_reference(c)[0]
    assert np.array_equal(raw[:, 2, :], np.zeros((c["n"], 3)))  # z constant: the off-diagonal pair is exactly zero
    lat = next(c for c in R.CLOUDS if c["shape"] == "lattice" and c["offset"] == 0.0 and c["scale"] == 1.0)
    assert np.array_equal(lat["pts"] * 4, np.round(lat["pts"] * 4))


@pytest.mark.parametrize("method", R.METHODS, ids=R.METHOD_NAMES)
def test_model_of_the_kernels_passes_every_check(method):
    """fp64 centred sums + the twin + one fp32 rounding stay inside every bound of part b, with room: the bounds are ones a correct
    implementation meets on every cloud (worst NONE / MIN_EIG / NORMALIZED_MIN_EIG error 6e-8 against the 2e-7 they are held to)."""
    worst = 0.0
    for c in R.CLOUDS:
        bad, rel = R.cloud_violations(c, method, R.kernel_model(c["pts"], c["idx"], method))
        assert not bad.any(), (c["name"], int(bad.sum()), rel)
        worst = max(worst, rel)
    print("worst error / bound: %.3f" % worst)
    assert worst <= 0.5


def test_the_checks_see_one_wrong_neighbour_index():
    seen = 0
    for c in R.CLOUDS:
        idx = c["idx"].copy()
        idx[:, 0] = (idx[:, 0] + max(c["n"] // 2, 1)) % c["n"]  # slot 0 of every list names another point
        if c["k"] == 1 or np.array_equal(c["pts"][idx[:, 0]], c["pts"][c["idx"][:, 0]]):
            continue  # (one neighbour has the covariance 0 whoever it is; in a cloud of one point the other index names the same place)
        seen += 1
        bad, rel = R.cloud_violations(c, R.NONE, R.kernel_model(c["pts"], idx, R.NONE))
        assert bad.any(), c["name"]
    assert seen == sum(1 for c in R.CLOUDS if c["k"] > 1 and c["n"] > 1)


@pytest.mark.parametrize("defect", ["drop_centring", "mask_one_more"])
def test_the_checks_see_uncentred_sums_and_a_slot_masked_too_many(defect):
    seen = 0
    for c in R.CLOUDS:
        base = R.kernel_model(c["pts"], c["idx"], R.NONE)
        got = R.kernel_model(c["pts"], c["idx"], R.NONE, **{defect: True})
        if np.array_equal(got, base):
            continue
        seen += 1
        bad, rel = R.cloud_violations(c, R.NONE, got)
        assert bad.any(), c["name"]
    assert seen == sum(1 for c in R.CLOUDS if c["k"] > 1 or defect == "drop_centring")  # (one neighbour masked away: 0 as before)


def test_the_checks_see_planes_floor_on_the_wrong_eigenvalue():
    seen = 0
    for c in R.CLOUDS:
        raw = R.cloud_reference(c)[0]
        w = np.linalg.eigvalsh(raw)
        if not np.any(w[:, 2] - w[:, 0] > 1e-6 * w[:, 2]):
            continue  # (a multiple of the identity at every point -- the zero matrix of coincident neighbours: d[0] and d[2] are not told apart)
        seen += 1
        bad, rel = R.cloud_violations(c, R.PLANE, R.kernel_model(c["pts"], c["idx"], R.PLANE, plane_swapped=True))
        assert bad.any(), c["name"]
    assert seen == sum(1 for c in R.CLOUDS if c["k"] > 1 and c["n"] > 1 and c["shape"] != "coincident")


def test_regularize_binding_matches_the_header_and_refuses_bad_arguments():
    from fast_gicp_amd import build, capi
    hdr = re.sub(r"/\*.*?\*/", "", open(build.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+fvh_debug_regularize\s*\(([^)]*)\)\s*;", hdr)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(capi.REGULARIZE_ARGTYPES) == 7
    for p, t in zip(params, capi.REGULARIZE_ARGTYPES):
        assert t is (C.c_void_p if "*" in p else C.c_int), (p, t)
    assert "fvh_debug_regularize" in capi.declared_symbols()
    assert (capi.REG_NONE, capi.REG_MIN_EIG, capi.REG_NORMALIZED_MIN_EIG, capi.REG_PLANE, capi.REG_FROBENIUS) == R.METHODS
    # the argument checks come before the device is touched: they answer on a machine without one
    fn = capi.load().fvh_debug_regularize
    s = np.ascontiguousarray(np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (4, 1)))
    w, V, r = np.zeros((4, 3)), np.zeros((4, 9)), np.zeros((4, 6))
    ok = (0, 4, capi._p(s), 1, capi._p(w), capi._p(V), capi._p(r))
    for i in (2, 4, 5, 6):
        args = list(ok)
        args[i] = None
        assert fn(*args) == 1, i
    for n in (0, -1):
        args = list(ok)
        args[1] = n
        assert fn(*args) == 1, n
    for method in (-1, 5):
        args = list(ok)
        args[3] = method
        assert fn(*args) == 1, method
    for bad in (np.nan, np.inf, -np.inf):
        sb = s.copy()
        sb[3, 4] = bad
        args = list(ok)
        args[2] = capi._p(sb)
        assert fn(*args) == 1
    with pytest.raises(capi.FvhError):
        capi.debug_regularize(np.zeros((2, 5)), 1)
    with pytest.raises(capi.FvhError):
        capi.debug_regularize(np.full((2, 3, 3), np.nan), 1)
