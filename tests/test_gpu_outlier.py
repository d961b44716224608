"""Range crop, statistical and radius outlier removal on the voxel-grid handle (fvh_voxelgrid_crop_range, _remove_statistical_outliers,
_remove_radius_outliers) against the numpy twin of their definitions (tests/outlier_ref.py).

Radius and crop are exact by construction: twin and kernel evaluate the same fp32 expression, so kept set, indices, points (compared as
uint32) and scores must be EQUAL. The statistical filter's scores may differ in the last bit (order of the fp64 sum before the cast),
so scores are held to a relative 1e-6 and the threshold to 1e-12, and the kept set must be equal on inputs whose scores all stay a
relative 1e-5 away from the threshold -- asserted on the twin first (tests/test_outlier_cpu.py proves the same without a GPU).
No cloud is larger than 4,099 points: the brute-force twin costs 0.5 s there."""
import functools
import os

import numpy as np
import pytest

from tests import outlier_ref as R
from tests import util

pytestmark = pytest.mark.gpu

RADIUS_PARAMS = [(0.3, 5), (0.5, 2), (0.8, 2)]
RADIUS_PARAMS_SPARSE = [(4.0, 2), (8.0, 10)]  # in addition, on the random clouds: the three above keep next to nothing of a +-20 m uniform cloud


@functools.lru_cache(maxsize=None)
def cloud(name):
    from fast_gicp_amd import preprocess
    if name == "A":
        return np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099])
    if name == "U":
        return R.cloud_u()
    if name == "lattice":
        return R.cloud_lattice()
    if name == "dup":
        return R.cloud_duplicates()
    assert name.startswith("ragged")
    return R.cloud_ragged(int(name[6:]))


@functools.lru_cache(maxsize=None)
def nearest(name):
    return R.nearest_sq(cloud(name), 64)


RAGGED = ["ragged%d" % n for n in R.RAGGED_SIZES]
ALL_CLOUDS = ["A", "U"] + RAGGED + ["lattice", "dup"]


@pytest.fixture(scope="module")
def vg():
    from fast_gicp_amd import capi
    v = capi.VoxelGrid(0)
    yield v
    v.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_exact(vg, out, tw, n_in):
    idx = vg.kept_indices()
    scores, threshold = vg.scores()
    assert out.shape == (len(tw["idx"]), 3) and out.dtype == np.float32
    assert idx.dtype == np.int32 and np.array_equal(idx, tw["idx"])
    assert same_bits(out, tw["points"])
    assert scores.shape == (n_in,) and same_bits(scores, tw["scores"])
    assert threshold == tw["threshold"]


# ---- radius ----
@pytest.mark.parametrize("name", ALL_CLOUDS)
def test_radius_filter_equals_the_twin(vg, name):
    p = cloud(name)
    for r, m in RADIUS_PARAMS + (RADIUS_PARAMS_SPARSE if name not in ("A", "lattice") else []):
        check_exact(vg, vg.remove_radius_outliers(p, r, m), R.radius(p, r, m), len(p))


def test_radius_filter_edges(vg):
    lat = cloud("lattice")
    for r, m in ((0.5, 6), (0.5, 7), (0.5, 3), (0.25, 1)):  # r = the spacing: the six axis neighbours sit at d2 == r2 exactly (0.5 and 0.25 are exact in fp32)
        tw = R.radius(lat, r, m)
        check_exact(vg, vg.remove_radius_outliers(lat, r, m), tw, len(lat))
    assert R.radius(lat, 0.5, 6)["keep"].sum() == 7 ** 3 and R.radius(lat, 0.5, 7)["keep"].sum() == 0
    u = cloud("U")
    out = vg.remove_radius_outliers(u, 0.8, 10 ** 6)  # more neighbours than the cloud has points: nothing kept, no query leaves early
    assert out.shape == (0, 3) and len(vg.kept_indices()) == 0
    s, t = vg.scores()
    assert same_bits(s, R.radius(u, 0.8, 10 ** 6)["scores"]) and t == 10 ** 6
    d = cloud("dup")
    tw = R.radius(d, 1e-3, 1)  # duplicates are each other's neighbours at distance 0; a point is not its own
    assert tw["keep"].sum() >= 100
    check_exact(vg, vg.remove_radius_outliers(d, 1e-3, 1), tw, len(d))
    check_exact(vg, vg.remove_radius_outliers(u, 1e30, 1), R.radius(u, 1e30, 1), len(u))  # r * r overflows fp32: clamped, everything kept
    assert len(vg.kept_indices()) == len(u)


# ---- statistical ----
def check_statistical(vg, p, k, mul, near):
    tw = R.statistical(p, k, mul, near)
    assert tw["margin"] >= R.SOR_MIN_MARGIN, tw["margin"]  # precondition: no score within 1e-5 (relative) of the threshold
    out = vg.remove_statistical_outliers(p, k, mul)
    idx = vg.kept_indices()
    scores, t = vg.scores()
    print("n=%d k=%d mul=%.1f: kept %d, max score rel err %.2e, threshold rel err %.2e, margin %.2e" % (
        len(p), k, mul, len(idx), np.max(np.abs(scores - tw["scores"]) / tw["scores"]), abs(t - tw["threshold"]) / tw["threshold"], tw["margin"]))
    assert np.all(np.abs(scores.astype(np.float64) - tw["scores"]) <= 1e-6 * tw["scores"])
    assert abs(t - tw["threshold"]) <= 1e-12 * tw["threshold"]
    assert np.array_equal(idx, tw["idx"]) and same_bits(out, tw["points"])
    return tw, t


@pytest.mark.parametrize("name,k,mul,kept", R.SOR_TABLE)
def test_statistical_filter_equals_the_twin(vg, name, k, mul, kept):
    tw, _ = check_statistical(vg, cloud(name), k, mul, nearest(name))
    assert int(tw["keep"].sum()) == kept


@pytest.mark.parametrize("name", RAGGED)
def test_statistical_filter_on_ragged_sizes(vg, name):
    p = cloud(name)
    mul = R.ragged_stddev_mul(p, R.RAGGED_MEAN_K, nearest(name))
    assert mul is not None
    check_statistical(vg, p, R.RAGGED_MEAN_K, mul, nearest(name))


def test_statistical_filter_on_a_lattice(vg):
    """every interior score is equal: the variance is a difference of nearly equal sums and must not go negative"""
    p = cloud("lattice")
    tw, t = check_statistical(vg, p, 8, 1.0, nearest("lattice"))
    scores, _ = vg.scores()
    assert np.isfinite(t) and np.all(np.isfinite(scores)) and t >= scores.astype(np.float64).mean() and tw["var"] >= 0
    q = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], np.float32)  # identical scores: var clamps at 0, everything is kept
    out = vg.remove_statistical_outliers(q, 3, 1.0)
    s, t = vg.scores()
    assert same_bits(out, q) and np.isfinite(t) and np.all(s.astype(np.float64) <= t)


# ---- crop ----
def test_crop_equals_the_twin_and_the_host_origin_filter(vg):
    from fast_gicp_amd import preprocess
    for f in ("251370668.pcd", "251371071.pcd"):
        raw = preprocess.load_pcd(os.path.join(util.DATA, f))
        out = vg.crop_range(raw, 1e-3, np.inf)
        check_exact(vg, out, R.crop(raw, 1e-3, np.inf), len(raw))
        assert same_bits(out, preprocess.remove_origin_points(raw))
        far = vg.crop_range(raw, 1e-3, 400.0)  # a finite upper bound cuts the far points too
        check_exact(vg, far, R.crop(raw, 1e-3, 400.0), len(raw))
        assert 0 < len(far) < len(out)
    rng = np.random.default_rng(5)
    p = rng.uniform(-30, 30, (3001, 3)).astype(np.float32)
    p[rng.choice(3001, 200, replace=False)] *= np.float32(1e-3)  # some points near the origin
    for v in (np.nan, np.inf, -np.inf):
        rows = rng.choice(3001, 40, replace=False)
        p[rows, rng.integers(0, 3, 40)] = v
    tw = R.crop(p, 1e-3, np.inf)
    out = vg.crop_range(p)
    assert same_bits(out, tw["points"]) and np.array_equal(vg.kept_indices(), tw["idx"]) and np.all(np.isfinite(out))
    s, _ = vg.scores()
    ok = np.isfinite(tw["scores"])
    assert same_bits(s[ok], tw["scores"][ok]) and np.array_equal(s, tw["scores"], equal_nan=True)  # (a NaN's payload is not part of the contract)
    fin = p[np.isfinite(p).all(axis=1)]
    assert same_bits(out, preprocess.remove_origin_points(fin))
    # its output is valid input for the other filters
    assert len(vg.remove_radius_outliers(out, 3.0, 1)) > 0


# ---- plumbing ----
def test_host_strided_and_device_routes_agree(vg):
    import torch
    p = cloud("U")
    p4 = np.ascontiguousarray(np.hstack([p, np.full((len(p), 1), 7.0, np.float32)]))
    dev = torch.device("cuda", 0)
    d3, d4 = torch.from_numpy(p).to(dev).contiguous(), torch.from_numpy(p4).to(dev).contiguous()
    calls = [("crop_range", (4.0, 150.0)), ("remove_statistical_outliers", (20, 1.0)), ("remove_radius_outliers", (0.8, 2))]
    for name, args in calls:
        host = getattr(vg, name)(p, *args)
        ref = (host.copy(), vg.kept_indices(), vg.scores())
        assert 0 < len(host) < len(p)

        def same():
            s, t = vg.scores()
            return np.array_equal(vg.kept_indices(), ref[1]) and same_bits(s, ref[2][0]) and t == ref[2][1]

        assert same_bits(getattr(vg, name)(p4, *args, stride=4), ref[0]) and same()
        ptr, m = getattr(vg, name + "_device")(d3.data_ptr(), len(p), *args)
        assert m == len(host) and ptr and same_bits(vg.get_points(m), ref[0]) and same()
        ptr, m = getattr(vg, name + "_device")(d4.data_ptr(), len(p), *args, stride=4)
        assert m == len(host) and same_bits(vg.get_points(m), ref[0]) and same()
        # two consecutive runs: identical bytes, threshold included
        again = getattr(vg, name)(p, *args)
        assert same_bits(again, ref[0]) and same()


def test_stages_chain_on_one_handle_into_an_ndt_handle():
    """ApproximateVoxelGrid, then radius outlier removal fed with the handle's own device_points() pointer, then the result taken by an NDT
    handle without a copy: the NDT source equals the host-computed chain point for point and aligns like the same cloud uploaded from the host."""
    import torch
    from fast_gicp_amd import capi, preprocess
    raw_t, raw_s = [preprocess.remove_origin_points(preprocess.load_pcd(os.path.join(util.DATA, f))) for f in ("251370668.pcd", "251371071.pcd")]
    leaf, r, m_nb = 0.6, 1.0, 2
    tgt = preprocess.approximate_voxel_grid(raw_t, leaf)
    down = preprocess.approximate_voxel_grid(raw_s, leaf)
    assert len(down) <= 4099
    want = R.radius(down, r, m_nb)
    assert 0 < len(want["idx"]) < len(down)
    d_raw = torch.from_numpy(raw_s).to(torch.device("cuda", 0)).contiguous()
    vg = capi.VoxelGrid(0)
    ptr, m = vg.filter_device(d_raw.data_ptr(), len(raw_s), leaf)
    assert m == len(down) and same_bits(vg.get_points(m), down)
    own_ptr, own_n = vg.device_points()
    assert (own_ptr, own_n) == (ptr, m)
    ptr2, m2 = vg.remove_radius_outliers_device(own_ptr, own_n, r, m_nb)  # input and output are the same buffer of the handle
    assert m2 == len(want["idx"]) and same_bits(vg.get_points(m2), want["points"]) and np.array_equal(vg.kept_indices(), want["idx"])

    def make():
        c = capi.NDTMapCore(0)
        c.set_distance_mode(1); c.set_neighbor_search_method(1); c.set_resolution(1.0)
        c.set_target_cloud(tgt)
        return c

    c, c_host = make(), make()
    c.set_source_cloud_from_voxelgrid(vg)
    with pytest.raises(capi.FvhError):
        c.set_source_cloud_from_voxelgrid(vg)  # an output can be taken once
    c_host.set_source_cloud(want["points"])
    ra, rb = c.align(), c_host.align()
    assert ra["converged"] and (ra["num_linearize"], ra["num_error_evals"]) == (rb["num_linearize"], rb["num_error_evals"])
    assert util.rel_err(ra["T"], rb["T"]) < 1e-9
    c.swap_source_and_target()
    assert same_bits(c.get_target_points(), want["points"])
    assert same_bits(vg.get_points(m2), want["points"])  # the packed output is still there
    vg.close(); c.close(); c_host.close()


def test_getters_need_an_outlier_call_and_arguments_are_checked(vg):
    import ctypes as C
    from fast_gicp_amd import capi
    u = cloud("U")
    vg.remove_radius_outliers(u, 0.8, 2)
    assert len(vg.kept_indices()) > 0
    vg.filter(u, 0.5)  # a plain voxel filter: the side outputs are gone
    for getter in (vg.kept_indices, vg.scores):
        with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
            getter()
    bad = u.copy()
    bad[17, 1] = np.nan
    p5 = np.zeros((100, 5), np.float32)
    errors = [lambda: vg.remove_statistical_outliers(u, 0, 1.0), lambda: vg.remove_statistical_outliers(u, 64, 1.0), lambda: vg.remove_statistical_outliers(u[:20], 20, 1.0),
              lambda: vg.remove_statistical_outliers(u[:8], 8, 1.0), lambda: vg.remove_statistical_outliers(u, 8, np.inf), lambda: vg.remove_radius_outliers(u, 0.0, 2),
              lambda: vg.remove_radius_outliers(u, -1.0, 2), lambda: vg.remove_radius_outliers(u, np.nan, 2), lambda: vg.remove_radius_outliers(u, 0.8, 0),
              lambda: vg.remove_radius_outliers(p5, 0.8, 2, stride=5), lambda: vg.crop_range(p5, stride=5), lambda: vg.remove_statistical_outliers(p5, 8, 1.0, stride=5),
              lambda: vg.remove_radius_outliers(bad, 0.8, 2), lambda: vg.remove_statistical_outliers(bad, 8, 1.0)]
    for i, call in enumerate(errors):
        with pytest.raises(capi.FvhError, match="code 1"):  # FVH_ERR_INVALID_ARGUMENT
            call()
        ptr, m = vg.device_points()
        assert m == 0, i  # a refused call leaves no output
        with pytest.raises(capi.FvhError, match="code 2"):
            vg.kept_indices()
    lib = capi.load()
    a = np.ascontiguousarray(u)
    assert lib.fvh_voxelgrid_remove_radius_outliers(vg._h, capi._p(a), len(a), 0.8, 2, None) == 1  # null out_n
    assert lib.fvh_voxelgrid_crop_range(vg._h, capi._p(a), len(a), 1e-3, 1e6, None) == 1
    assert lib.fvh_voxelgrid_remove_statistical_outliers(vg._h, capi._p(a), len(a), 8, 1.0, None) == 1
    n = C.c_int(5)
    assert lib.fvh_voxelgrid_remove_radius_outliers(vg._h, None, 10, 0.8, 2, C.byref(n)) == 1 and n.value == 0  # null points
    # n == 0: an empty result, not an error; the getters answer (with nothing)
    empty = np.zeros((0, 3), np.float32)
    for out in (vg.crop_range(empty), vg.remove_radius_outliers(empty, 0.8, 2), vg.remove_statistical_outliers(empty, 8, 1.0)):
        assert out.shape == (0, 3)
        assert len(vg.kept_indices()) == 0 and len(vg.scores()[0]) == 0
    # the handle still works
    check_exact(vg, vg.remove_radius_outliers(u, 0.8, 2), R.radius(u, 0.8, 2), len(u))


def test_profile_classes(vg):
    u = cloud("U")
    vg.profile_enable(True); vg.profile_reset()
    vg.remove_radius_outliers(u, 0.8, 2)
    vg.remove_statistical_outliers(u, 20, 1.0)
    got = {c: vg.profile_get(c) for c in ("sort", "knn", "outlier_count", "outlier_score", "compact", "downsample")}
    vg.profile_enable(False); vg.profile_reset()
    assert got["outlier_count"][1] == 1 and got["outlier_score"][1] == 1 and got["knn"][1] == 1 and got["sort"][1] == 2 and got["compact"][1] == 3, got
    assert got["downsample"] == (0.0, 0) and all(ms > 0 for c, (ms, k) in got.items() if c != "downsample"), got


def test_pygicp_bindings_equal_the_capi_route(vg):
    import torch  # noqa: F401  (its HIP runtime first, see tests/conftest.py)
    import pygicp
    u = cloud("U")
    for kw, ref in ((dict(method="STATISTICAL", mean_k=20, stddev_mul=1.0), lambda: vg.remove_statistical_outliers(u, 20, 1.0)),
                    (dict(method="RADIUS", radius=0.8, min_neighbors=2), lambda: vg.remove_radius_outliers(u, 0.8, 2))):
        want = ref()
        want_idx = vg.kept_indices()
        got = pygicp.remove_outliers_device(u, **kw)
        assert got.dtype == np.float64 and same_bits(got.astype(np.float32), want)
        got, idx = pygicp.remove_outliers_device(u, return_indices=True, **kw)
        assert same_bits(got.astype(np.float32), want) and np.array_equal(idx, want_idx)
    p = np.vstack([u, np.zeros((3, 3), np.float32)])
    assert same_bits(pygicp.crop_range_device(p).astype(np.float32), vg.crop_range(p))
    got, idx = pygicp.crop_range_device(p, min_sq_norm=4.0, max_sq_norm=150.0, return_indices=True)
    assert same_bits(got.astype(np.float32), vg.crop_range(p, 4.0, 150.0)) and np.array_equal(idx, vg.kept_indices())
    with pytest.raises(Exception):
        pygicp.remove_outliers_device(u, method="NONE")
