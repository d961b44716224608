"""RANSAC plane segmentation on the voxel-grid handle (fvh_voxelgrid_segment_plane) against the numpy twin of its contract
(tests/plane_ref.py). Twin and kernel evaluate the same division-free fp64 tests, so every one of the H counts, the winner, the sample,
info, the kept indices and the kept points (compared as uint32) must be EQUAL; the unrefined coefficients are within 4 fp64 ulp (one host
square root, three divisions), the scores within 1 float32 ulp (the device's fp64 sqrt and / may round the last fp64 bit differently:
through the float cast that is at most one float step). A refit's labelling is reproduced EXACTLY from the coefficients the device
returned; those are within 1e-9 of the twin's own fp64 refit -- with the eigen gaps pinned in tests/test_plane_cpu.py, fp64 rounding of
<= 4,099-term sums and a converged Jacobi stay below 1e-12 and a float32 leak would show at 1e-7. The inputs are those of the pinned
table, proven without a GPU on the same arrays. No cloud is larger than 4,099 points."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cluster_ref as K
from tests import outlier_ref as R
from tests import plane_ref as P
from tests import util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cloud(name):
    from fast_gicp_amd import preprocess
    a = np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099]) if name == "A" else None
    return P.named_cloud(name, a)


def axis_of(ax):
    return (P.Z, P.DEG10) if ax == "Z" else (None, 0.0)


@functools.lru_cache(maxsize=None)
def twin(name, t, H, seed, ax, flags):
    axis, eps = axis_of(ax)
    return P.segment(cloud(name), t, H, seed, axis, eps, flags)  # computed once, shared, never written to


@pytest.fixture(scope="module")
def vg():
    from fast_gicp_amd import capi
    v = capi.VoxelGrid(0)
    yield v
    v.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ulps64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


def check_state(vg, p, t, flags, tw, got):
    """the handle's state after a segmentation call equals the twin's result; `got` is what the call returned"""
    n = len(p)
    co, ninl = got
    m = vg.plane_model()
    ptr, out_n = vg.device_points()
    idx = vg.kept_indices()
    scores, threshold = vg.scores()
    assert m["counts"].dtype == np.int32 and np.array_equal(m["counts"], tw["counts"])  # every one of the H counts, the -1s included
    assert (m["winner"], m["valid"], m["count_winner"]) == (tw["winner"], tw["valid"], tw["count_winner"])
    assert np.array_equal(m["sample"], tw["sample"]) and np.array_equal(m["coefficients"], co) and m["num_inliers"] == ninl
    assert threshold == float(t) and scores.shape == (n,)
    if tw["winner"] < 0:
        assert not co.any() and ninl == 0 and np.all(np.isinf(scores)) and np.all(scores > 0)
        inl = np.zeros(n, bool)
    else:
        assert abs(np.linalg.norm(co[:3]) - 1.0) < 1e-12 and co[3] >= 0.0
        sc_t = tw["scores"]
        print("scores: max ulp", np.max(np.abs(scores.view(np.int32).astype(np.int64) - sc_t.view(np.int32).astype(np.int64))))
        assert np.all(np.abs(scores.view(np.int32).astype(np.int64) - sc_t.view(np.int32).astype(np.int64)) <= 1)  # (non-negative floats: ulp distance = integer distance)
        if tw["refit"]:
            inl = P.label_with(p, co, t)  # the labelling under the RETURNED doubles, reproduced exactly
            print("refit: |dn|", np.max(np.abs(co[:3] - tw["coefficients"][:3])), "|dd|", abs(co[3] - tw["coefficients"][3]))
            assert np.all(np.abs(co[:3] - tw["coefficients"][:3]) <= 1e-9)
            assert abs(co[3] - tw["coefficients"][3]) <= 1e-9 * (1.0 + float(np.max(np.abs(p))))
        else:
            inl = tw["inlier"]
            print("coefficients: ulp", ulps64(co, tw["coefficients"]))
            assert ulps64(co, tw["coefficients"]) <= 4 and ninl == tw["count_winner"]
    keep = ~inl if flags & P.KEEP_OUTLIERS else inl
    assert ninl == int(inl.sum()) and out_n == int(keep.sum())
    assert idx.dtype == np.int32 and np.array_equal(idx, np.flatnonzero(keep))
    assert same_bits(vg.get_points(out_n), p[keep])
    if not tw["refit"]:
        assert np.array_equal(idx, tw["idx"]) and same_bits(vg.get_points(out_n), tw["points"])
    from fast_gicp_amd import capi
    with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
        vg.cluster_labels()


def run_all_forms(vg, name, t, H, seed, ax, flags):
    import torch
    p, tw = cloud(name), twin(name, t, H, seed, ax, flags)
    axis, eps = axis_of(ax)
    n = len(p)
    got = vg.segment_plane(p, t, H, seed, axis, eps, flags=flags)
    check_state(vg, p, t, flags, tw, got)
    p4 = np.ascontiguousarray(np.hstack([p, np.full((n, 1), 7.0, np.float32)]))
    got4 = vg.segment_plane(p4, t, H, seed, axis, eps, flags=flags, stride=4)
    check_state(vg, p, t, flags, tw, got4)
    d3 = torch.from_numpy(p).to(torch.device("cuda", 0)).contiguous()
    gotd = vg.segment_plane((d3.data_ptr(), n), t, H, seed, axis, eps, flags=flags, device=True)
    check_state(vg, p, t, flags, tw, gotd)
    assert np.array_equal(got[0], got4[0]) and np.array_equal(got[0], gotd[0])  # the three forms return the same bits
    return tw


# ---- equality with the twin ----
@pytest.mark.parametrize("name,t,H,seed,ax,flags,valid,winner,count,inliers", P.TABLE)
def test_segmentation_equals_the_twin(vg, name, t, H, seed, ax, flags, valid, winner, count, inliers):
    tw = run_all_forms(vg, name, t, H, seed, ax, flags)
    assert (tw["valid"], tw["winner"], tw["count_winner"]) == (valid, winner, count)


@pytest.mark.parametrize("n", P.EDGE_N)
def test_segmentation_at_the_size_edges(vg, n):
    """n = 0 ... 4, the wave size +- 1, the slab size +- 1; with and without the refit, the axis and the complement"""
    for H, ax, flags in ((64, None, P.REFINE), (65, "Z", P.KEEP_OUTLIERS), (1, None, 0)):
        tw = run_all_forms(vg, "wall%d" % n, 0.05, H, 3, ax, flags)
        if n < 3:
            assert tw["winner"] == -1 and np.all(tw["counts"] == -1)


# ---- other behaviour ----
def test_two_runs_give_identical_bits_and_the_complement_is_exact(vg):
    p = cloud("wall")
    for flags in (0, P.REFINE):
        a = vg.segment_plane(p, 0.05, 64, 3, flags=flags)
        ia, sa, ma = vg.kept_indices(), vg.scores()[0], vg.plane_model()
        b = vg.segment_plane(p, 0.05, 64, 3, flags=flags)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1] == b[1]
        assert np.array_equal(ia, vg.kept_indices()) and same_bits(sa, vg.scores()[0]) and np.array_equal(ma["counts"], vg.plane_model()["counts"])
        c = vg.segment_plane(p, 0.05, 64, 3, flags=flags | P.KEEP_OUTLIERS)
        ic = vg.kept_indices()
        assert np.array_equal(a[0].view(np.uint64), c[0].view(np.uint64)) and a[1] == c[1] == len(ia) == len(p) - len(ic)
        assert np.array_equal(np.sort(np.concatenate([ia, ic])), np.arange(len(p))) and np.all(np.diff(ic) > 0)  # exactly the complement, in input order
        assert same_bits(vg.get_points(len(ic)), p[ic])


def test_the_axis_constraint_changes_the_winner(vg):
    p = cloud("wall")
    free, _ = vg.segment_plane(p, 0.05, 64, 3)
    w_free = vg.plane_model()["winner"]
    held, _ = vg.segment_plane(p, 0.05, 64, 3, P.Z, P.DEG10)
    w_held = vg.plane_model()["winner"]
    assert w_free == twin("wall", 0.05, 64, 3, None, 0)["winner"] != w_held == twin("wall", 0.05, 64, 3, "Z", 0)["winner"]
    assert abs(free[0]) > 0.99 and abs(held[2]) > 0.99  # the wall without the constraint, the ground with it


def test_crop_then_plane_then_cluster_chain_on_the_handles_own_output(vg):
    import torch
    p = cloud("wall")
    cropped = R.crop(p, 1.0, 60.0)["points"]
    assert 0 < len(cropped) < len(p)
    d = torch.from_numpy(p).to(torch.device("cuda", 0)).contiguous()
    ptr, m = vg.crop_range_device(d.data_ptr(), len(p), 1.0, 60.0)
    assert m == len(cropped) and (ptr, m) == vg.device_points()
    vg.segment_plane((ptr, m), 0.05, 64, 3, P.Z, P.DEG10, keep_outliers=True, device=True)  # input and output are the same buffer of the handle
    tp = P.segment(cropped, 0.05, 64, 3, P.Z, P.DEG10, P.KEEP_OUTLIERS)
    assert tp["winner"] >= 0 and 0 < len(tp["idx"]) < len(cropped)
    assert np.array_equal(vg.kept_indices(), tp["idx"]) and np.array_equal(vg.plane_model()["counts"], tp["counts"])
    ptr2, m2 = vg.device_points()
    assert m2 == len(tp["idx"]) and same_bits(vg.get_points(m2), tp["points"])
    labels, sizes = vg.cluster_euclidean((ptr2, m2), 0.5, 5, 0, device=True)  # ... and the objects standing on the removed ground
    tc = K.cluster(tp["points"], 0.5, 5, 0)
    assert tc["num_clusters"] >= 1 and np.array_equal(labels, tc["labels"]) and np.array_equal(sizes, tc["sizes"])
    assert np.array_equal(vg.kept_indices(), tc["idx"]) and same_bits(vg.get_points(len(tc["idx"])), tc["points"])
    from fast_gicp_amd import capi
    with pytest.raises(capi.FvhError, match="code 2"):  # the plane model is gone after the clustering call
        vg.plane_model()


def test_an_ndt_handle_takes_the_kept_points():
    from fast_gicp_amd import capi
    p = cloud("wall")
    tw = twin("wall", 0.05, 64, 3, "Z", P.KEEP_OUTLIERS)
    v = capi.VoxelGrid(0)
    v.segment_plane(p, 0.05, 64, 3, P.Z, P.DEG10, keep_outliers=True)
    c = capi.NDTMapCore(0)
    c.set_distance_mode(1); c.set_neighbor_search_method(1); c.set_resolution(1.0)
    c.set_target_cloud(p)
    c.set_source_cloud_from_voxelgrid(v)
    with pytest.raises(capi.FvhError):
        c.set_source_cloud_from_voxelgrid(v)  # an output can be taken once
    c.swap_source_and_target()
    assert same_bits(c.get_target_points(), tw["points"])
    assert same_bits(v.get_points(len(tw["idx"])), tw["points"])  # the packed output is still there
    assert np.array_equal(v.plane_model()["counts"], tw["counts"])
    v.close(); c.close()


def test_refusals_leave_the_handle_usable(vg):
    from fast_gicp_amd import capi
    u = cloud("wall")
    bad = u.copy()
    bad[17, 1] = np.nan
    inf = u.copy()
    inf[1999, 2] = np.inf
    p5 = np.zeros((100, 5), np.float32)
    S = vg.segment_plane
    errors = [lambda: S(u, 0.0), lambda: S(u, -1.0), lambda: S(u, np.nan), lambda: S(u, np.inf),                       # the threshold
              lambda: S(u, 0.05, 0), lambda: S(u, 0.05, -4), lambda: S(u, 0.05, 16385),                                  # H outside [1, 16384]
              lambda: S(u, 0.05, 64, 3, P.Z, -0.1), lambda: S(u, 0.05, 64, 3, P.Z, 1.6), lambda: S(u, 0.05, 64, 3, P.Z, np.nan),  # eps_angle with an axis
              lambda: S(u, 0.05, 64, 3, (0.0, 0.0, 0.0), 0.1), lambda: S(u, 0.05, 64, 3, (0.0, np.nan, 1.0), 0.1), lambda: S(u, 0.05, 64, 3, (np.inf, 0.0, 1.0), 0.1),  # the axis
              lambda: S(u, 0.05, flags=4), lambda: S(u, 0.05, flags=-1),                                                 # unknown flag bits
              lambda: S(p5, 0.05, stride=5), lambda: S((0, 10), 0.05, device=True), lambda: S((0, -1), 0.05, device=True),
              lambda: S(bad, 0.05), lambda: S(inf, 0.05, refine=True)]                                                  # non-finite coordinates
    for i, call in enumerate(errors):
        S(u, 0.05, 64, 3)  # a good state for the refused call to take away
        assert vg.device_points()[1] > 0
        with pytest.raises(capi.FvhError, match="code 1"):  # FVH_ERR_INVALID_ARGUMENT
            call()
        assert vg.device_points()[1] == 0, i  # a refused call leaves no output
        for getter in (vg.plane_model, vg.kept_indices, vg.scores):
            with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
                getter()
    lib = capi.load()
    a = np.ascontiguousarray(u)
    for null in range(3):  # null coefficients / num_inliers / out_n: the others are zeroed
        co, ni, m = np.full(4, 5.0), C.c_int(5), C.c_int(5)
        outs = [capi._p(co), C.byref(ni), C.byref(m)]
        outs[null] = None
        assert lib.fvh_voxelgrid_segment_plane(vg._h, capi._p(a), len(a), 0.05, 64, 3, None, 0.0, 0, *outs) == 1
        assert (null == 0 or not co.any()) and (null == 1 or ni.value == 0) and (null == 2 or m.value == 0)
    co, ni, m = np.full(4, 5.0), C.c_int(5), C.c_int(5)
    assert lib.fvh_voxelgrid_segment_plane(vg._h, None, 10, 0.05, 64, 3, None, 0.0, 0, capi._p(co), C.byref(ni), C.byref(m)) == 1 and not co.any() and (ni.value, m.value) == (0, 0)
    # eps_angle is not looked at without an axis; its two ends are legal with one
    tw = twin("wall", 0.05, 64, 3, None, 0)
    check_state(vg, u, 0.05, 0, tw, S(u, 0.05, 64, 3, None, -5.0))
    S(u, 0.05, 64, 3, P.Z, 0.0)
    t0 = P.segment(u, 0.05, 64, 3, P.Z, 0.0)
    assert t0["valid"] == 0 and vg.plane_model()["valid"] == 0 and vg.plane_model()["winner"] == -1  # no normal is exactly (0, 0, +-1): no model, FVH_OK
    S(u, 0.05, 64, 3, P.Z, np.pi / 2)
    assert np.array_equal(vg.plane_model()["counts"], P.segment(u, 0.05, 64, 3, P.Z, np.pi / 2)["counts"])
    # n == 0: FVH_OK with zeros; the getters answer
    co, ni = S(np.zeros((0, 3), np.float32), 0.05, 70)
    m0 = vg.plane_model()
    assert not co.any() and ni == 0 and vg.device_points()[1] == 0 and m0["winner"] == -1 and np.array_equal(m0["counts"], np.full(70, -1))
    assert len(vg.kept_indices()) == 0 and len(vg.scores()[0]) == 0
    # NULL outputs of the getter are legal
    S(u, 0.05, 64, 3)
    assert lib.fvh_voxelgrid_get_plane_model(vg._h, None, None, None, None) == 0
    # the handle still works
    check_state(vg, u, 0.05, 0, tw, S(u, 0.05, 64, 3))


def test_the_model_needs_a_segmentation_call(vg):
    from fast_gicp_amd import capi
    u = cloud("wall")
    others = [lambda: vg.crop_range(u, 4.0, 150.0), lambda: vg.remove_radius_outliers(u, 0.8, 2), lambda: vg.remove_statistical_outliers(u, 8, 1.0),
              lambda: vg.cluster_euclidean(u, 0.5, 2, 0), lambda: vg.filter(u, 0.5)]
    for other in others:
        vg.segment_plane(u, 0.05, 64, 3)
        assert vg.plane_model()["winner"] >= 0
        other()
        with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
            vg.plane_model()
    vg.segment_plane(u, 0.05, 64, 3)
    assert len(vg.kept_indices()) == vg.plane_model()["num_inliers"]


def test_counts_can_be_copied_to_device_memory(vg):
    import torch
    from fast_gicp_amd import capi
    tw = twin("wall", 0.05, 64, 3, None, 0)
    vg.segment_plane(cloud("wall"), 0.05, 64, 3)
    d_counts = torch.full((64,), -5, dtype=torch.int32, device=torch.device("cuda", 0))
    assert capi.load().fvh_voxelgrid_get_plane_model(vg._h, None, None, None, C.c_void_p(d_counts.data_ptr())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_counts.cpu().numpy(), tw["counts"])


def test_profile_classes(vg):
    u = cloud("wall")
    for refine in (False, True):
        vg.profile_enable(True); vg.profile_reset()
        vg.segment_plane(u, 0.05, 64, 3, refine=refine)
        got = {c: vg.profile_get(c) for c in ("plane", "compact", "sort", "cluster")}
        vg.profile_enable(False); vg.profile_reset()
        assert got["plane"][1] == 1 and got["compact"][1] == 1 and got["sort"] == (0.0, 0) and got["cluster"] == (0.0, 0), got
        assert got["plane"][0] > 0 and got["compact"][0] > 0, got


def test_pygicp_binding_equals_the_capi_route(vg):
    import torch  # noqa: F401  (its HIP runtime first, see tests/conftest.py)
    import pygicp
    u = cloud("wall")
    for kw in (dict(), dict(axis=P.Z, eps_angle=P.DEG10), dict(refine=True), dict(axis=P.Z, eps_angle=P.DEG10, keep_outliers=True, refine=True)):
        want = vg.segment_plane(u, 0.05, 64, 3, **kw)
        co, idx = pygicp.segment_plane_device(u, 0.05, max_iterations=64, seed=3, **kw)
        assert co.dtype == np.float64 and co.shape == (4,) and idx.dtype == np.int32
        assert np.array_equal(co.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(idx, vg.kept_indices())
    co, idx = pygicp.segment_plane_device(u, 0.05)  # the defaults: 256 hypotheses, seed 0, no axis, the inliers
    tw = P.segment(u, 0.05, 256, 0)
    assert np.array_equal(idx, tw["idx"])
    with pytest.raises(Exception):
        pygicp.segment_plane_device(u, -1.0)
