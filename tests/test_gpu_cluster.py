"""Euclidean cluster extraction on the voxel-grid handle (fvh_voxelgrid_cluster_euclidean) against the numpy twin of its contract
(tests/cluster_ref.py). Twin and kernel evaluate the same fp32 d2, and everything the call returns is an integer or a bit copy, so labels,
sizes, counts, kept indices, kept points (compared as uint32), scores and threshold must be EQUAL. The inputs are those of the pinned
table in tests/test_cluster_cpu.py, which proves without a GPU that they are non-degenerate. No cloud is larger than 4,099 points."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cluster_ref as K
from tests import outlier_ref as R
from tests import util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cloud(name):
    from fast_gicp_amd import preprocess
    a = np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099]) if name == "A" else None
    return K.named_cloud(name, a)


@functools.lru_cache(maxsize=None)
def twin(name, tol, mn, mx):
    return K.cluster(cloud(name), tol, mn, mx)  # computed once, shared, never written to


@pytest.fixture(scope="module")
def vg():
    from fast_gicp_amd import capi
    v = capi.VoxelGrid(0)
    yield v
    v.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_state(vg, tw, n_in):
    """the handle's state after a clustering call equals the twin's result"""
    labels, sizes = vg.cluster_labels()
    ptr, out_n = vg.device_points()
    idx = vg.kept_indices()
    scores, threshold = vg.scores()
    assert labels.dtype == np.int32 and labels.shape == (n_in,) and np.array_equal(labels, tw["labels"])
    assert sizes.dtype == np.int32 and np.array_equal(sizes, tw["sizes"])
    assert vg.num_clusters == tw["num_clusters"] and out_n == len(tw["idx"])
    assert idx.dtype == np.int32 and np.array_equal(idx, tw["idx"])
    assert same_bits(vg.get_points(out_n), tw["points"])
    assert scores.shape == (n_in,) and same_bits(scores, tw["scores"])
    assert threshold == tw["threshold"]


def run_all_forms(vg, p, tol, mn, mx, tw):
    import torch
    n = len(p)
    got = vg.cluster_euclidean(p, tol, mn, mx)
    assert np.array_equal(got[0], tw["labels"]) and np.array_equal(got[1], tw["sizes"])
    check_state(vg, tw, n)
    p4 = np.ascontiguousarray(np.hstack([p, np.full((n, 1), 7.0, np.float32)]))
    vg.cluster_euclidean(p4, tol, mn, mx, stride=4)
    check_state(vg, tw, n)
    d3 = torch.from_numpy(p).to(torch.device("cuda", 0)).contiguous()
    vg.cluster_euclidean((d3.data_ptr(), n), tol, mn, mx, device=True)
    check_state(vg, tw, n)


# ---- equality with the twin ----
@pytest.mark.parametrize("name,tol,mn,mx,clusters,kept,largest", K.TABLE)
def test_clustering_equals_the_twin(vg, name, tol, mn, mx, clusters, kept, largest):
    tw = twin(name, tol, mn, mx)
    assert (tw["num_clusters"], len(tw["idx"])) == (clusters, kept)
    run_all_forms(vg, cloud(name), tol, mn, mx, tw)


@pytest.mark.parametrize("n,c4,c8", K.EDGE_SIZES)
def test_clustering_at_the_tile_edges(vg, n, c4, c8):
    name = "ragged%d" % n
    for tol, mn, want in ((4.0, 1, c4), (8.0, 2, c8)):
        tw = twin(name, tol, mn, 0)
        assert want is None or tw["num_clusters"] == want
        run_all_forms(vg, cloud(name), tol, mn, 0, tw)


# ---- other behaviour ----
def test_two_runs_agree_and_a_shuffle_gives_the_same_partition(vg):
    p = cloud("U")
    tw = twin("U", 1.2, 2, 0)
    a = vg.cluster_euclidean(p, 1.2, 2, 0)
    pts_a, idx_a, sc_a = vg.get_points(vg.device_points()[1]), vg.kept_indices(), vg.scores()
    b = vg.cluster_euclidean(p, 1.2, 2, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], tw["labels"])
    assert same_bits(pts_a, vg.get_points(vg.device_points()[1])) and np.array_equal(idx_a, vg.kept_indices()) and same_bits(sc_a[0], vg.scores()[0]) and sc_a[1] == vg.scores()[1]
    perm = np.random.default_rng(9).permutation(len(p))
    labels_p, sizes_p = vg.cluster_euclidean(p[perm], 1.2, 2, 0)
    assert same_bits(vg.scores()[0], tw["scores"][perm])
    inv = np.argsort(perm)
    assert K.partition(labels_p[inv]) == K.partition(tw["labels"]) and sorted(sizes_p.tolist()) == sorted(tw["sizes"].tolist())
    check_state(vg, K.cluster(p[perm], 1.2, 2, 0), len(p))  # ... and the smallest-index rule in the shuffled cloud's own indices


def test_crop_then_cluster_chains_on_the_handles_own_output(vg):
    import torch
    p = cloud("U")
    cropped = R.crop(p, 9.0, 120.0)["points"]
    assert 0 < len(cropped) < len(p)
    d = torch.from_numpy(p).to(torch.device("cuda", 0)).contiguous()
    ptr, m = vg.crop_range_device(d.data_ptr(), len(p), 9.0, 120.0)
    assert m == len(cropped) and (ptr, m) == vg.device_points()
    vg.cluster_euclidean((ptr, m), 1.6, 2, 0, device=True)  # input and output are the same buffer of the handle
    tw = K.cluster(cropped, 1.6, 2, 0)
    assert 1 < tw["num_clusters"] and 0 < len(tw["idx"]) < len(cropped)
    check_state(vg, tw, len(cropped))


def test_an_ndt_handle_takes_the_kept_points():
    from fast_gicp_amd import capi
    p = cloud("U")
    tw = twin("U", 1.6, 2, 0)
    v = capi.VoxelGrid(0)
    v.cluster_euclidean(p, 1.6, 2, 0)
    c = capi.NDTMapCore(0)
    c.set_distance_mode(1); c.set_neighbor_search_method(1); c.set_resolution(1.0)
    c.set_target_cloud(p)
    c.set_source_cloud_from_voxelgrid(v)
    with pytest.raises(capi.FvhError):
        c.set_source_cloud_from_voxelgrid(v)  # an output can be taken once
    c.swap_source_and_target()
    assert same_bits(c.get_target_points(), tw["points"])
    assert same_bits(v.get_points(len(tw["idx"])), tw["points"])  # the packed output is still there
    labels, sizes = v.cluster_labels()
    assert np.array_equal(labels, tw["labels"]) and np.array_equal(sizes, tw["sizes"])
    v.close(); c.close()


def test_refusals_leave_the_handle_usable(vg):
    from fast_gicp_amd import capi
    u = cloud("U")
    tw = twin("U", 1.2, 2, 0)
    bad = u.copy()
    bad[17, 1] = np.nan
    inf = u.copy()
    inf[1999, 2] = np.inf
    p5 = np.zeros((100, 5), np.float32)
    errors = [lambda: vg.cluster_euclidean(u, 0.0), lambda: vg.cluster_euclidean(u, -1.0), lambda: vg.cluster_euclidean(u, np.nan), lambda: vg.cluster_euclidean(u, np.inf),
              lambda: vg.cluster_euclidean(u, 1.2, 0), lambda: vg.cluster_euclidean(u, 1.2, -3), lambda: vg.cluster_euclidean(u, 1.2, 10, 5), lambda: vg.cluster_euclidean(u, 1.2, 2, 1),
              lambda: vg.cluster_euclidean(p5, 1.2, stride=5), lambda: vg.cluster_euclidean((0, 10), 1.2, device=True), lambda: vg.cluster_euclidean((0, -1), 1.2, device=True),
              lambda: vg.cluster_euclidean(bad, 1.2, 2), lambda: vg.cluster_euclidean(inf, 1.2, 2)]
    for i, call in enumerate(errors):
        vg.cluster_euclidean(u, 1.2, 2, 0)  # a good state for the refused call to take away
        with pytest.raises(capi.FvhError, match="code 1"):  # FVH_ERR_INVALID_ARGUMENT
            call()
        assert vg.device_points()[1] == 0 and vg.num_clusters == 0, i  # a refused call leaves no output
        for getter in (vg.cluster_labels, vg.kept_indices, vg.scores):
            with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
                getter()
    lib = capi.load()
    a = np.ascontiguousarray(u)
    nc, m = C.c_int(5), C.c_int(5)
    assert lib.fvh_voxelgrid_cluster_euclidean(vg._h, capi._p(a), len(a), 1.2, 2, 0, C.byref(nc), None) == 1 and nc.value == 0  # null out_n
    assert lib.fvh_voxelgrid_cluster_euclidean(vg._h, capi._p(a), len(a), 1.2, 2, 0, None, C.byref(m)) == 1 and m.value == 0  # null num_clusters
    nc, m = C.c_int(5), C.c_int(5)
    assert lib.fvh_voxelgrid_cluster_euclidean(vg._h, None, 10, 1.2, 2, 0, C.byref(nc), C.byref(m)) == 1 and (nc.value, m.value) == (0, 0)  # null points
    # max_cluster_size <= 0 is "no upper bound", max == min is a window of one size
    vg.cluster_euclidean(u, 1.2, 2, -7)
    check_state(vg, tw, len(u))
    vg.cluster_euclidean(u, 1.2, 2, 2)
    check_state(vg, K.cluster(u, 1.2, 2, 2), len(u))
    # n == 0: FVH_OK with zeros; the getters answer (with nothing)
    labels, sizes = vg.cluster_euclidean(np.zeros((0, 3), np.float32), 1.2)
    assert labels.shape == (0,) and sizes.shape == (0,) and vg.num_clusters == 0 and vg.device_points()[1] == 0
    assert len(vg.kept_indices()) == 0 and len(vg.scores()[0]) == 0
    # NULL outputs of the getter are legal
    vg.cluster_euclidean(u, 1.2, 2, 0)
    assert lib.fvh_voxelgrid_get_cluster_labels(vg._h, None, None) == 0
    # a huge tolerance: r * r overflows fp32, clamped -- one cluster of everything
    vg.cluster_euclidean(u, 1e30, 1, 0)
    check_state(vg, K.cluster(u, 1e30, 1, 0), len(u))
    assert vg.num_clusters == 1
    # the handle still works
    vg.cluster_euclidean(u, 1.2, 2, 0)
    check_state(vg, tw, len(u))


def test_labels_need_a_clustering_call(vg):
    from fast_gicp_amd import capi
    u = cloud("U")
    vg.cluster_euclidean(u, 1.2, 2, 0)
    assert len(vg.cluster_labels()[0]) == len(u)
    vg.crop_range(u, 4.0, 150.0)  # a crop: its own side outputs are there, the labels are gone
    assert len(vg.kept_indices()) > 0
    with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
        vg.cluster_labels()
    vg.cluster_euclidean(u, 1.2, 2, 0)
    vg.remove_radius_outliers(u, 0.8, 2)
    with pytest.raises(capi.FvhError, match="code 2"):
        vg.cluster_labels()
    vg.cluster_euclidean(u, 1.2, 2, 0)
    vg.filter(u, 0.5)  # a voxel filter: every side output is gone
    for getter in (vg.cluster_labels, vg.kept_indices, vg.scores):
        with pytest.raises(capi.FvhError, match="code 2"):
            getter()


def test_labels_can_be_copied_to_device_memory(vg):
    import torch
    u = cloud("U")
    tw = twin("U", 1.2, 2, 0)
    vg.cluster_euclidean(u, 1.2, 2, 0)
    d_labels = torch.full((len(u),), -5, dtype=torch.int32, device=torch.device("cuda", 0))
    d_sizes = torch.full((tw["num_clusters"],), -5, dtype=torch.int32, device=torch.device("cuda", 0))
    from fast_gicp_amd import capi
    assert capi.load().fvh_voxelgrid_get_cluster_labels(vg._h, C.c_void_p(d_labels.data_ptr()), C.c_void_p(d_sizes.data_ptr())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_labels.cpu().numpy(), tw["labels"]) and np.array_equal(d_sizes.cpu().numpy(), tw["sizes"])


def test_profile_classes(vg):
    u = cloud("U")
    vg.profile_enable(True); vg.profile_reset()
    vg.cluster_euclidean(u, 1.2, 2, 0)
    got = {c: vg.profile_get(c) for c in ("sort", "cluster", "compact", "outlier_count")}
    vg.profile_enable(False); vg.profile_reset()
    assert got["sort"][1] == 1 and got["cluster"][1] == 1 and got["compact"][1] == 1 and got["outlier_count"] == (0.0, 0), got
    assert all(ms > 0 for c, (ms, k) in got.items() if c != "outlier_count"), got


def test_pygicp_binding_equals_the_capi_route(vg):
    import torch  # noqa: F401  (its HIP runtime first, see tests/conftest.py)
    import pygicp
    u = cloud("U")
    for tol, mn, mx in ((1.2, 2, 0), (1.6, 2, 100)):
        want = vg.cluster_euclidean(u, tol, mn, mx)
        labels, sizes = pygicp.cluster_euclidean_device(u, tol, min_cluster_size=mn, max_cluster_size=mx)
        assert labels.dtype == np.int32 and labels.shape == (len(u),) and sizes.dtype == np.int32
        assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[1])
    labels, sizes = pygicp.cluster_euclidean_device(u, 1.2)  # the defaults: min 1, no upper bound
    tw = twin("U", 1.2, 1, 0)
    assert np.array_equal(labels, tw["labels"]) and np.array_equal(sizes, tw["sizes"])
    with pytest.raises(Exception):
        pygicp.cluster_euclidean_device(u, -1.0)
