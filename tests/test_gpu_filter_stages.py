"""The stages of the voxel-grid filter handle against each other: every ordered pair of calls on ONE handle, and every refusal after
every other stage. The stages share the handle's buffers (keep flags, scanned positions, scores, kept indices, the scan's block sums and
a control block whose size differs per stage) and one "last call" state, so a stage must neither read what the stage before it left
there nor leave its getters answering after a later call.

For every ordered pair (A, B): A runs on the cloud, B runs in its device form on A's own device_points() (the aliased input), and B's
points, kept indices, scores, labels and plane model must be BIT-EQUAL to B run in its host form on the downloaded output of A on a fresh
handle -- both are the same kernels on the same input, so nothing but carried-over state can make them differ; no tolerance. After B
exactly the getters of B's row of the table in DESIGN.md answer and the others return FVH_ERR_BAD_STATE (2). A call refused for its
stride leaves no output and no getter, whatever succeeded before it.

The cloud (331 points: two 256-point blocks) is a jittered wall, two blobs and a few strays; every stage but deskew keeps at least 64 of
its points and drops at least one (test_every_stage_keeps_and_drops_on_the_cloud, with the numpy twins)."""
import functools
import itertools

import numpy as np
import pytest

from tests import cluster_ref as K
from tests import deskew_ref as D
from tests import outlier_ref as R
from tests import plane_ref as P

pytestmark = pytest.mark.gpu

STAGES = ("filter", "crop_range", "remove_statistical_outliers", "remove_radius_outliers", "deskew", "cluster_euclidean", "segment_plane")
# which getters answer after a successful call: (kept_indices and scores, cluster_labels, plane_model)
ROW = {"filter": (False, False, False), "crop_range": (True, False, False), "remove_statistical_outliers": (True, False, False),
       "remove_radius_outliers": (True, False, False), "deskew": (False, False, False), "cluster_euclidean": (True, True, False),
       "segment_plane": (True, False, True)}
LEAF = 0.5
CROP = (1e-3, 49.0)
SOR = (8, 1.0)
ROR = (0.8, 2)
CLUSTER = (0.6, 10, 0)
PLANE = (0.05, 64, 1)  # distance_threshold, max_iterations, seed


@functools.lru_cache(maxsize=None)
def cloud():
    rng = np.random.default_rng(5)
    wall = np.stack([np.full(171, 5.0) + rng.normal(0.0, 0.01, 171), rng.uniform(-3.0, 3.0, 171), rng.uniform(-1.5, 1.5, 171)], 1)
    blobs = np.concatenate([rng.normal(0.0, 0.25, (76, 3)) + [0.0, 3.0, 0.0], rng.normal(0.0, 0.25, (76, 3)) + [-1.0, -3.0, 0.5]])
    strays = np.array([[9.0, 9.0, 4.0], [-9.0, 8.0, -3.0], [8.0, -9.0, 5.0], [-8.0, -8.0, -5.0], [0.0, 0.0, 9.0], [0.0, 12.0, 0.0], [-12.0, 0.0, 1.0], [3.0, 0.5, -8.0]])
    p = np.concatenate([wall, blobs, strays]).astype(np.float32)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


@functools.lru_cache(maxsize=None)
def times():
    return D.azimuth_times(cloud())


@functools.lru_cache(maxsize=None)
def trajectory():
    return D.random_trajectory(5, 3)


def test_every_stage_keeps_and_drops_on_the_cloud():
    from fast_gicp_amd import preprocess
    p = cloud()
    n = len(p)
    assert n > 256
    kept = {"filter": len(preprocess.approximate_voxel_grid(p, LEAF)), "crop_range": int(R.crop(p, *CROP)["keep"].sum()),
            "remove_statistical_outliers": int(R.statistical(p, *SOR)["keep"].sum()), "remove_radius_outliers": int(R.radius(p, *ROR)["keep"].sum()),
            "cluster_euclidean": int(K.cluster(p, *CLUSTER)["keep"].sum()), "segment_plane": int(P.segment(p, *PLANE)["keep"].sum())}
    print(n, kept)
    for stage, m in kept.items():
        assert 64 <= m < n, (stage, m)


@pytest.fixture(scope="module")
def vg():
    from fast_gicp_amd import capi
    v = capi.VoxelGrid(0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def device_times():
    import torch
    return torch.from_numpy(times()).to(torch.device("cuda", 0)).contiguous()


def run(v, stage, points, t, stride=3):
    """one call of `stage`: points a host array (t: its host times) or a (device pointer, n) pair (t: the device pointer of its times)"""
    dev = isinstance(points, tuple)
    tau, T = trajectory()
    if stage == "filter":
        return v.filter_device(points[0], points[1], LEAF) if dev else v.filter(points, LEAF)
    if stage == "crop_range":
        return v.crop_range_device(*points, *CROP) if dev else v.crop_range(points, *CROP, stride=stride)
    if stage == "remove_statistical_outliers":
        return v.remove_statistical_outliers_device(*points, *SOR) if dev else v.remove_statistical_outliers(points, *SOR, stride=stride)
    if stage == "remove_radius_outliers":
        return v.remove_radius_outliers_device(*points, *ROR) if dev else v.remove_radius_outliers(points, *ROR, stride=stride)
    if stage == "deskew":
        return v.deskew_device(*points, t, tau, T) if dev else v.deskew(points, t, tau, T, stride=stride)
    if stage == "cluster_euclidean":
        return v.cluster_euclidean(points, *CLUSTER, device=dev, stride=stride)
    assert stage == "segment_plane"
    return v.segment_plane(points, *PLANE, device=dev, stride=stride)


def bits(x):
    """anything a getter returns, as something == compares bit for bit"""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in sorted(x.items())}
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    a = np.ascontiguousarray(x)
    return (a.dtype.str, a.shape, a.tobytes())


def observe(v):
    """(the output points, what each getter answered or None where it returned FVH_ERR_BAD_STATE)"""
    from fast_gicp_amd import capi
    _, m = v.device_points()
    out = {"count": m, "points": bits(v.get_points(m))}
    for name in ("kept_indices", "scores", "cluster_labels", "plane_model"):
        try:
            out[name] = bits(getattr(v, name)())
        except capi.FvhError as e:
            assert "(code 2)" in str(e), (name, str(e))
            out[name] = None
    return out


def answering(obs):
    assert (obs["kept_indices"] is None) == (obs["scores"] is None)
    return (obs["kept_indices"] is not None, obs["cluster_labels"] is not None, obs["plane_model"] is not None)


@pytest.mark.parametrize("a,b", list(itertools.product(STAGES, STAGES)))
def test_stage_b_after_stage_a_on_one_handle(vg, device_times, a, b):
    from fast_gicp_amd import capi
    run(vg, a, cloud(), times())
    ptr, m = vg.device_points()
    a_out = vg.get_points(m).copy()
    assert m >= 64 and ptr
    got_call = run(vg, b, (ptr, m), device_times.data_ptr())
    got = observe(vg)
    fresh = capi.VoxelGrid(0)
    try:
        want_call = run(fresh, b, a_out, times()[:m])
        want = observe(fresh)
    finally:
        fresh.close()
    print(a, "->", b, ":", len(cloud()), "->", m, "->", got["count"])
    assert got["count"] == want["count"] and got == want
    if b in ("cluster_euclidean", "segment_plane"):  # (labels, sizes) / (coefficients, num_inliers): what the call itself returned
        assert bits(got_call) == bits(want_call)
    else:
        assert got_call[1] == got["count"] and len(want_call) == want["count"]
    assert answering(got) == ROW[b]


@pytest.mark.parametrize("other,stage", [(o, s) for s in STAGES[1:] for o in STAGES if o != s])
def test_a_refused_call_leaves_nothing_of_the_stage_before(vg, other, stage):
    from fast_gicp_amd import capi
    run(vg, other, cloud(), times())
    assert answering(observe(vg)) == ROW[other] and vg.device_points()[1] >= 64
    with pytest.raises(capi.FvhError, match="stride must be 3 or 4 floats"):
        run(vg, stage, np.zeros((10, 5), np.float32), np.zeros(10, np.float32), stride=5)
    obs = observe(vg)
    assert obs["count"] == 0 and answering(obs) == (False, False, False)
