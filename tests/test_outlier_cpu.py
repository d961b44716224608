"""Range crop / outlier removal without a GPU: the numpy twin (tests/outlier_ref.py) against an independent fp64 brute force on lattices,
its crop against preprocess.remove_origin_points, the public surface (header, exported symbols, ctypes argtypes), the new kernels'
register budget, and the preconditions of tests/test_gpu_outlier.py (the margin table) proven on the very arrays that test uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import outlier_ref as R
from tests import util

NEW = (["fvh_voxelgrid_%s%s" % (b, s) for b in ("crop_range", "remove_statistical_outliers", "remove_radius_outliers") for s in ("", "_strided", "_device")]
       + ["fvh_voxelgrid_get_kept_indices", "fvh_voxelgrid_get_scores", "fvh_voxelgrid_profile_get_class"])


def _raw_scans():
    from fast_gicp_amd import preprocess
    return [preprocess.load_pcd(os.path.join(util.DATA, f)) for f in ("251370668.pcd", "251371071.pcd")]


@pytest.fixture(scope="module")
def cloud_a():
    from fast_gicp_amd import preprocess
    return np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099])


# ---- the twin against an independent fp64 brute force, on lattices (coordinates k / 2, |k| <= 4: every difference, square and sum of
# three squares is a multiple of 1/4 below 2^24 / 4 -- exact in fp32, so fp32 and fp64 brute force see the same d2) ----
def _brute64(p):
    p64 = np.asarray(p, np.float64)
    d2 = np.zeros((len(p), len(p)))
    for a in range(3):  # (another association and another loop order than the twin's)
        d2 += np.subtract.outer(p64[:, a], p64[:, a]) ** 2
    return d2


def test_twin_radius_equals_fp64_brute_force_on_a_lattice():
    p = R.cloud_lattice()
    assert len(p) == 729
    d2 = _brute64(p)
    for r, m in ((0.5, 6), (0.5, 4), (0.3, 1), (0.75, 18), (0.8, 19), (1.0, 200)):
        counts = (d2 <= float(np.float32(r)) ** 2).sum(axis=1) - 1
        tw = R.radius(p, r, m)
        assert np.array_equal(tw["counts"], counts), (r, m)
        assert np.array_equal(tw["keep"], counts >= m) and np.array_equal(tw["scores"], np.minimum(counts, m).astype(np.float32))
        assert np.array_equal(tw["points"].view(np.uint32), p[counts >= m].view(np.uint32)) and np.array_equal(tw["idx"], np.flatnonzero(counts >= m))
    # r equal to the spacing: the six axis neighbours sit at d2 == r2 exactly and count; interior points have exactly 6
    assert R.radius(p, 0.5, 6)["keep"].sum() == 7 ** 3
    # duplicates are neighbours of each other, a point is not its own
    q = np.concatenate([p, p[:10]])
    assert np.array_equal(R.radius(q, 0.25, 1)["idx"], np.concatenate([np.arange(10), 729 + np.arange(10)]))


def test_twin_statistical_equals_fp64_brute_force_on_a_lattice():
    p = R.cloud_lattice()
    n = len(p)
    d2 = np.sort(_brute64(p), axis=1)
    for k, mul in ((8, 1.0), (6, 0.5), (20, 2.0), (63, 1.0)):
        # fp64 sqrt instead of the twin's sqrtf: the scores agree to the rounding of sqrtf and of the final cast (2 x 6e-8), not to the bit
        d = np.sqrt(d2[:, 1:k + 1]).sum(axis=1) / k
        mu, var = d.mean(), d.var(ddof=1)
        t = mu + mul * np.sqrt(var)
        tw = R.statistical(p, k, mul)
        assert np.allclose(tw["scores"], d, rtol=2e-7, atol=0)
        assert abs(tw["threshold"] - t) <= 1e-6 * t and tw["var"] >= 0 and np.isfinite(tw["threshold"])
        if np.min(np.abs(d - t)) / t >= 1e-5:  # (the few distinct scores of a lattice: clear of the threshold, the kept sets are equal)
            assert np.array_equal(tw["keep"], d <= t), (k, mul)
    # a cloud of identical mean distances: the variance is clamped at 0, everything is kept
    ring = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], np.float32)
    tw = R.statistical(ring, 3, 1.0)
    assert tw["var"] >= 0 and tw["keep"].all()


def test_twin_crop_equals_remove_origin_points_on_the_raw_scans():
    from fast_gicp_amd import preprocess
    for raw in _raw_scans():
        tw = R.crop(raw, 1e-3, np.inf)
        want = preprocess.remove_origin_points(raw)
        assert 0 < len(want) < len(raw)
        assert np.array_equal(tw["points"].view(np.uint32), want.view(np.uint32))
        far = R.crop(raw, 1e-3, 400.0)
        assert 0 < len(far["points"]) < len(want) and R.sq_norm(far["points"]).max() <= 400.0
    bad = np.array([[1, 2, 3], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.01, 0.01, 0.01], [4, 5, 6]], np.float32)
    assert np.array_equal(R.crop(bad)["idx"], [0, 5])


# ---- the public surface ----
def test_header_library_and_capi_expose_the_filters():
    from fast_gicp_amd import build, capi
    declared = capi.declared_symbols()
    lib = build.build_lib()
    have = set(l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout.splitlines() if l.split())
    hdr = re.sub(r"/\*.*?\*/", "", open(build.HEADER).read(), flags=re.S)
    ctype = {"int": C.c_int, "double": C.c_double}
    L = capi.load()
    for name in NEW:
        assert name in declared and name in have, name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = arg.strip()
            if "*" in arg:
                want.append(C.c_char_p if arg.startswith("const char") else C.c_void_p)
            else:
                want.append(ctype[arg.split()[0]])
        assert capi.OUTLIER_ARGTYPES[name] == want, (name, m.group(1))
        assert list(getattr(L, name).argtypes) == want and getattr(L, name).restype is C.c_int
    for meth in ("crop_range", "crop_range_device", "remove_statistical_outliers", "remove_statistical_outliers_device", "remove_radius_outliers",
                 "remove_radius_outliers_device", "kept_indices", "scores", "profile_get"):
        assert callable(getattr(capi.VoxelGrid, meth, None)), meth
    # the kernels are device code of the library's one translation unit, launched by the host section
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_outlier.hpp")).read()
    host = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_outlier.inc.hpp")).read()
    stage = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_filter_stage.inc.hpp")).read()  # set-up and compaction of every mask stage
    for k in ("outlier_radius_count_kernel", "outlier_mean_dist_kernel", "outlier_stats_kernel", "outlier_flag_kernel", "crop_flag_kernel", "outlier_compact_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, src), k
        assert re.search(r"\b%s(<\d+>)?<<<" % k, stage if k == "outlier_compact_kernel" else host), k
    assert "mask_stage_setup(" in host and "upload_cloud(" in stage and stage.index("upload_cloud(") < stage.index("d.out.ensure(")  # the input is widened before the output state is touched
    for f in ("kernels_outlier.hpp", "host_outlier.inc.hpp"):
        assert any(s.endswith(os.sep + f) for s in build.SOURCES), f
    pyg = open(os.path.join(util.ROOT, "fast_gicp_amd", "python", "pygicp.cpp")).read()
    assert 'm.def("crop_range_device"' in pyg and 'm.def("remove_outliers_device"' in pyg


def test_new_kernels_fit_their_register_budget():
    """one query per wave relies on full occupancy like the sweep it is modelled on; nothing spills"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(util.ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.kernel_resources()
    hit = {k: v for k, v in res.items() if "outlier_radius_count_kernel" in k}
    assert len(hit) == 1, sorted(hit)
    v = list(hit.values())[0]
    assert v["occupancy"] >= 8 and v["vgpr_spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0, v
    for name, count in (("outlier_mean_dist_kernel", 2), ("outlier_stats_kernel", 1), ("outlier_flag_kernel", 1), ("crop_flag_kernel", 1), ("outlier_compact_kernel", 1),
                        ("outlier_finite_kernel", 1)):
        hit = {k: v for k, v in res.items() if name in k}
        assert len(hit) == count, (name, sorted(hit))
        for k, v in hit.items():
            assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
    # the names existing tests select kernels by do not occur in the new kernels' names
    for k in res:
        if "outlier" in k or "crop_flag" in k:
            name = k.split("(")[0]
            assert not any(s in name for s in ("knn_tiled1_kernel", "nn1_rows_kernel", "cov_rbf1_kernel", "cov_from_neighbors_kernel", "vm_accumulate_kernel", "sort_coop_kernel", "cost_kernel")), k


# ---- the preconditions of the GPU test, on its own inputs ----
def test_statistical_margin_table_holds_for_the_twin(cloud_a):
    """Every (cloud, mean_k, stddev_mul) the GPU test compares kept sets on keeps every score at least 1e-5 (relative) away from the
    threshold, and the twin keeps the number of points the table records."""
    clouds = {"A": cloud_a, "U": R.cloud_u()}
    assert len(cloud_a) == 4099 and len(clouds["U"]) == 2000
    near = {name: R.nearest_sq(p, 64) for name, p in clouds.items()}
    for name, k, mul, kept in R.SOR_TABLE:
        tw = R.statistical(clouds[name], k, mul, near[name])
        print("%s k=%d mul=%.1f margin=%.2e kept=%d t=%.9g" % (name, k, mul, tw["margin"], tw["keep"].sum(), tw["threshold"]))
        assert tw["margin"] >= R.SOR_MIN_MARGIN, (name, k, mul, tw["margin"])
        assert int(tw["keep"].sum()) == kept, (name, k, mul, int(tw["keep"].sum()))
    # the two combinations the table leaves out are indeed too close to call
    assert R.statistical(clouds["A"], 50, 0.5, near["A"])["margin"] < R.SOR_MIN_MARGIN
    assert R.statistical(clouds["U"], 50, 1.0, near["U"])["margin"] < R.SOR_MIN_MARGIN


def test_ragged_and_lattice_clouds_meet_the_precondition():
    for n in R.RAGGED_SIZES:
        p = R.cloud_ragged(n)
        assert len(p) == n and np.abs(p).max() <= 20
        assert R.ragged_stddev_mul(p) is not None, n
    d = R.cloud_duplicates()
    _, inverse, counts = np.unique(d, axis=0, return_inverse=True, return_counts=True)
    assert (counts[inverse.reshape(-1)] > 1).sum() == 100  # 50 copies + their 50 originals
    tw = R.statistical(R.cloud_lattice(), 8, 1.0)
    assert tw["var"] >= 0 and np.isfinite(tw["threshold"]) and tw["margin"] >= R.SOR_MIN_MARGIN and 0 < tw["keep"].sum() < 729
