"""Euclidean cluster extraction without a GPU: the numpy twin (tests/cluster_ref.py) against an independent route (fp64 brute-force
adjacency + scipy's connected_components) on clouds where fp32 is exact, the pinned table of tests/test_gpu_cluster.py proven on the very
arrays that test uses, the chain cloud, the permutation rule, the public surface and the link kernel's register budget."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cluster_ref as K
from tests import outlier_ref as R
from tests import util

NEW = ["fvh_voxelgrid_cluster_euclidean", "fvh_voxelgrid_cluster_euclidean_strided", "fvh_voxelgrid_cluster_euclidean_device", "fvh_voxelgrid_get_cluster_labels"]


@pytest.fixture(scope="module")
def cloud_a():
    from fast_gicp_amd import preprocess
    return np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099])


def check_label_rule(tw, n):
    """labels / sizes obey the contract, whatever produced the components"""
    labels, sizes = tw["labels"], tw["sizes"]
    assert labels.dtype == np.int32 and sizes.dtype == np.int32 and labels.shape == (n,) and sizes.shape == (tw["num_clusters"],)
    assert np.array_equal(labels >= 0, tw["keep"]) and np.array_equal(np.flatnonzero(tw["keep"]), tw["idx"])
    if n == 0:
        return
    first = np.array([np.flatnonzero(labels == c)[0] for c in range(tw["num_clusters"])], np.int64)
    assert np.all(np.diff(first) > 0)  # numbered in ascending order of the smallest input index
    assert np.array_equal(np.bincount(labels[labels >= 0], minlength=tw["num_clusters"]), sizes)
    assert np.array_equal(tw["scores"][tw["keep"]], sizes[labels[tw["keep"]]].astype(np.float32))
    assert set(np.unique(labels[labels >= 0]).tolist()) == set(range(tw["num_clusters"]))


# ---- the twin against an independent route ----
def _scipy_components(p, tolerance):
    """fp64 brute-force adjacency (another association and loop order than the twin's) + scipy's connected components"""
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    p64 = np.asarray(p, np.float64)
    d2 = np.zeros((len(p), len(p)))
    for a in range(3):
        d2 += np.subtract.outer(p64[:, a], p64[:, a]) ** 2
    adj = d2 <= float(K.r2_of(tolerance))
    np.fill_diagonal(adj, False)
    return csgraph.connected_components(sparse.csr_matrix(adj), directed=False)


def _blobs():
    """eight blobs of lattice points (multiples of 1/4, so every d2 is exact in fp32) whose centres are 16 apart, rows shuffled"""
    rng = np.random.default_rng(21)
    parts = []
    for b in range(8):
        centre = np.array([(b & 1) * 16.0, ((b >> 1) & 1) * 16.0, ((b >> 2) & 1) * 16.0])
        parts.append(centre + rng.integers(-6, 7, (40 + 7 * b, 3)) * 0.25)
    p = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def test_twin_equals_scipy_connected_components_where_fp32_is_exact():
    pytest.importorskip("scipy")
    for p, tolerances in ((R.cloud_lattice(), (0.5, K.LATTICE_BELOW, 0.25, 0.75, 1.0)), (_blobs(), (0.25, 0.3, 0.5, 0.75, 3.0, 40.0))):
        for tol in tolerances:
            ncomp, comp = _scipy_components(p, tol)
            tw = K.cluster(p, tol, 1, 0)
            assert tw["num_clusters"] == ncomp, tol
            assert K.partition(tw["labels"]) == K.partition(comp), tol
            check_label_rule(tw, len(p))
            sizes = np.bincount(comp)
            for mn, mx in ((2, 0), (3, 50), (1, 1)):
                tw = K.cluster(p, tol, mn, mx)
                want = (sizes >= mn) & ((sizes <= mx) if mx > 0 else True)
                assert tw["num_clusters"] == int(want.sum()) and np.array_equal(tw["keep"], want[comp]), (tol, mn, mx)
                check_label_rule(tw, len(p))
    assert K.cluster(_blobs(), 3.0)["num_clusters"] == 8 and K.cluster(_blobs(), 40.0)["num_clusters"] == 1


# ---- the pinned table: the GPU test's inputs are non-degenerate, proven on the very same arrays ----
@pytest.mark.parametrize("name,tol,mn,mx,clusters,kept,largest", K.TABLE)
def test_pinned_table_holds_for_the_twin(cloud_a, name, tol, mn, mx, clusters, kept, largest):
    p = K.named_cloud(name, cloud_a)
    tw = K.cluster(p, tol, mn, mx)
    print(name, tol, mn, mx, tw["num_clusters"], len(tw["idx"]), tw["largest"])
    assert (tw["num_clusters"], len(tw["idx"]), tw["largest"]) == (clusters, kept, largest)
    check_label_rule(tw, len(p))
    assert tw["threshold"] == float(mn) and tw["points"].shape == (kept, 3)


def test_lattice_bound_is_inclusive_and_duplicates_are_connected():
    lat = R.cloud_lattice()
    assert np.float32(0.5) * np.float32(0.5) == np.float32(0.25) and K.LATTICE_BELOW < 0.5  # d2 == r2 exactly at the spacing
    assert K.cluster(lat, 0.5)["num_clusters"] == 1 and K.cluster(lat, K.LATTICE_BELOW)["num_clusters"] == 729
    d = R.cloud_duplicates()
    tw = K.cluster(d, 1e-6, 2, 0)
    assert np.all(tw["sizes"] == 2) and all(np.array_equal(d[list(s)][0], d[list(s)][1]) for s in K.partition(tw["labels"]))


def test_tile_edge_sizes():
    for n, c4, c8 in K.EDGE_SIZES:
        p = R.cloud_ragged(n)
        a, b = K.cluster(p, 4.0, 1, 0), K.cluster(p, 8.0, 2, 0)
        check_label_rule(a, n); check_label_rule(b, n)
        if c4 is not None:
            assert (a["num_clusters"], b["num_clusters"]) == (c4, c8), n
    one = K.cluster(R.cloud_ragged(1), 4.0, 1, 0)
    assert one["num_clusters"] == 1 and np.array_equal(one["labels"], [0]) and np.array_equal(one["sizes"], [1])
    assert K.cluster(R.cloud_ragged(1), 4.0, 2, 0)["num_clusters"] == 0
    empty = K.cluster(np.zeros((0, 3), np.float32), 1.0)
    assert empty["num_clusters"] == 0 and empty["labels"].shape == (0,) and empty["sizes"].shape == (0,)


def test_chain_cloud():
    """the helix: neighbours along the curve 0.1 apart, turns 0.25 apart -- one chain of 3,000 unions over 47 tiles, or none at all"""
    h = K.cloud_helix()
    assert h.shape == (3000, 3) and h.dtype == np.float32 and (3000 + 63) // 64 == 47
    one = K.cluster(h, 0.15)
    assert one["num_clusters"] == 1 and np.array_equal(one["sizes"], [3000]) and np.all(one["labels"] == 0)
    none = K.cluster(h, 0.09)
    assert none["num_clusters"] == 3000 and np.array_equal(none["labels"], np.arange(3000)) and np.all(none["sizes"] == 1)
    assert K.cluster(h, 0.09, 2, 0)["num_clusters"] == 0


def test_permuting_the_input_permutes_the_result():
    rng = np.random.default_rng(9)
    for p, tol, mn, mx in ((R.cloud_u(), 1.2, 2, 0), (R.cloud_u(), 1.6, 2, 100), (R.cloud_duplicates(), 0.5, 3, 0)):
        tw = K.cluster(p, tol, mn, mx)
        perm = rng.permutation(len(p))
        tp = K.cluster(p[perm], tol, mn, mx)
        assert np.array_equal(tp["scores"], tw["scores"][perm]) and np.array_equal(tp["keep"], tw["keep"][perm])
        assert tp["num_clusters"] == tw["num_clusters"]
        inv = np.argsort(perm)  # row i of p is row inv[i] of the permuted cloud
        assert K.partition(tp["labels"][inv]) == K.partition(tw["labels"])
        check_label_rule(tp, len(p))  # the smallest-index rule, in the permuted cloud's own indices


# ---- the public surface ----
def test_header_library_and_capi_expose_clustering():
    from fast_gicp_amd import build, capi
    declared = capi.declared_symbols()
    lib = build.build_lib()
    have = set(l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout.splitlines() if l.split())
    raw = open(build.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ctype = {"int": C.c_int, "double": C.c_double}
    L = capi.load()
    for name in NEW:
        assert name in declared and name in have, name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = arg.strip()
            want.append(C.c_void_p if "*" in arg else ctype[arg.split()[0]])  # only types the null-handle test knows
        assert capi.CLUSTER_ARGTYPES[name] == want, (name, m.group(1))
        assert list(getattr(L, name).argtypes) == want and getattr(L, name).restype is C.c_int
    for meth in ("cluster_euclidean", "cluster_labels", "kept_indices", "scores", "profile_get"):
        assert callable(getattr(capi.VoxelGrid, meth, None)), meth
    assert "sorts its clusters by size" in raw and '"cluster"' in raw  # the deviation from PCL and the profile class are part of the contract text
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_cluster.hpp")).read()
    host = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_cluster.inc.hpp")).read()
    for k in ("cluster_init_kernel", "cluster_link_kernel", "cluster_flatten_kernel", "cluster_flag_kernel", "cluster_label_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, src), k
        assert re.search(r"\b%s<<<" % k, host), k
    stage = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_filter_stage.inc.hpp")).read()
    for k in ("mask_stage_setup(", "mask_stage_compact(", "mask_stage_finish(", "ensure_sorted(", "device_scan("):  # the existing stages are reused, not copied
        assert k in host, k
    for k in ("outlier_finite_kernel<<<", "outlier_compact_kernel<<<", "device_scan("):  # (the shared layer launches what every mask stage launches)
        assert k in stage and (k == "device_scan(" or k not in host), k
    assert "upload_cloud(" not in host and "d.out.ensure(" not in host and stage.index("upload_cloud(") < stage.index("d.out.ensure(")  # the input is widened before the output state is touched
    # one synchronisation per entry point and one readback of the control words: the call's are the shared finish's, the getter's its own
    assert host.count("hipStreamSynchronize(") == 1 and host.count("hipMemcpyDeviceToHost") == 0 and host.count("mask_stage_finish(") == 1
    assert stage.count("hipStreamSynchronize(") == 1 and stage.count("hipMemcpyDeviceToHost") == 1
    # every access to parent[] in the link kernel is an agent-scope atomic
    link = src[src.index("void cluster_link_kernel"):src.index("void cluster_flatten_kernel")]
    assert not re.search(r"parent\s*\[", link) and "__HIP_MEMORY_SCOPE_AGENT" in src and "atomicCAS(" in src
    assert not re.search(r"atomic\w*\([^;]*float", src) and "__shared__" not in src
    for f in ("kernels_cluster.hpp", "host_cluster.inc.hpp"):
        assert any(s.endswith(os.sep + f) for s in build.SOURCES), f
    capi_hip = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "fvh_capi.hip")).read()
    assert capi_hip.index('#include "host_outlier.inc.hpp"') < capi_hip.index('#include "host_cluster.inc.hpp"')
    pyg = open(os.path.join(util.ROOT, "fast_gicp_amd", "python", "pygicp.cpp")).read()
    assert 'm.def("cluster_euclidean_device"' in pyg and 'm.def("remove_outliers_device"' in pyg


def test_link_kernel_fits_its_register_budget():
    """one query per wave relies on full occupancy like the sweep it is modelled on: no VGPR spill, and an occupancy not below that of
    outlier_radius_count_kernel"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(util.ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.kernel_resources()
    model = [v for k, v in res.items() if "outlier_radius_count_kernel" in k]
    link = [v for k, v in res.items() if "cluster_link_kernel" in k]
    assert len(model) == 1 and len(link) == 1, (model, link)
    print("link:", link[0], "model:", model[0])
    assert link[0]["vgpr_spill"] == 0 and link[0]["scratch"] == 0 and link[0]["lds"] == 0, link[0]
    assert link[0]["occupancy"] >= model[0]["occupancy"] >= 8, (link[0], model[0])
    for name in ("cluster_init_kernel", "cluster_flatten_kernel", "cluster_flag_kernel", "cluster_label_kernel"):
        hit = {k: v for k, v in res.items() if name in k}
        assert len(hit) == 1, (name, sorted(hit))
        for k, v in hit.items():
            assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
    # the names existing tests select kernels by do not occur in the new kernels' names
    for k in res:
        if "cluster_" in k.split("(")[0]:
            assert not any(s in k.split("(")[0] for s in ("knn_tiled1_kernel", "nn1_rows_kernel", "cov_rbf1_kernel", "cov_from_neighbors_kernel", "vm_accumulate_kernel", "sort_coop_kernel",
                                                           "cost_kernel", "outlier_")), k
