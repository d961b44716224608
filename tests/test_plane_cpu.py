"""RANSAC plane segmentation without a GPU: the numpy twin (tests/plane_ref.py) against an independent route on lattice clouds where fp64
is exact, the issue's prototype figures, the pinned table of tests/test_gpu_plane.py proven on the very arrays that test uses (with the
axis margins and eigen gaps its tolerances rest on), the public surface and the register budget of the plane_* kernels."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import plane_ref as P
from tests import util

NEW = ["fvh_voxelgrid_segment_plane", "fvh_voxelgrid_segment_plane_strided", "fvh_voxelgrid_segment_plane_device", "fvh_voxelgrid_get_plane_model"]
KERNELS = ("plane_hypo_kernel", "plane_sweep_kernel", "plane_winner_kernel", "plane_refit_partial_kernel", "plane_refit_final_kernel", "plane_flag_kernel")
TAKEN = ("outlier", "crop_flag", "deskew", "cluster_", "cost_kernel", "knn_", "nn1_", "cov_", "vm_", "sort_")  # substrings existing tests select kernels by


@pytest.fixture(scope="module")
def cloud_a():
    from fast_gicp_amd import preprocess
    return np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099])


def axis_of(name):
    return (P.Z, P.DEG10) if name == "Z" else (None, 0.0)


# ---- the generator ----
def test_mix32_and_the_sample_indices():
    assert P.mix32(0) == 0 and P.mix32(2**32) == 0  # uint32 wrap-around (the figures below pin the constants end to end)
    for seed in (0, 7, 2**32 - 1, 2**32, 2**64 - 1):
        assert 0 <= P.seed_word(seed) < 2**32
    assert P.seed_word(7) != P.seed_word(7 << 32)  # both halves of the seed count
    for n in (1, 2, 3, 65, 4099, 2**31 - 1):
        idx = P.sample_indices(7, 200, n)
        assert idx.shape == (200, 3) and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(P.sample_indices(7, 64, 4099), P.sample_indices(7, 256, 4099)[:64])  # hypothesis h does not depend on H
    assert np.all(P.sample_indices(5, 50, 1) == 0)


# ---- the issue's prototype figures: a twin that disagrees deviates from the text ----
def test_prototype_figures_on_the_bundled_source(cloud_a):
    r = P.segment(cloud_a, 0.1, 64, 7)
    assert (r["valid"], r["winner"], r["count_winner"]) == (64, 23, 1768)
    r = P.segment(cloud_a, 0.1, 64, 7, P.Z, P.DEG10)
    assert (r["valid"], r["winner"], r["count_winner"]) == (4, 14, 893)
    assert P.segment(cloud_a, 0.1, 256, 7)["winner"] == 23
    r = P.segment(cloud_a, 0.1, 256, 7, P.Z, P.DEG10)
    assert (r["valid"], r["winner"]) == (18, 14)


# ---- the twin against an independent route where fp64 is exact ----
def test_twin_equals_the_normalised_plane_route_on_lattice_clouds():
    """np.cross, a unit normal and |n.p + d| <= t: another formula (a square root and divisions) than the twin's division-free test. On
    multiples of 1/4 every product and sum of the twin is exact, and no distance lies within 1e-9 of t, so the two must agree on every count."""
    for p, t in ((P.cloud_slabs(), 0.3), (P.cloud_slabs(), 0.55), (P.cloud_two_planes(), 0.1)):
        p64 = p.astype(np.float64)
        H = 96
        hyp = P.hypotheses(p, H, 3)
        got = P.counts_of(p, hyp, t)
        closest = np.inf
        for h in range(H):
            i0, i1, i2 = hyp["idx"][h]
            nrm = np.cross(p64[i1] - p64[i0], p64[i2] - p64[i0])
            if len({i0, i1, i2}) < 3 or not nrm.any():
                assert got[h] == -1
                continue
            nrm = nrm / np.linalg.norm(nrm)
            dist = np.abs(p64 @ nrm - nrm @ p64[i0])
            closest = min(closest, np.min(np.abs(dist - t)))
            assert got[h] == int((dist <= t).sum()), h
        assert closest > 1e-9, closest
        assert (got >= 0).sum() > H // 2


# ---- the pinned table: the GPU test's inputs are what they are meant to be, proven on the very same arrays ----
@pytest.mark.parametrize("name,t,H,seed,ax,flags,valid,winner,count,inliers", P.TABLE)
def test_pinned_table_holds_for_the_twin(cloud_a, name, t, H, seed, ax, flags, valid, winner, count, inliers):
    p = P.named_cloud(name, cloud_a)
    assert len(p) <= 4099
    axis, eps = axis_of(ax)
    r = P.segment(p, t, H, seed, axis, eps, flags)
    print(name, t, H, seed, ax, flags, r["valid"], r["winner"], r["count_winner"], r["num_inliers"])
    assert (r["valid"], r["winner"], r["count_winner"], r["num_inliers"]) == (valid, winner, count, inliers)
    assert r["counts"].shape == (H,) and int((r["counts"] >= 0).sum()) == valid and (winner < 0 or r["counts"][winner] == r["counts"].max() == count)
    assert winner < 0 or not np.any(r["counts"][:winner] == count)  # ties go to the smallest h
    if axis is not None:  # no hypothesis sits within 1e-9 (relative) of the axis bound: the last bit of a cos cannot move one across
        c2 = math.cos(eps) ** 2
        rat = r["hyp"]["ratio"][r["hyp"]["ratio"] > 0]
        assert len(rat) and np.min(np.abs(rat - c2)) / c2 > 1e-9
    if flags & P.REFINE and winner >= 0:
        assert r["refit"] and r["eig"][1] > 0 and r["eig"][1] >= 100 * r["eig"][0], r["eig"]  # the eigen gap the 1e-9 of the GPU test rests on
        co = r["coefficients"]
        assert abs(np.linalg.norm(co[:3]) - 1) < 1e-12 and co[3] >= 0 and np.array_equal(r["inlier"], P.label_with(p, co, t))
    elif winner >= 0:
        assert not r["refit"] and inliers == count
    if winner < 0:
        assert not r["inlier"].any() and not r["coefficients"].any() and np.all(np.isinf(r["scores"]))
    keep_outliers = bool(flags & P.KEEP_OUTLIERS)
    assert np.array_equal(r["keep"], ~r["inlier"] if keep_outliers else r["inlier"]) and len(r["idx"]) == (len(p) - inliers if keep_outliers else inliers)


def test_the_tie_and_the_constrained_winner_are_what_the_gpu_test_means(cloud_a):
    # two parallel planes of equal size: a later hypothesis on the OTHER plane ties with the winner and loses
    p = P.cloud_two_planes()
    r = P.segment(p, 0.1, 65, 5)
    later = [h for h in range(r["winner"] + 1, 65) if r["counts"][h] == r["count_winner"] and p[r["hyp"]["idx"][h, 0], 2] != p[r["sample"][0], 2]]
    assert later, "no tie across the two planes"
    # a wall with more points than the ground: the axis constraint changes the winner, and the normals say which is which
    w = P.cloud_wall()
    free, held = P.segment(w, 0.05, 64, 3), P.segment(w, 0.05, 64, 3, P.Z, P.DEG10)
    assert free["winner"] != held["winner"] and abs(free["coefficients"][0]) > 0.99 and abs(held["coefficients"][2]) > 0.99
    assert free["count_winner"] > held["count_winner"] > 0


def test_edge_sizes_and_degenerate_clouds():
    for n in P.EDGE_N:
        p = P.named_cloud("wall%d" % n)
        assert len(p) == n
        r = P.segment(p, 0.05, 64, 3, None, 0.0, P.REFINE)
        assert (r["winner"] < 0) == (n < 3) and r["counts"].shape == (64,)
        if n < 3:
            assert r["valid"] == 0 and np.all(r["counts"] == -1) and r["num_inliers"] == 0 and len(r["idx"]) == 0
        else:
            assert r["count_winner"] >= 3 and r["refit"]
    assert P.SLAB - 1 in P.EDGE_N and P.SLAB + 1 in P.EDGE_N
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_plane.hpp")).read()
    assert re.search(r"constexpr int PLANE_SLAB = %d;" % P.SLAB, src)  # the twin's slab size is the kernel's


# ---- the public surface ----
def test_header_library_and_capi_expose_plane_segmentation():
    from fast_gicp_amd import build, capi
    declared = capi.declared_symbols()
    lib = build.build_lib()
    have = set(l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout.splitlines() if l.split())
    raw = open(build.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ctype = {"int": C.c_int, "double": C.c_double, "unsigned long long": C.c_ulonglong}
    L = capi.load()
    for name in NEW:
        assert name in declared and name in have, name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else ctype[arg.rsplit(" ", 1)[0]])  # only types the null-handle test knows
        assert capi.PLANE_ARGTYPES[name] == want, (name, m.group(1))
        assert list(getattr(L, name).argtypes) == want and getattr(L, name).restype is C.c_int
    assert re.search(r"enum fvh_plane_flags \{ FVH_PLANE_KEEP_OUTLIERS = 1, FVH_PLANE_REFINE = 2 \};", hdr)
    assert (capi.PLANE_KEEP_OUTLIERS, capi.PLANE_REFINE) == (P.KEEP_OUTLIERS, P.REFINE) == (1, 2)
    for meth in ("segment_plane", "plane_model", "kept_indices", "scores", "profile_get"):
        assert callable(getattr(capi.VoxelGrid, meth, None)), meth
    assert "DIFFERS from PCL" in raw and '"plane"' in raw and "0x7feb352d" in raw  # the deviation, the profile class and the generator are contract text
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_plane.hpp")).read()
    host = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_plane.inc.hpp")).read()
    for k in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\b" % k, src), k
        assert re.search(r"\b%s<<<" % k, host), k
        assert not any(s in k for s in TAKEN), k
    stage = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_filter_stage.inc.hpp")).read()
    for k in ("mask_stage_setup(", "mask_stage_compact(", "mask_stage_finish("):  # the existing stages are reused, not copied
        assert k in host, k
    for k in ("outlier_finite_kernel<<<", "outlier_compact_kernel<<<", "device_scan("):  # (the shared layer launches what every mask stage launches)
        assert k in stage and k not in host, k
    assert "ensure_sorted(" not in host  # no Morton sort: the samples are input indices, the sweep is dense
    assert "sym_eig3(" in src and "sqrt(" not in src[src.index("void plane_sweep_kernel"):src.index("void plane_winner_kernel")]
    assert src.count("#pragma clang fp contract(off)") >= 5 and not re.search(r"atomic\w*\([^;]*(float|double)", src)
    assert "upload_cloud(" not in host and "d.out.ensure(" not in host and stage.index("upload_cloud(") < stage.index("d.out.ensure(")  # the input is widened before the output state is touched
    # one synchronisation per entry point and one readback of the control words: the call's are the shared finish's, the getter's its own
    assert host.count("hipStreamSynchronize(") == 1 and host.count("hipMemcpyDeviceToHost") == 0 and host.count("mask_stage_finish(") == 1
    assert stage.count("hipStreamSynchronize(") == 1 and stage.count("hipMemcpyDeviceToHost") == 1
    for f in ("kernels_plane.hpp", "host_plane.inc.hpp"):
        assert any(s.endswith(os.sep + f) for s in build.SOURCES), f
    capi_hip = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "fvh_capi.hip")).read()
    assert capi_hip.index('#include "host_cluster.inc.hpp"') < capi_hip.index('#include "host_plane.inc.hpp"')
    pyg = open(os.path.join(util.ROOT, "fast_gicp_amd", "python", "pygicp.cpp")).read()
    assert 'm.def("segment_plane_device"' in pyg and 'm.def("cluster_euclidean_device"' in pyg


def test_plane_kernels_fit_their_register_budget():
    """no VGPR spill and no scratch in any plane_* kernel; the sweep keeps full occupancy with its 6 KiB slab; the names existing tests
    select kernels by do not occur in the new kernels' names"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(util.ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.kernel_resources()
    for name in KERNELS:
        hit = {k: v for k, v in res.items() if name in k}
        assert len(hit) == 1, (name, sorted(hit))
        for k, v in hit.items():
            print(k.split("(")[0], v)
            assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
    sweep = [v for k, v in res.items() if "plane_sweep_kernel" in k][0]
    assert sweep["lds"] == 3 * 8 * P.SLAB and sweep["occupancy"] >= 8, sweep
    ours = [k.split("(")[0] for k in res if "plane_" in k.split("(")[0]]
    assert len(ours) == len(KERNELS), ours
    for k in ours:
        assert not any(s in k for s in TAKEN), k
