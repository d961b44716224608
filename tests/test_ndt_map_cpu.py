"""Incremental NDT target map, the parts that need no GPU: the C ABI surface, the numpy contract's own arithmetic (tests/ndtmap_ref.py) and
the snapshot file format with mode 3 (FVH_VOXEL_NDT_SUMS)."""
import ctypes
import os
import re

import numpy as np

from tests import ndtmap_ref as N
from tests import util

SYMBOLS = ["fvh_ndt_map_begin", "fvh_ndt_map_insert_source", "fvh_ndt_map_insert_cloud", "fvh_ndt_map_prune", "fvh_ndt_map_get_info",
           "fvh_ndt_voxelmap_export", "fvh_ndt_voxelmap_import", "fvh_ndt_voxelmap_merge_from"]


def test_library_exports_and_header_declares_the_ndt_map_calls():
    from fast_gicp_amd import build, capi
    lib = ctypes.CDLL(build.build_lib())
    declared = capi.declared_symbols()
    for s in SYMBOLS:
        assert s in declared, "%s is not declared in include/fast_vgicp_hip.h" % s
        assert hasattr(lib, s), "%s is not exported by the library" % s
    hdr = open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()
    assert re.search(r"FVH_VOXEL_NDT_SUMS\s*=\s*3\b", hdr)
    assert capi.VOXEL_NDT_SUMS == 3
    for name in ("map_begin", "map_insert_source", "map_insert_cloud", "map_prune", "map_info", "map_export", "map_import", "map_merge_from", "map_save", "map_load"):
        assert callable(getattr(capi.NDTMapCore, name, None)), name
    assert issubclass(capi.NDTMapCore, capi.NDTCore)


def test_pygicp_and_the_cpp_class_expose_the_ndt_incremental_target(tmp_path):
    """pygicp.NDTCudaMap: NDTCuda + FastVGICPCuda's incremental-target names (NDTCuda itself keeps the reference's surface); the C++ NDTCuda has
    the methods with FastVGICPCuda's signatures (host-only compile, no HIP)."""
    import subprocess
    from fast_gicp_amd import build_host
    build_host.build_all()
    import pygicp
    names = {"begin_incremental_target", "insert_source_into_target", "prune_target", "export_target_map", "import_target_map", "merge_target_from",
             "save_target_map", "load_target_map"}
    assert names <= set(dir(pygicp.NDTCudaMap)) and names <= set(dir(pygicp.FastVGICPCuda))
    assert issubclass(pygicp.NDTCudaMap, pygicp.NDTCuda)
    src = tmp_path / "ndt_inc.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'using V = NDTCuda<PointXYZ, PointXYZ>;\n'
                   'void (V::*a)(int) = &V::beginIncrementalTarget;\n'
                   'void (V::*b)(const Matrix4f&) = &V::insertSourceIntoTarget;\n'
                   'void (V::*c)() = &V::insertSourceIntoTarget;\n'
                   'int (V::*d)(const double*, double, int) = &V::pruneTarget;\n'
                   'bool (V::*e)() const = &V::hasIncrementalTarget;\n'
                   'TargetMapSnapshot (V::*f)() = &V::exportTargetMap;\n'
                   'void (V::*g)(const TargetMapSnapshot&) = &V::importTargetMap;\n'
                   'void (V::*h)(V&) = &V::mergeTargetFrom;\n'
                   'void (V::*i)(const std::string&) = &V::saveTargetMap;\n'
                   'void (V::*j)(const std::string&) = &V::loadTargetMap;\n'
                   'int main() { return (a && b && c && d && e && f && g && h && i && j) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def _cloud(seed, n, lo=-20.0, hi=20.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def test_sums_of_two_scans_equal_the_sums_of_their_concatenation():
    """Voxel sums add: scan A + scan B against the concatenation, per entry within 2 (n - 1) 2^-53 sum|x| (two summation orders of the same
    terms); coordinates and counts exactly."""
    res = 1.0
    A, B = _cloud(1, 6000), N.transform_points(_cloud(2, 5000), np.array([[0.8, -0.6, 0, 1.5], [0.6, 0.8, 0, -2.25], [0, 0, 1, 0.5], [0, 0, 0, 1]]))
    a, b, ab = N.voxel_sums(A, res), N.voxel_sums(B, res), N.voxel_sums(np.concatenate([A, B]), res)
    index = {tuple(c): i for i, c in enumerate(ab["coords"])}
    total = np.zeros_like(ab["sums"])
    for part in (a, b):
        rows = np.array([index[tuple(c)] for c in part["coords"]])
        assert len(set(rows.tolist())) == len(rows)
        total[rows] += part["sums"]
    assert set(index) == {tuple(c) for c in a["coords"]} | {tuple(c) for c in b["coords"]}
    assert np.array_equal(total[:, 9], ab["sums"][:, 9]) and int(ab["sums"][:, 9].sum()) == len(A) + len(B)
    bound = N.sum_order_bound(ab["sums"][:, 9], ab["abs_sums"])
    d = np.abs(total - ab["sums"])
    print("two scans vs concatenation: largest |difference| / bound %.3g over %d voxels" % (float((d / np.maximum(bound, 1e-300)).max()), len(ab["coords"])))
    assert np.all(d <= bound)
    # rows come in ascending packed-key order: z-major, then y, then x
    c = ab["coords"].astype(np.int64)
    key = (c[:, 2] << 42) + (c[:, 1] << 21) + c[:, 0]
    assert np.all(np.diff(key) > 0)


def test_skipped_points_and_single_point_voxels_in_the_contract():
    P = np.array([[0.6, 0.6, 0.6], [np.nan, 0, 0], [3e9, 0, 0], [0.7, 0.6, 0.6], [5.6, 0.6, 0.6]], np.float32)
    v = N.voxel_sums(P, 1.0)
    assert v["coords"].tolist() == [[0, 0, 0], [5, 0, 0]] and v["sums"][:, 9].tolist() == [2.0, 1.0]
    s = v["sums"][1]  # one point: sum pp^T - mean sum p^T vanishes exactly
    mean = s[:3] / s[9]
    assert s[3] - mean[0] * s[0] == 0.0 and s[6] - mean[1] * s[1] == 0.0 and s[8] - mean[2] * s[2] == 0.0
    assert np.all(v["delta"] > 0) and np.all(v["delta"] < 1e-12)


def test_mode_3_snapshot_file_round_trip_is_byte_equal(tmp_path):
    from fast_gicp_amd import capi
    v = N.voxel_sums(_cloud(3, 3000), 0.5)
    n = len(v["coords"])
    snap = dict(resolution=0.5, mode=capi.VOXEL_NDT_SUMS, num_inserts=3, num_points=3000, num_voxels=n, coords=v["coords"], sums=v["sums"],
                ages=(np.arange(n) % 3).astype(np.uint32))
    p1, p2 = str(tmp_path / "a.fvhmap"), str(tmp_path / "b.fvhmap")
    capi.write_map_file(p1, snap)
    back = capi.read_map_file(p1)
    assert back["mode"] == 3 and back["num_voxels"] == n and back["resolution"] == 0.5 and back["num_inserts"] == 3 and back["num_points"] == 3000
    for k in ("coords", "sums", "ages"):
        assert np.array_equal(back[k], snap[k]) and back[k].dtype == snap[k].dtype, k
    capi.write_map_file(p2, back)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    assert os.path.getsize(p1) == 40 + 96 * n
