"""CPU tests of the incremental target map's boundary (no GPU): header / ctypes / C++ / pygicp agree on the new calls, the numpy statement
of its contract (tests/incmap_ref.py) is self-consistent, and the preconditions the GPU tests rely on hold for the bundled pair."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import incmap_ref as R
from tests import util

NEW = {
    "fvh_vgicp_map_begin": ["fvh_vgicp*", "int"],
    "fvh_vgicp_map_insert_source": ["fvh_vgicp*", "const double*"],
    "fvh_vgicp_map_insert_cloud": ["fvh_vgicp*", "const float*", "int", "int", "const double*", "const double*", "int"],
    "fvh_vgicp_map_prune": ["fvh_vgicp*", "const double*", "double", "int", "int*"],
    "fvh_vgicp_map_get_info": ["fvh_vgicp*", "int*", "int*", "int*", "int*", "long long*", "int*"],
}


def _prototypes():
    hdr = open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fvh_vgicp_map_\w+)\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in args.split(",")]
    return out


def test_header_declares_the_map_calls_with_plain_signatures():
    protos = _prototypes()
    assert protos == NEW, protos  # pointers and scalars only: no struct crosses the boundary


def test_library_exports_and_capi_binds_the_map_calls():
    from fast_gicp_amd import build, capi
    lib = ctypes.CDLL(build.build_lib())
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.declared_symbols()
    for m in ("map_begin", "map_insert_source", "map_insert_cloud", "map_prune", "map_info"):
        assert callable(getattr(capi.VGICPCore, m)), m
    for name in NEW:  # (exported by the LIBRARY: declared_symbols() only parses the header)
        assert getattr(lib, name) is not None
    # the kernels are in the device code of the library's one translation unit
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_voxelmap.hpp")).read()
    for k in ("vm_insert_kernel", "vm_refresh_kernel", "vm_rehash_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, src), k


def test_capi_passes_what_the_header_declares():
    """capi.py calls through ctypes without argtypes, so a wrong argument count or a bare Python float where the header says `double`
    would only show on a GPU: record what every map_* method hands to the library and hold it against the parsed prototypes."""
    from fast_gicp_amd import capi
    calls = []
    core = object.__new__(capi.VGICPCore)
    core.h = None  # (never created: close() has nothing to destroy)
    core._call = lambda name, *args: calls.append((name, args))
    P, Cov, T = np.zeros((5, 3), np.float32), np.tile(np.eye(3), (5, 1, 1)), np.eye(4)
    core.map_begin(16); core.map_insert_source(T); core.map_insert_source(); core.map_insert_cloud(P, Cov, T)
    core.map_insert_cloud(None, Cov, T, device_ptr=4096, n=5, stride=4); core.map_prune([0, 0, 0], 2.5, 1); core.map_prune(None, 0.0, 3); core.map_info()
    assert [c[0] for c in calls] == ["map_begin", "map_insert_source", "map_insert_source", "map_insert_cloud", "map_insert_cloud", "map_prune", "map_prune", "map_get_info"]
    for name, args in calls:
        proto = NEW["fvh_vgicp_" + name][1:]  # (the handle is _call's own first argument)
        assert len(args) == len(proto), (name, len(args), proto)
        for a, t in zip(args, proto):
            if t == "double":
                assert isinstance(a, ctypes.c_double), (name, t, a)
            elif t == "int":
                assert isinstance(a, int) and not isinstance(a, bool), (name, t, a)
            else:  # a pointer: NULL, a raw address or a byref
                assert a is None or isinstance(a, ctypes.c_void_p) or type(a).__name__ == "CArgObject", (name, t, a)
    assert calls[5][1][1].value == 2.5 and calls[6][1][0] is None  # radius as a C double; a NULL centre = no distance rule
    assert calls[4][1][0].value == 4096 and calls[4][1][1:3] == (5, 4) and calls[4][1][5] == 1  # device cloud: pointer, n, stride, on_device


def test_registration_hpp_compiles_with_the_new_methods(tmp_path):
    """host-only build (g++, no HIP): FastVGICPCuda's incremental-target methods exist with the documented signatures"""
    src = tmp_path / "inc.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'using V = FastVGICPCuda<PointXYZ, PointXYZ>;\n'
                   'void (V::*a)(int) = &V::beginIncrementalTarget;\n'
                   'void (V::*b)(const Matrix4f&) = &V::insertSourceIntoTarget;\n'
                   'void (V::*c)() = &V::insertSourceIntoTarget;\n'
                   'int (V::*d)(const double*, double, int) = &V::pruneTarget;\n'
                   'bool (V::*e)() const = &V::hasIncrementalTarget;\n'
                   'int main() { return (a && b && c && d && e) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def test_pygicp_exposes_the_incremental_target():
    from fast_gicp_amd import build_host
    build_host.build_all()
    import pygicp
    assert {"begin_incremental_target", "insert_source_into_target", "prune_target"} <= set(dir(pygicp.FastVGICPCuda))
    assert "begin_incremental_target" not in dir(pygicp.NDTCuda)  # NDT maps are rebuilt per frame by design


def test_contract_in_numpy_is_self_consistent():
    rng = np.random.default_rng(3)
    P = rng.uniform(-40, 40, (500, 3)).astype(np.float32)
    A = rng.normal(size=(500, 3, 3))
    C = (A @ np.transpose(A, (0, 2, 1))).astype(np.float32)
    C = ((C + np.transpose(C, (0, 2, 1))) / 2).astype(np.float32)
    # identity: the inserted values ARE the inputs (the products are exact)
    Pi, Ci = R.transform_cloud(P, C, np.eye(4))
    assert np.array_equal(Pi, P) and np.array_equal(Ci, C)
    T = util.random_pose(rng, 20.0, 3.0)
    Pp, Cp = R.transform_cloud(P, C, T)
    assert Pp.dtype == np.float32 and Cp.dtype == np.float32 and np.array_equal(Cp, np.transpose(Cp, (0, 2, 1)))
    assert np.abs(Pp - (P.astype(np.float64) @ T[:3, :3].T + T[:3, 3])).max() < 1e-5
    # a point sits in the voxel whose centre is nearest: |p' - centre| <= res / 2 per axis
    for res in (1.0, 0.5, 0.3):
        c, ok = R.voxel_coords(Pp, res)
        assert ok.all()
        assert np.abs(Pp.astype(np.float64) - R.voxel_centres(c, res)).max() <= res / 2 + 1e-12
    bad = P.copy(); bad[0, 1] = np.nan; bad[1] = [3e9, 0, 0]
    assert list(np.nonzero(~R.voxel_coords(bad, 1.0)[1])[0]) == [0, 1]
    keep, slack = R.prune_keep(np.array([[0, 0, 0], [9, 0, 0]]), 1.0, [1.0, 1.0, 1.0], 5.0)
    assert list(keep) == [True, False] and abs(slack - 4.0) < 1e-12
    m = (np.array([[1, 2, 3], [0, 0, 0]]), np.array([4, 5]), np.ones((2, 3), np.float32), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)))
    s = R.map_spread(m, tuple(x[::-1] for x in m))  # the order of the getter does not matter
    assert s["mean_ulps"] == 0 and s["cov_excess"] == 0


def test_bundled_pair_meets_the_gpu_tests_preconditions():
    tgt, src = util.bundled_pair()
    T, k = R.safe_pose(src, util.relative_pose(), (1.0, 0.5))
    assert R.face_margin(src, T, 1.0) > 1e-6 and R.face_margin(src, T, 0.5) > 1e-6
    assert np.abs(T[:3, 3] - util.relative_pose()[:3, 3]).max() <= k * 3.0e-4 + 1e-15
    # the distance prune of the GPU test: no voxel centre on the sphere
    P = np.concatenate([tgt, (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)])
    c, ok = R.voxel_coords(P, 1.0)
    keep, slack = R.prune_keep(np.unique(c[ok], axis=0), 1.0, [1.0, -2.0, 0.5], 20.0)
    assert slack > 1e-9 and 0 < keep.sum() < len(keep)
