"""CPU tests of the target-from-map boundary (no GPU): header / library / ctypes / C++ / pygicp agree on fvh_vgicp_target_from_map,
fvh_ndt_target_from_map and the two get_target_points calls, the kernels are where the design says, and the numpy statement of the
contract (tests/targetmap_ref.py) orders voxels as the engine's packed key does."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import mapsnap_ref as S
from tests import table_sim
from tests import targetmap_ref as TM
from tests import util

NEW = {
    "fvh_vgicp_target_from_map": ["fvh_vgicp*", "int", "int*"],
    "fvh_ndt_target_from_map": ["fvh_ndt*", "int", "int*"],
    "fvh_vgicp_get_target_points": ["fvh_vgicp*", "float*"],
    "fvh_ndt_get_target_points": ["fvh_ndt*", "float*"],
}


def _prototypes():
    hdr = open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fvh_(?:vgicp|ndt)_(?:target_from_map|get_target_points))\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in args.split(",")]
    return out


def test_header_declares_the_four_calls():
    assert _prototypes() == NEW, _prototypes()
    # the names stay clear of the two patterns whose prototype sets other tests pin
    assert not any(re.match(r"fvh_vgicp_map_\w+$|fvh_vgicp_voxelmap_\w+$", n) for n in NEW)


def test_library_exports_the_calls_and_holds_the_kernels():
    from fast_gicp_amd import build, capi
    lib = ctypes.CDLL(build.build_lib())
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.declared_symbols()
    for cls, base in ((capi.VGICPMapCore, capi.VGICPCore), (capi.NDTMapCore, capi.NDTCore)):
        assert issubclass(cls, base) and cls._prefix == base._prefix
        assert callable(getattr(cls, "target_from_map")) and callable(getattr(cls, "get_target_points"))
        # the calls live on the scan-to-map handle classes: the plain handle classes keep the surface whose in-flight guards
        # tests/test_gpu_streaming.py tabulates method by method
        assert not hasattr(base, "target_from_map") and not hasattr(base, "get_target_points")
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_voxelmap.hpp")).read()
    for k in ("vm_target_select_kernel", "vm_target_keys_kernel", "vm_target_gather_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, src), k
    host = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_incmap.inc.hpp")).read()
    body = host[host.index("int incmap_to_cloud("):]
    for k in ("vm_target_select_kernel<<<", "vm_target_keys_kernel<<<", "vm_target_gather_kernel<<<", "radix_sort_pairs("):
        assert k in body, k
    # the sort runs on the map's own scratch: the Engine-wide buffers may belong to a preparation on the second stream
    assert "&inc.tm_hist" in body and not re.search(r"e->(sort_keys|sort_idx|sort_hist|staging)\b", body)


def test_capi_passes_what_the_header_declares():
    """capi.py calls through ctypes without argtypes: record what the new methods hand to the library and hold it against the prototypes"""
    from fast_gicp_amd import capi
    for cls, prefix in ((capi.VGICPMapCore, "fvh_vgicp_"), (capi.NDTMapCore, "fvh_ndt_")):
        calls = []

        def fake(name, *args):
            calls.append((name, args))
            if name in ("target_from_map", "get_num_target_points"):
                args[-1]._obj.value = 3

        core = object.__new__(cls)
        core.h = None
        core._call = fake
        assert core.target_from_map() == 3 and core.target_from_map(min_points=True) == 3 and core.target_from_map(4) == 3
        pts = core.get_target_points()
        assert pts.shape == (3, 3) and pts.dtype == np.float32
        assert [c[0] for c in calls] == ["target_from_map"] * 3 + ["get_num_target_points", "get_target_points"]
        assert [c[1][0] for c in calls[:3]] == [1, 1, 4]
        for name, args in calls:
            if name == "get_num_target_points":
                continue
            proto = NEW[prefix + name][1:]
            assert len(args) == len(proto), (name, len(args), proto)
            for a, t in zip(args, proto):
                if t == "int":
                    assert isinstance(a, int) and not isinstance(a, bool), (name, t, a)
                else:
                    assert isinstance(a, ctypes.c_void_p) or type(a).__name__ == "CArgObject", (name, t, a)


def test_registration_hpp_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "tm.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'using V = FastVGICPCuda<PointXYZ, PointXYZ>;\n'
                   'using N = NDTCuda<PointXYZ, PointXYZ>;\n'
                   'int (V::*a)(int) = &V::targetCloudFromMap;\n'
                   'int (N::*b)(int) = &N::targetCloudFromMap;\n'
                   'int (*c)(fvh_vgicp*, int, int*) = &detail::MapCalls<fvh_vgicp>::target_from_map;\n'
                   'int (*d)(fvh_ndt*, int, int*) = &detail::MapCalls<fvh_ndt>::target_from_map;\n'
                   'int main() { return (a && b && c && d) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def test_pygicp_exposes_target_cloud_from_map():
    from fast_gicp_amd import build_host
    build_host.build_all()
    import pygicp
    for cls in (pygicp.FastVGICPCuda, pygicp.NDTCudaMap):
        assert "target_cloud_from_map" in dir(cls), cls
    assert "target_cloud_from_map" not in dir(pygicp.NDTCuda)


def test_reference_orders_as_the_packed_key():
    rng = np.random.default_rng(3)
    lim = S.COORD_LIMIT - 1
    far = np.array([[-lim, -lim, -lim], [lim, lim, lim], [lim, -lim, 0], [-lim, lim, 0], [0, 0, -lim], [0, 0, lim], [-1, -1, -1], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],
                    [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.int64)
    coords = np.unique(np.concatenate([far, rng.integers(-lim, lim + 1, (500, 3)), rng.integers(-3, 4, (200, 3))]), axis=0).astype(np.int32)
    coords = coords[rng.permutation(len(coords))]
    counts = rng.integers(1, 5, len(coords)).astype(np.int32)
    means = rng.normal(size=(len(coords), 3)).astype(np.float32)
    covs = rng.normal(size=(len(coords), 3, 3)).astype(np.float32)
    keys = table_sim.pack_key(coords)
    assert len(np.unique(keys)) == len(keys)
    for mp in (0, 1, 2, 4, 5):
        rows, pts, cov = TM.expected_rows(coords, counts, means, covs, mp)
        want = np.argsort(keys, kind="stable")
        want = want[counts[want] >= max(mp, 1)]
        assert np.array_equal(rows, want), mp
        assert all(int(keys[rows[i]]) < int(keys[rows[i + 1]]) for i in range(len(rows) - 1))
        assert TM.same_bits(pts, means[want]) and TM.same_bits(cov, covs[want])
        # z-major, then y, then x -- in plain tuples, negative coordinates included
        assert [tuple(c) for c in coords[rows][:, ::-1]] == sorted(tuple(c) for c in coords[rows][:, ::-1])
    assert len(TM.expected_rows(coords, counts, means, covs, 5)[0]) == 0
    rows, pts, cov = TM.from_voxelmap((coords, counts, means, covs), 2, with_cov=False)
    assert cov is None and np.array_equal(counts[rows] >= 2, np.ones(len(rows), bool))
