"""CPU tests of the map snapshot boundary (no GPU): header / library / ctypes / C++ / pygicp agree on fvh_vgicp_voxelmap_export / _import /
_merge_from, the file format round-trips, and the numpy statement of the contract (tests/mapsnap_ref.py) is self-consistent."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mapsnap_ref as S
from tests import util

NEW = {
    "fvh_vgicp_voxelmap_export": ["fvh_vgicp*", "int*", "double*", "int*", "int*", "long long*", "int*", "double*", "unsigned*"],
    "fvh_vgicp_voxelmap_import": ["fvh_vgicp*", "int", "const int*", "const double*", "const unsigned*", "double", "int", "int", "long long"],
    "fvh_vgicp_voxelmap_merge_from": ["fvh_vgicp*", "fvh_vgicp*"],
}


def _prototypes():
    hdr = open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fvh_vgicp_voxelmap_\w+)\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in args.split(",")]
    return out


def _random_snapshot(rng, n, mode=0, num_inserts=4):
    coords = np.unique(rng.integers(-300, 300, (n, 3)).astype(np.int32), axis=0)
    coords = coords[S.key_order(coords)]
    n = len(coords)
    sums = rng.normal(size=(n, 10)) * 100.0
    sums[:, 9] = rng.integers(1, 50, n)
    return dict(resolution=0.5, mode=mode, num_inserts=num_inserts, num_points=int(sums[:, 9].sum()) + 3, num_voxels=n, coords=coords, sums=sums,
                ages=rng.integers(0, num_inserts, n).astype(np.uint32))


def test_header_declares_the_snapshot_calls_with_plain_signatures():
    assert _prototypes() == NEW, _prototypes()  # pointers and scalars only: no struct crosses the boundary


def test_library_exports_the_calls_and_holds_the_kernels():
    from fast_gicp_amd import build, capi
    lib = ctypes.CDLL(build.build_lib())
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.declared_symbols()
    for m in ("map_export", "map_import", "map_merge_from", "map_save", "map_load"):
        assert callable(getattr(capi.VGICPCore, m)), m
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_voxelmap.hpp")).read()
    for k in ("vm_import_kernel", "vm_export_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, src), k
    # merge_from is the second instantiation of the import kernel: both are launched by the host section
    host = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_incmap.inc.hpp")).read()
    assert "vm_import_kernel<FROM_MAP>" in host and "incmap_add_rows<true>" in host and "incmap_add_rows<false>" in host and "vm_export_kernel<<<" in host


def test_capi_passes_what_the_header_declares():
    """capi.py calls through ctypes without argtypes: record what the snapshot methods hand to the library and hold it against the prototypes"""
    from fast_gicp_amd import capi
    calls = []

    def fake(name, *args):
        calls.append((name, args))
        if name == "voxelmap_export":
            args[0]._obj.value = 3  # num_voxels: the second call then passes the arrays

    core, other = object.__new__(capi.VGICPCore), object.__new__(capi.VGICPCore)
    core.h, other.h = None, ctypes.c_void_p(4096)
    core._call = fake
    snap = _random_snapshot(np.random.default_rng(0), 5)
    core.map_export(); core.map_import(snap); core.map_merge_from(other)
    core.map_import(dict(snap, ages=None))  # no ages: zeros are passed (the C call also takes NULL)
    other.h = None
    assert [c[0] for c in calls] == ["voxelmap_export", "voxelmap_export", "voxelmap_import", "voxelmap_merge_from", "voxelmap_import"]
    for name, args in calls:
        proto = NEW["fvh_vgicp_" + name][1:]
        assert len(args) == len(proto), (name, len(args), proto)
        for a, t in zip(args, proto):
            if t == "double":
                assert isinstance(a, ctypes.c_double), (name, t, a)
            elif t == "long long":
                assert isinstance(a, ctypes.c_longlong), (name, t, a)
            elif t == "int":
                assert isinstance(a, int) and not isinstance(a, bool), (name, t, a)
            else:
                assert a is None or isinstance(a, ctypes.c_void_p) or type(a).__name__ == "CArgObject", (name, t, a)
    assert calls[0][1][5:] == (None, None, None) and all(a is not None for a in calls[1][1][5:])  # header query first, then the rows
    imp = calls[2][1]
    assert imp[0] == len(snap["coords"]) and imp[4].value == 0.5 and imp[5] == 0 and imp[6] == 4 and imp[7].value == snap["num_points"]
    assert calls[3][1][0].value == 4096


def test_registration_hpp_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "snap.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'using V = FastVGICPCuda<PointXYZ, PointXYZ>;\n'
                   'TargetMapSnapshot (V::*a)() = &V::exportTargetMap;\n'
                   'void (V::*b)(const TargetMapSnapshot&) = &V::importTargetMap;\n'
                   'void (V::*c)(V&) = &V::mergeTargetFrom;\n'
                   'void (V::*d)(const std::string&) = &V::saveTargetMap;\n'
                   'void (V::*e)(const std::string&) = &V::loadTargetMap;\n'
                   'int main() { TargetMapSnapshot s; s.coords = {1, 2, 3}; s.sums.assign(10, 1.0); s.ages = {0u}; return (a && b && c && d && e && s.num_voxels() == 1) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def test_cpp_and_python_write_the_same_file(tmp_path):
    """the file functions of registration.hpp need no GPU either: a host-only program reads the Python file and writes it back, byte for byte"""
    from fast_gicp_amd import capi
    src = tmp_path / "copy.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'int main(int argc, char** argv) {\n'
                   '  try { fast_gicp::detail::write_map_file(argv[2], fast_gicp::detail::read_map_file(argv[1])); } catch (const std::exception& e) { std::fprintf(stderr, "%s\\n", e.what()); return 3; }\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "copy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src), "-o", str(exe)])
    snap = _random_snapshot(np.random.default_rng(5), 40, mode=2)
    a, b = tmp_path / "a.fvhmap", tmp_path / "b.fvhmap"
    capi.write_map_file(str(a), snap)
    subprocess.check_call([str(exe), str(a), str(b)])
    assert a.read_bytes() == b.read_bytes()
    a.write_bytes(a.read_bytes()[:-1])
    assert subprocess.call([str(exe), str(a), str(b)], stderr=subprocess.DEVNULL) == 3  # truncated: refused by the C++ reader too


def test_pygicp_exposes_the_snapshot_methods():
    from fast_gicp_amd import build_host
    build_host.build_all()
    import pygicp
    new = {"export_target_map", "import_target_map", "merge_target_from", "save_target_map", "load_target_map"}
    assert new <= set(dir(pygicp.FastVGICPCuda))
    assert not (new & set(dir(pygicp.NDTCuda)))


def test_map_file_round_trips_and_rejects_what_is_not_one(tmp_path):
    from fast_gicp_amd import capi
    rng = np.random.default_rng(11)
    for n, mode in ((200, 0), (1, 2), (0, 0)):
        snap = _random_snapshot(rng, n, mode) if n else S.empty_snapshot(0.25, mode)
        snap["num_points"] = (1 << 40) + 7  # (past 32 bits)
        p = str(tmp_path / ("m%d.fvhmap" % n))
        capi.write_map_file(p, snap)
        assert os.path.getsize(p) == 40 + 96 * snap["num_voxels"]
        back = capi.read_map_file(p)
        assert S.same(back, snap), n
        q = str(tmp_path / "again.fvhmap")
        capi.write_map_file(q, back)
        assert open(p, "rb").read() == open(q, "rb").read()
    raw = open(str(tmp_path / "m200.fvhmap"), "rb").read()
    assert raw[:8] == b"FVHVMAP\0" and raw[8:12] == (1).to_bytes(4, "little")
    bad = str(tmp_path / "bad.fvhmap")
    for data in (raw[:-1], raw[:39], raw[:40], raw + b"\0", b"FVHVMAQ\0" + raw[8:], raw[:8] + (2).to_bytes(4, "little") + raw[12:], b""):
        open(bad, "wb").write(data)
        with pytest.raises(capi.FvhError):
            capi.read_map_file(bad)


def test_contract_in_numpy_is_self_consistent():
    rng = np.random.default_rng(7)
    c = np.array([[0, 0, 1], [5, 0, 0], [0, 1, 0], [-3, 0, 0], [0, 0, -1]], np.int32)
    assert list(S.key_order(c)) == [4, 3, 1, 2, 0]  # z-major, then y, then x
    a, b = _random_snapshot(rng, 300), _random_snapshot(rng, 300)
    b["coords"][:50] = a["coords"][:50]  # shared voxels
    keep = np.unique(S.packed_key(b["coords"]), return_index=True)[1]
    b = dict(b, coords=b["coords"][keep], sums=b["sums"][keep], ages=b["ages"][keep], num_voxels=len(keep))
    ab, ba = S.merge(a, b), S.merge(b, a)
    assert S.same(ab, ba)  # commutative: equal insert counts, so also in the ages
    assert np.all(np.diff(S.packed_key(ab["coords"]).astype(np.int64)) > 0)
    shared = np.isin(S.packed_key(ab["coords"]), np.intersect1d(S.packed_key(a["coords"]), S.packed_key(b["coords"])))
    assert shared.sum() >= 50 and ab["num_voxels"] == a["num_voxels"] + b["num_voxels"] - shared.sum()
    ia = {k: i for i, k in enumerate(S.packed_key(a["coords"]))}
    ib = {k: i for i, k in enumerate(S.packed_key(b["coords"]))}
    for r, k in enumerate(S.packed_key(ab["coords"])):
        rows = [m["sums"][i[k]] for m, i in ((a, ia), (b, ib)) if k in i]
        ages = [m["ages"][i[k]] for m, i in ((a, ia), (b, ib)) if k in i]
        assert np.array_equal(ab["sums"][r], rows[0] + rows[1] if len(rows) == 2 else rows[0]) and ab["ages"][r] == min(ages)
    # different insert counts: keys, sums and header still commute; the ages of the map with fewer inserts count from the merged insert number
    b7 = dict(b, num_inserts=7)
    x, y = S.merge(a, b7), S.merge(b7, a)
    assert all(np.array_equal(x[k], y[k]) for k in ("coords", "sums")) and x["num_inserts"] == y["num_inserts"] == 7 and x["num_points"] == y["num_points"]
    only_a = ~np.isin(S.packed_key(x["coords"]), S.packed_key(b["coords"]))
    assert np.array_equal(x["ages"][only_a], a["ages"][np.isin(S.packed_key(a["coords"]), S.packed_key(x["coords"])[only_a])] + 3)
    # the empty snapshot is the identity, on either side
    e = S.empty_snapshot(a["resolution"], a["mode"])
    assert S.same(S.merge(e, a), a) and S.same(S.merge(a, e), a)
    # additive records: 2s * 1/(2n) is exact -- a map imported twice has the records of the original
    n0, m0, c0 = S.additive_records(a["sums"])
    n2, m2, c2 = S.additive_records(2.0 * a["sums"])
    assert np.array_equal(n2, 2 * n0) and np.array_equal(m2, m0) and np.array_equal(c2, c0) and np.array_equal(c0, np.transpose(c0, (0, 2, 1)))
