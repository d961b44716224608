"""CPU tests of the posed map merge's boundary (no GPU): header / library / ctypes / C++ / pygicp agree on fvh_*_posed_merge_from /
fvh_*_transform_map, the numpy statement of the contract (tests/posedmerge_ref.py) is self-consistent, and the inputs the GPU tests use keep
every transformed mean off the voxel faces."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mapsnap_ref as S
from tests import posedmerge_ref as P
from tests import util

NEW = {
    "fvh_vgicp_posed_merge_from": ["fvh_vgicp*", "fvh_vgicp*", "const double*", "int*"],
    "fvh_ndt_posed_merge_from": ["fvh_ndt*", "fvh_ndt*", "const double*", "int*"],
    "fvh_vgicp_transform_map": ["fvh_vgicp*", "const double*", "int*"],
    "fvh_ndt_transform_map": ["fvh_ndt*", "const double*", "int*"],
}


def _prototypes():
    hdr = open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fvh_(?:vgicp|ndt)_(?:posed_merge_from|transform_map))\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in args.split(",")]
    return out


def _random_snapshot(rng, n, mode, num_inserts=4, res=1.0):
    coords = np.unique(rng.integers(-40, 40, (n, 3)).astype(np.int32), axis=0)
    coords = coords[S.key_order(coords)]
    n = len(coords)
    cnt = rng.integers(1, 30, n).astype(np.float64)
    mean = (coords + 1.0) * res + rng.uniform(-0.3, 0.3, (n, 3)) * res
    A = rng.normal(size=(n, 3, 3)) * 0.2
    C = A @ np.transpose(A, (0, 2, 1)) + 0.01 * np.eye(3)
    if mode == 3:
        C = cnt[:, None, None] * (C + mean[:, :, None] * mean[:, None, :])
        first = cnt[:, None] * mean
    elif mode == 2:
        C = cnt[:, None, None] * np.linalg.inv(C)
        first = np.einsum("nij,nj->ni", C, mean)
    else:
        C = cnt[:, None, None] * C
        first = cnt[:, None] * mean
    sums = np.concatenate([first, np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=1), cnt[:, None]], axis=1)
    return dict(resolution=res, mode=mode, num_inserts=num_inserts, num_points=int(cnt.sum()), num_voxels=n, coords=coords, sums=sums, ages=rng.integers(0, num_inserts, n).astype(np.uint32))


def test_header_declares_the_four_calls_and_the_library_exports_them():
    from fast_gicp_amd import build, capi
    assert _prototypes() == NEW, _prototypes()  # pointers only: no struct crosses the boundary
    lib = ctypes.CDLL(build.build_lib())
    for name in NEW:
        assert hasattr(lib, name) and name in capi.declared_symbols(), name
    for cls in (capi.VGICPMapCore, capi.NDTMapCore):
        for m in ("map_merge_from_posed", "map_transform"):
            assert callable(getattr(cls, m)), (cls, m)
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "kernels_voxelmap.hpp")).read()
    assert re.search(r"__global__[^;{]*\bvm_import_posed_kernel\b", src)
    host = open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "host_incmap.inc.hpp")).read()
    assert "vm_import_posed_kernel<M><<<" in host and "deskew_rigid(" not in host  # the pose rule is the deskew's, asked where the entry points live
    assert open(os.path.join(util.ROOT, "fast_gicp_amd", "csrc", "fvh_capi.hip")).read().count("deskew_rigid(") == 1


def test_capi_passes_what_the_header_declares():
    from fast_gicp_amd import capi
    calls = []
    core, other = object.__new__(capi.VGICPMapCore), object.__new__(capi.VGICPMapCore)
    core.h, other.h = None, ctypes.c_void_p(4096)
    core._call = lambda name, *args: calls.append((name, args))
    T = P.GENERAL
    assert core.map_merge_from_posed(other, T) == 0 and core.map_transform(T) == 0
    other.h = None
    assert [c[0] for c in calls] == ["posed_merge_from", "transform_map"]
    for name, args in calls:
        proto = NEW["fvh_vgicp_" + name][1:]
        assert len(args) == len(proto), (name, args)
        assert all(isinstance(a, ctypes.c_void_p) or type(a).__name__ == "CArgObject" for a in args), (name, args)
    assert calls[0][1][0].value == 4096


def test_registration_hpp_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "posed.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'using V = FastVGICPCuda<PointXYZ, PointXYZ>;\n'
                   'using N = NDTCuda<PointXYZ, PointXYZ>;\n'
                   'int (V::*a)(V&, const Isometry3d&) = &V::mergeTargetFromPosed;\n'
                   'int (V::*b)(const Isometry3d&) = &V::transformTargetMap;\n'
                   'int (N::*c)(N&, const Isometry3d&) = &N::mergeTargetFromPosed;\n'
                   'int (N::*d)(const Isometry3d&) = &N::transformTargetMap;\n'
                   'void (V::*e)(V&) = &V::mergeTargetFrom;\n'
                   'int main() { return (a && b && c && d && e) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def test_pygicp_binds_the_new_methods():
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "python", "pygicp.cpp")).read()
    assert src.count('"merge_target_from_posed"') >= 1 and src.count('"transform_target_map"') >= 1


@pytest.mark.parametrize("mode", [0, 3, 2])
def test_identity_pose_is_the_plain_merge(mode):
    rng = np.random.default_rng(5 + mode)
    dst, inc = _random_snapshot(rng, 400, mode, 6), _random_snapshot(rng, 300, mode, 3)
    got, info = P.posed_merge(dst, inc, P.IDENTITY)
    assert S.same(got, S.merge(dst, inc))
    assert info["rows_skipped"] == 0 and info["landed"].sum() == inc["num_voxels"] and info["landed"].max() == 1


@pytest.mark.parametrize("mode", [0, 3])
def test_whole_voxel_translations_compose_exactly(mode):
    """t of whole voxels and R = I: every product is exact, n t and the sums' increments are whole multiples that fp64 holds exactly at this
    size, so two translations in a row equal their sum to the bit"""
    rng = np.random.default_rng(9)
    inc = _random_snapshot(rng, 300, mode)
    inc["sums"] = np.round(inc["sums"] * 1024.0) / 1024.0  # sums on a 2^-10 grid: the integer-shifted sums stay exactly representable
    empty = S.empty_snapshot(1.0, mode)
    a, b = P.pose(np.eye(3), [3.0, -2.0, 5.0]), P.pose(np.eye(3), [-7.0, 4.0, 1.0])
    one, _ = P.posed_merge(empty, inc, a)
    two, _ = P.posed_merge(empty, one, b)
    direct, _ = P.posed_merge(empty, inc, b @ a)
    assert S.same(two, direct)
    assert np.array_equal(direct["coords"], (inc["coords"] + np.array([-4, 2, 6])).astype(np.int32)[S.key_order(inc["coords"] + np.array([-4, 2, 6]))])


@pytest.mark.parametrize("mode", [0, 3, 2])
@pytest.mark.parametrize("T", [P.EXACT, P.GENERAL, P.DIAGONAL], ids=["exact", "general", "diagonal"])
def test_counts_are_conserved_exactly(mode, T):
    rng = np.random.default_rng(3)
    dst, inc = _random_snapshot(rng, 200, mode), _random_snapshot(rng, 500, mode)
    got, info = P.posed_merge(dst, inc, T)
    assert got["sums"][:, 9].sum() == dst["sums"][:, 9].sum() + inc["sums"][:, 9].sum() and info["rows_skipped"] == 0
    assert got["num_points"] == dst["num_points"] + inc["num_points"] and got["num_inserts"] == max(dst["num_inserts"], inc["num_inserts"])
    if mode != 2:  # first moments: sum p' = R sum p + n t (the multiplicative b is not a first moment)
        R, t = T[:3, :3], T[:3, 3]
        want = dst["sums"][:, :3].sum(axis=0) + inc["sums"][:, :3].sum(axis=0) @ R.T + inc["sums"][:, 9].sum() * t
        assert np.allclose(got["sums"][:, :3].sum(axis=0), want, rtol=1e-12, atol=1e-9)
    # the NDT covariance recomputed from S' is R C R^T
    if mode == 3:
        coords, sums, _, _, _, _ = P.transform_rows(inc, T)
        n = inc["sums"][:, 9]

        def cov(s):
            m = s[:, :3] / s[:, 9:10]
            return S._full(s[:, 3:9]) / s[:, 9, None, None] - m[:, :, None] * m[:, None, :]

        assert np.allclose(cov(sums), T[:3, :3] @ cov(inc["sums"]) @ T[:3, :3].T, atol=1e-9 * (1.0 + np.abs(sums[:, 3:9] / n[:, None]).max()))


def test_far_translation_skips_every_row():
    inc = _random_snapshot(np.random.default_rng(1), 100, 0)
    dst = _random_snapshot(np.random.default_rng(2), 50, 0)
    got, info = P.posed_merge(dst, inc, P.FAR)
    assert info["rows_skipped"] == inc["num_voxels"] and info["skipped_points"] == int(inc["sums"][:, 9].sum())
    assert np.array_equal(got["coords"], dst["coords"]) and np.array_equal(got["sums"], dst["sums"]) and got["num_points"] == dst["num_points"] + inc["num_points"]


def test_the_lattice_collides_under_45_degrees():
    for mode in (0, 3):
        inc = P.numpy_map(P.lattice_cloud(), None, mode)
        assert inc["num_voxels"] == len(P.lattice_cloud()) and np.all(inc["sums"][:, 9] == 1.0)
        got, info = P.posed_merge(S.empty_snapshot(P.RES, mode), inc, P.DIAGONAL)
        shared = (info["landed"] >= 2).mean()
        print("lattice under 45 degrees, mode %d: %d rows -> %d voxels, %.1f %% of them received two or more rows" % (mode, inc["num_voxels"], got["num_voxels"], 100 * shared))
        assert shared >= 0.10


@pytest.mark.parametrize("kind", list(P.KINDS))
def test_no_gpu_test_input_sits_on_a_voxel_face(kind):
    """the input guard: with TWICE the guard near_face flags no row of any map a GPU test sends through a general pose"""
    mode = P.KINDS[kind]
    for name, cloud, cov, T_in, T in P.guarded_cases():
        snap = P.numpy_map(cloud, cov, mode, T_in)
        near = P.transform_rows(snap, T, guard=2.0)[5]
        print("%s, %s: %d rows, %d near a face at twice the guard" % (kind, name, snap["num_voxels"], int(near.sum())))
        assert not near.any(), (kind, name, np.flatnonzero(near))
    # the age test's `other`: three inserts into one map
    other = S.empty_snapshot(P.RES, mode)
    for seed in P.AGE_SEEDS:
        other = S.merge(other, P.numpy_map(P.voxel_cloud(300, seed), None, mode))
    assert not P.transform_rows(other, P.GENERAL, guard=2.0)[5].any()
    # map_transform after a general merge transforms the MERGED map: its rows too
    b = P.bundled()
    merged, _ = P.posed_merge(P.numpy_map(b["tgt"], b["Ct"], mode), P.numpy_map(b["src"], b["Cs"], mode), P.GENERAL)
    assert not P.transform_rows(merged, P.SECOND, guard=2.0)[5].any()
