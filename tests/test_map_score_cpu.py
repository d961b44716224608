"""Scoring a scan against the voxel map, without a GPU: tests/mapscore_ref.py (the twin the GPU tests hold the kernel to) is itself held to a
second formulation (numpy.linalg.inv) and to its tie, singular-record and skip rules on hand-made records; the scenes the GPU tests run are
shown to exercise every rule under the twin alone; header, library, ctypes mirror, wrapper, C++ and pygicp agree on the four entry points."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mapscore_ref as M
from tests import util

ARGS_SOURCE = ["const double*", "int", "int", "double", "double", "fvh_map_score*", "int*", "int*", "double*"]
ARGS_CLOUD = ["const float*", "int", "int", "int"] + ARGS_SOURCE
NEW = {"fvh_%s_score_%s" % (k, f): ["fvh_%s*" % k] + (ARGS_SOURCE if f == "source" else ARGS_CLOUD) for k in ("vgicp", "ndt") for f in ("source", "cloud")}
FIELDS = [("int", "n_points"), ("int", "n_used"), ("int", "n_in_voxel"), ("int", "n_near"), ("int", "n_explained"), ("double", "sum_best_m2"), ("double", "sum_score_max"),
          ("double", "sum_score_all")]


def _header():
    return open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()


def _prototypes():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fvh_(?:vgicp|ndt)_score_(?:source|cloud))\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in args.split(",")]
    return out


def _spd(rng, n):
    A = rng.normal(size=(n, 3, 3))
    return (A @ np.transpose(A, (0, 2, 1)) * 0.05 + 0.02 * np.eye(3)).astype(np.float32)  # eigenvalues within [0.02, ~1]: well conditioned


def test_the_twin_against_an_inverse_on_well_conditioned_records():
    rng = np.random.default_rng(3)
    covs = _spd(rng, 300)
    d = rng.uniform(-1.5, 1.5, (300, 3))
    for v, C in zip(d, covs):
        C64 = C.astype(np.float64)
        got = M.mahalanobis2(tuple(float(x) for x in v), (float(C[0, 0]), float(C[0, 1]), float(C[0, 2]), float(C[1, 1]), float(C[1, 2]), float(C[2, 2])))
        want = float(v @ np.linalg.inv(C64) @ v)
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    # and through score(): one voxel, points around its mean
    rec = M.records_of([[0, 0, 0]], [5], [[1.0, 1.0, 1.0]], covs[:1])
    pts = (1.0 + rng.uniform(-0.4, 0.4, (50, 3))).astype(np.float32)
    r = M.score(rec, 1.0, pts, None, M.DIRECT1, 1, M.INF, 1.0)
    Ci = np.linalg.inv(covs[0].astype(np.float64))
    for p, m2, f, b in zip(pts.astype(np.float64), r["best_m2"], r["found"], r["best"]):
        want = float((p - 1.0) @ Ci @ (p - 1.0))
        assert (f, b) == (1, 0) and abs(m2 - want) <= 1e-9 * want
    assert r["n_used"] == r["n_in_voxel"] == r["n_near"] == r["n_explained"] == 50
    assert abs(r["sum_score_max"] - sum(math.exp(-0.5 * m) for m in r["best_m2"])) < 1e-12 and r["sum_score_all"] == r["sum_score_max"]


def test_tie_singular_and_skip_rules_on_hand_made_records():
    C = np.diag([0.25, 0.25, 0.25]).astype(np.float32)
    flat = np.diag([0.25, 0.25, 0.0]).astype(np.float32)
    nan = np.full((3, 3), np.nan, np.float32)
    neg = np.diag([0.25, -0.25, 0.25]).astype(np.float32)
    # voxels 0 and 2 on the x axis with means one cell either side of the centre of cell 1; cell 1 is empty
    rec = M.records_of([[0, 0, 0], [2, 0, 0], [5, 0, 0], [7, 0, 0], [9, 0, 0]], [4, 4, 2, 2, 2], [[1, 1, 1], [3, 1, 1], [6, 1, 1], [8, 1, 1], [10, 1, 1]], [C, C, flat, nan, neg])
    p = np.array([[2, 1, 1]], np.float32)
    r = M.score(rec, 1.0, p, None, M.DIRECT7, 1, M.INF, 1.0)
    assert (r["found"][0], r["best"][0], r["best_m2"][0], r["ties"]) == (2, 1, 4.0, 1)  # +x (index 1) before -x (index 2)
    r = M.score(rec, 1.0, p, None, M.DIRECT27, 1, M.INF, 1.0)
    assert (r["found"][0], r["best"][0], r["best_m2"][0]) == (2, 4, 4.0)               # (-1, 0, 0) is index 4, (1, 0, 0) index 22
    assert r["terms"][0].tolist() == [4.0, math.exp(-2.0), math.exp(-2.0) + math.exp(-2.0)]
    r = M.score(rec, 1.0, p, None, M.DIRECT1, 1, M.INF, 1.0)
    assert (r["found"][0], r["best"][0], r["best_m2"][0], r["n_near"], r["n_used"]) == (0, -1, M.INF, 0, 1)
    assert M.score(rec, 1.0, p, None, M.DIRECT7, 5, M.INF, 1.0)["found"][0] == 0      # min_points above both counts
    assert M.score(rec, 1.0, p, None, M.DIRECT7, 1, 3.9, 1.0)["n_explained"] == 0      # 4.0 > max_m2
    assert M.score(rec, 1.0, p, None, M.DIRECT7, 1, 4.0, 1.0)["n_explained"] == 1      # the bound is inclusive
    assert M.score(rec, 1.0, p, None, M.DIRECT7, 1, M.INF, 0.5)["terms"][0, 1] == math.exp(-1.0)
    # singular, non-finite and indefinite records: found, +inf, score 0, never explained -- not even with max_m2 = +inf
    for x in (6, 8, 10):
        r = M.score(rec, 1.0, np.array([[x, 1.25, 1]], np.float32), None, M.DIRECT1, 1, M.INF, 1.0)
        assert (r["found"][0], r["best"][0], r["best_m2"][0], r["n_near"], r["n_explained"], r["singular_hits"]) == (1, 0, M.INF, 1, 0, 1)
        assert r["terms"][0].tolist() == [0.0, 0.0, 0.0]
    # a regular voxel beats a singular neighbour whatever the order; two singular candidates: the first stays
    rec2 = M.records_of([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [1, 1, 1], [[1, 1, 1], [2, 1, 1], [3, 1, 1]], [flat, C, flat])
    r = M.score(rec2, 1.0, np.array([[2, 1, 1], [9, 9, 9]], np.float32), None, M.DIRECT7, 1, M.INF, 1.0)
    assert (r["found"][0], r["best"][0], r["best_m2"][0]) == (3, 0, 0.0) and r["found"][1] == 0
    rec3 = M.records_of([[0, 0, 0], [2, 0, 0]], [1, 1], [[1, 1, 1], [3, 1, 1]], [flat, flat])
    r = M.score(rec3, 1.0, np.array([[2, 1, 1]], np.float32), None, M.DIRECT7, 1, M.INF, 1.0)
    assert (r["found"][0], r["best"][0], r["best_m2"][0], r["ties"]) == (2, 1, M.INF, 0)
    # skips: non-finite coordinates, a cell at the index limit; the last cell inside it is used
    lim = float((1 << 20) - 4096)
    pts = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [lim + 1.0, 1, 1], [lim, 1, 1], [3e38, 1, 1]], np.float32)
    r = M.score(rec, 1.0, pts, None, M.DIRECT27, 1, M.INF, 1.0)
    assert r["found"].tolist() == [-1, -1, -1, -1, 0, -1] and r["best"].tolist() == [-1] * 6
    assert np.isnan(r["best_m2"][[0, 1, 2, 3, 5]]).all() and r["best_m2"][4] == M.INF and (r["n_points"], r["n_used"]) == (6, 1)
    assert M.score(rec, 1.0, np.zeros((0, 3), np.float32))["n_points"] == 0
    # a negative quotient cannot come from a positive definite record, but the rule is there: 0
    assert M.mahalanobis2((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0, 0.0, 1.0)) == 0.0


SCENES = [(res, n, seed) for res in (1.0, 0.5) for n, seed in ((63, 1), (64, 2), (65, 3), (257, 4), (1000, 5))]


@pytest.mark.parametrize("res,n,seed", SCENES)
def test_the_gpu_scenes_exercise_every_rule_under_the_twin(res, n, seed):
    sc = M.plane_scene(res, n, seed)
    assert sc["scan"].shape == (n, 3) and M.rounding_is_stable(sc["pose"], sc["scan"])
    R, t = M.pose_parts(sc["pose"])
    for p, q in zip(sc["scan"], sc["targets"]):  # every product and sum of R p + t is exact: p' is the intended point
        if np.all(np.isfinite(p)):
            assert M.transform_point(R, t, [float(v) for v in p]) == tuple(float(v) for v in q)
    for kind in ("additive", "multiplicative", "ndt"):
        rec = M.model_records(kind, res, sc["map_points"], sc["map_covs"])
        assert len(rec) == 64 + 32 + 4
        for nb in (M.DIRECT7, M.DIRECT27):
            for mp in (1, 3):
                r = M.score(rec, res, sc["scan"], sc["pose"], nb, mp, 16.0, 1.0)
                what = (kind, nb, mp, {k: r[k] for k in ("n_points", "n_used", "n_in_voxel", "n_near", "n_explained", "ties", "singular_hits")})
                assert 0 < r["n_in_voxel"] < r["n_near"] < r["n_used"] < r["n_points"], what
                assert 0 < r["n_explained"] < r["n_near"], what
                assert r["ties"] >= 1 and (r["singular_hits"] >= 1 or kind == "ndt"), what  # (the device's MIN_EIG regularisation leaves an NDT map no singular record)
                assert r["best"][1] == (1 if nb == M.DIRECT7 else 4) and r["found"][1] == 2, what  # row 1 is the hand-made tie
                assert r["found"][9:12].tolist() == [-1, -1, -1] and r["found"][6] == 0, what
        r1 = M.score(rec, res, sc["scan"], sc["pose"], M.DIRECT1, 1, 16.0, 1.0)  # one candidate at most: in-voxel and near are the same thing
        assert 0 < r1["n_in_voxel"] == r1["n_near"] < r1["n_used"] and r1["ties"] == 0 and (r1["singular_hits"] >= 1 or kind == "ndt")


@pytest.mark.parametrize("capacity", [64, 1024])
def test_the_wrap_scene_makes_probe_sequences_cross_the_end_of_the_table(capacity):
    from tests import table_sim
    w = M.wrap_scene(capacity)
    st = w["stats"]
    assert st["wraps"] and st["across_end"] >= 3 and st["displaced"] >= 4 and st["max_displacement"] >= 3, st
    home = table_sim.hash_slot(table_sim.pack_key(np.concatenate([w["voxels"][:4], w["absent"][None]])), capacity)
    assert home.tolist() == [capacity - 1] * 5  # four voxels and the empty cell start their probes in the last slot
    assert not any((w["voxels"] == w["absent"]).all(axis=1))
    rec = M.model_records("additive", 1.0, w["map_points"], w["map_covs"])
    r = M.score(rec, 1.0, w["scan"], None, M.DIRECT1, 1, 16.0, 1.0)
    assert r["found"].tolist() == [1] * 36 + [0, 0]
    assert M.score(rec, 1.0, w["scan"], None, M.DIRECT27, 1, 16.0, 1.0)["found"].tolist() == [1] * 36 + [0, 0]  # (cells three apart: no neighbours)


def test_sum_bounds_are_the_any_order_bound():
    terms = np.array([[1.0, 0.5, 2.0], [3.0, 0.25, 0.0], [0.0, 0.0, 1.0]])
    b = M.sum_bounds(terms)
    assert b == [3 * 2.0 ** -53 * 4.0, 11 * 2.0 ** -53 * 0.75, 11 * 2.0 ** -53 * 3.0]


def test_header_declares_the_four_calls_and_the_library_exports_them():
    from fast_gicp_amd import build, capi
    assert _prototypes() == NEW, _prototypes()
    lib = ctypes.CDLL(build.build_lib())
    for name in NEW:
        assert hasattr(lib, name) and name in capi.declared_symbols(), name
        assert not re.match(r"fvh_vgicp_(map|voxelmap)_\w+", name)
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        z, d = ctypes.c_void_p(None), ctypes.c_double(0.0)
        tail = (z, 0, 0, d, d, z, z, z, z)
        assert (fn(z, *tail) if name.endswith("source") else fn(z, z, 0, 0, 0, *tail)) == 1  # a null handle is refused before anything else
    for cls in (capi.VGICPMapCore, capi.NDTMapCore):
        assert callable(cls.map_score)
    for name in ("fvh_vgicp_get_num_source_points", "fvh_ndt_get_num_source_points"):  # what sizes the per-point rows of a source score
        assert hasattr(lib, name) and name in capi.declared_symbols(), name
    assert any(s.endswith(os.sep + "kernels_mapscore.hpp") for s in build.SOURCES)


def test_the_struct_mirror_matches_the_header_field_by_field(tmp_path):
    from fast_gicp_amd import capi
    hdr = _header()
    body = hdr[hdr.index("typedef struct fvh_map_score {"):hdr.index("} fvh_map_score;")]
    assert re.findall(r"^\s+(int|double)\s+(\w+);", body, flags=re.M) == FIELDS
    assert [(("int" if t is ctypes.c_int else "double" if t is ctypes.c_double else "?"), n) for n, t in capi.MapScore._fields_] == FIELDS
    src = tmp_path / "ms.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fast_vgicp_hip.h"\nint main(void) { printf("%zu", sizeof(fvh_map_score));\n'
                   + "".join('printf(" %%zu", offsetof(fvh_map_score, %s));\n' % n for _, n in FIELDS) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "ms"
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(exe), str(src)])
    vals = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert ctypes.sizeof(capi.MapScore) == vals[0] == 48
    assert [getattr(capi.MapScore, n).offset for _, n in FIELDS] == vals[1:]


class _Recorder:
    """stands in for _Core._call: keeps what the wrapper hands to the library and fills the struct as the library would"""

    def __init__(self, n_points, fill=True):
        self.calls, self.n_points, self.fill = [], n_points, fill

    def __call__(self, name, *args):
        if name == "get_num_source_points":  # (the rows of a per-point score of the source)
            args[0]._obj.value = self.n_points
            return
        self.calls.append((name, args))
        if not self.fill:
            return
        out = args[-4]._obj  # byref(MapScore)
        out.n_points, out.n_used, out.n_in_voxel, out.n_near, out.n_explained = self.n_points, 4, 1, 2, 1
        out.sum_best_m2, out.sum_score_max, out.sum_score_all = 3.0, 0.5, 1.0


def _ctype_ok(arg, proto):
    if proto == "int":
        return isinstance(arg, int) and not isinstance(arg, bool)
    if proto == "double":
        return isinstance(arg, ctypes.c_double)
    return arg is None or isinstance(arg, ctypes.c_void_p) or type(arg).__name__ == "CArgObject"  # a pointer


@pytest.mark.parametrize("cls_name,prefix", [("VGICPMapCore", "fvh_vgicp_"), ("NDTMapCore", "fvh_ndt_")])
def test_capi_passes_what_the_header_declares(cls_name, prefix):
    from fast_gicp_amd import capi
    protos = _prototypes()
    core = object.__new__(getattr(capi, cls_name))
    core.h = None
    rec = core._call = _Recorder(5)
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    r = core.map_score(np.eye(4), xyz=pts, neighbors=capi.DIRECT27, min_points=3, max_m2=9.0, score_scale=0.5, per_point=True)
    assert (r["overlap"], r["nvtl"], r["tp"]) == (0.25, 0.25, 0.25) and r["n_points"] == 5 and r["sum_best_m2"] == 3.0
    assert r["found"].shape == r["best"].shape == r["best_m2"].shape == (5,) and r["found"].dtype == np.int32 and r["best_m2"].dtype == np.float64
    core.map_score(device_ptr=4096, n=7, stride=4)
    core.map_score()                      # the source: no rows
    r = core.map_score(per_point=True)    # the source: rows sized by the handle's point count, one scoring call
    assert len(r["found"]) == len(r["best"]) == len(r["best_m2"]) == 5
    assert [c[0] for c in rec.calls] == ["score_cloud", "score_cloud", "score_source", "score_source"]
    for name, args in rec.calls:
        proto = protos[prefix + name][1:]
        assert len(args) == len(proto), (name, args)
        assert all(_ctype_ok(a, p) for a, p in zip(args, proto)), (name, args, proto)
    first, second = rec.calls[0][1], rec.calls[1][1]
    assert first[1:4] == (5, 3, 0) and first[5:7] == (capi.DIRECT27, 3) and (first[7].value, first[8].value) == (9.0, 0.5) and all(a is not None for a in first[-3:])
    assert (second[0].value, second[1:4]) == (4096, (7, 4, 1)) and second[-3:] == (None, None, None) and second[7].value == float("inf")
    assert rec.calls[2][1][-3:] == (None, None, None) and all(a is not None for a in rec.calls[3][1][-3:])
    rec.n_points = 0
    r = core.map_score(xyz=np.zeros((0, 3), np.float32), per_point=True)
    assert rec.calls[-1][1][0] is None and rec.calls[-1][1][-3:] == (None, None, None) and len(r["found"]) == 0
    core._call = _Recorder(0, fill=False)
    r = core.map_score(xyz=pts)
    assert all(math.isnan(r[k]) for k in ("overlap", "nvtl", "tp"))  # zero denominators


def test_registration_hpp_compiles_with_the_new_method(tmp_path):
    src = tmp_path / "score.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'template <class R> int use(R& r) { MapScore s = r.scoreTarget(Matrix4f::Identity(), NeighborSearchMethod::DIRECT27, 3, 9.0, 1.0, true);\n'
                   '  return s.n_points + (int)s.found.size() + (int)s.best.size() + (int)s.best_m2.size() + (int)(s.overlap() + s.nvtl() + s.tp() + s.sum_best_m2); }\n'
                   'template int use(FastVGICPCuda<PointXYZ, PointXYZ>&);\n'
                   'template int use(FastVGICP<PointXYZ, PointXYZ>&);\n'
                   'template int use(NDTCuda<PointXYZ, PointXYZ>&);\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def test_pygicp_binds_the_new_method():
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "python", "pygicp.cpp")).read()
    assert src.count('"score_target"') >= 1
