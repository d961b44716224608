"""Ray casting into the voxel map, without a GPU: tests/raycast_ref.py (the twin the GPU tests hold the kernel to) is itself held to a second
formulation (numpy.linalg.inv and a dense 1-D minimisation) and to its clamp, bound, singular-record, min_points, min_range and skip rules on
hand-made records; the scenes the GPU tests run are shown to exercise every rule under the twin alone; a dense analytic plane is hit at
sub-voxel range error; header, library, ctypes mirror, wrapper, C++ and pygicp agree on the four entry points."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import raycast_ref as RC
from tests import util

ARGS_SOURCE = ["const double*", "const double*", "double", "double", "int", "double", "fvh_ray_cast*", "int*", "int*", "double*", "double*"]
ARGS_CLOUD = ["const float*", "int", "int", "int"] + ARGS_SOURCE
NEW = {"fvh_%s_cast_rays_%s" % (k, f): ["fvh_%s*" % k] + (ARGS_SOURCE if f == "source" else ARGS_CLOUD) for k in ("vgicp", "ndt") for f in ("source", "cloud")}
FIELDS = [("int", "n_rays"), ("int", "n_used"), ("int", "n_hit"), ("int", "n_hit_at_origin"), ("long long", "n_cells")]
CTYPES = {ctypes.c_int: "int", ctypes.c_longlong: "long long"}


def _header():
    return open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read()


def _prototypes():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fvh_(?:vgicp|ndt)_cast_rays_(?:source|cloud))\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in args.split(",")]
    return out


def _c6(C):
    return (float(C[0, 0]), float(C[0, 1]), float(C[0, 2]), float(C[1, 1]), float(C[1, 2]), float(C[2, 2]))


def test_the_twin_against_an_inverse_and_a_dense_minimisation_on_well_conditioned_records():
    """m2(s) = (e + s d)^T C^-1 (e + s d) is a parabola with curvature d^T C^-1 d: a grid of K + 1 samples over [lo, hi] contains both ends, so
    its minimum is the constrained minimum when that is clamped, and exceeds it by at most curvature * (h / 2)^2 (h the spacing) when it is
    interior. The records have eigenvalues within [0.02, ~1], where the adjugate form agrees with an explicit inverse to 1e-9 relative
    (tests/test_map_score_cpu.py states the same bound for the same form)."""
    rng = np.random.default_rng(7)
    K = 4000
    seen = set()
    for _ in range(200):
        A = rng.normal(size=(3, 3))
        C = (A @ A.T * 0.05 + 0.02 * np.eye(3)).astype(np.float32)
        Ci = np.linalg.inv(C.astype(np.float64))
        e, d = rng.uniform(-1.5, 1.5, 3), rng.uniform(-2.0, 2.0, 3)
        lo, hi = sorted(rng.uniform(0.0, 1.0, 2))
        s, m2, what = RC.closest_approach(tuple(e), tuple(d), lo, hi, _c6(C))
        seen.add(what)
        grid = lo + (hi - lo) * np.arange(K + 1) / K
        x = e[None] + grid[:, None] * d[None]
        vals = np.einsum("ni,ij,nj->n", x, Ci, x)
        curv = float(d @ Ci @ d)
        h = (hi - lo) / K
        tol = 1e-9 * float(vals.min()) + 1e-12
        assert lo <= s <= hi and what != "singular"
        assert m2 <= vals.min() + tol, (m2, vals.min())
        assert vals.min() - m2 <= curv * (h / 2) ** 2 + tol, (m2, vals.min(), what)
        assert abs(grid[int(vals.argmin())] - s) <= h, (s, grid[int(vals.argmin())], what)
        xs = e + s * d
        assert abs(m2 - float(xs @ Ci @ xs)) <= 1e-9 * m2 + 1e-12
    assert seen == {"low", "high", "interior"}


# one voxel in cell (0, 0, 0) at res 1: it covers metric [0.5, 1.5) per axis, its mean is the centre (1, 1, 1), sigma = 0.5 per axis
ISO = np.diag([0.25, 0.25, 0.25]).astype(np.float32)
FLAT = np.diag([0.25, 0.25, 0.0]).astype(np.float32)


def _one(cov=ISO, num=4):
    return RC.records_of([[0, 0, 0]], [num], [[1.0, 1.0, 1.0]], [cov])


def _cast1(rec, o, p, **kw):
    r = RC.cast(rec, 1.0, np.array([p], np.float32), None, o, **kw)
    return int(r["hit"][0]), tuple(r["cell"][0].tolist()), float(r["range"][0]), float(r["m2"][0]), r


def test_clamp_bound_singular_min_points_min_range_and_skip_rules_on_hand_made_records():
    rec = _one()
    # along x through the mean: interior, m2 = 0 at range 1.75; the segment is 4 long and crosses the cell over t in [1.25 / 4, 2.25 / 4]
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1, 1), (3.25, 1, 1))
    assert (hit, cell, rng, m2) == (1, (0, 0, 0), 1.75, 0.0) and (r["interior"], r["n_cells"], r["n_hit_at_origin"]) == (1, 3, 0)
    # ending inside the cell in front of the mean: clamped high, the endpoint itself
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1, 1), (0.75, 1, 1))
    assert (hit, cell, rng, m2, r["clamped_high"]) == (1, (0, 0, 0), 1.5, 0.25, 1)
    # starting inside the cell behind the mean: clamped low at s = 0 -- the sensor sits inside map matter
    hit, cell, rng, m2, r = _cast1(rec, (1.25, 1, 1), (3.25, 1, 1))
    assert (hit, cell, rng, m2, r["clamped_low"], r["n_hit_at_origin"], r["n_cells"]) == (1, (0, 0, 0), 0.0, 0.25, 1, 1, 1)
    # the bound is inclusive
    assert _cast1(rec, (-0.75, 1, 1), (0.75, 1, 1), max_m2=0.25)[0] == 1
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1, 1), (0.75, 1, 1), max_m2=0.2499)
    assert (hit, cell, rng, m2, r["passed_through"], r["n_used"], r["n_hit"]) == (0, (0, 0, 0), RC.INF, RC.INF, 1, 1, 0)
    assert _cast1(rec, (-0.75, 1, 1), (3.25, 1, 1), max_m2=0.0)[:4] == (1, (0, 0, 0), 1.75, 0.0)
    # a singular record: with max_m2 = +inf the cell stops the ray at its entry (t_in = 1.25 / 4), with a finite bound it is passed through
    for cov in (FLAT, np.full((3, 3), np.nan, np.float32), np.diag([0.25, -0.25, 0.25]).astype(np.float32)):
        hit, cell, rng, m2, r = _cast1(_one(cov), (-0.75, 1, 1), (3.25, 1, 1))
        assert (hit, cell, rng, m2, r["singular"]) == (1, (0, 0, 0), 1.25, RC.INF, 1)
        hit, cell, rng, m2, r = _cast1(_one(cov), (-0.75, 1, 1), (3.25, 1, 1), max_m2=1e300)
        assert (hit, rng, m2, r["singular"], r["passed_through"], r["n_cells"]) == (0, RC.INF, RC.INF, 1, 0, 5)
    # ... and a regular record far from the ray stops it too when the bound is +inf
    assert _cast1(rec, (-0.75, 3.25, 1), (3.25, 3.25, 1))[0] == 0  # (another row of cells: the voxel is not visited)
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1.375, 1), (3.25, 1.375, 1))
    assert (hit, rng, m2) == (1, 1.75, 0.5625)
    # min_points
    assert _cast1(_one(num=2), (-0.75, 1, 1), (3.25, 1, 1), min_points=3)[0] == 0
    assert _cast1(_one(num=3), (-0.75, 1, 1), (3.25, 1, 1), min_points=3)[0] == 1
    assert _cast1(_one(num=1), (-0.75, 1, 1), (3.25, 1, 1), min_points=0)[0] == 1
    # min_range skips nothing: it bounds where the hit may lie. 2.0 lies inside the cell's interval, behind the mean: clamped low at t_lo
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1, 1), (3.25, 1, 1), min_range=2.0)
    assert (hit, rng, m2, r["clamped_low"], r["n_used"]) == (1, 2.0, 0.25, 1, 1)
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1, 1), (3.25, 1, 1), min_range=2.25)  # t_out == t_lo: not a candidate
    assert (hit, rng, r["n_used"], r["n_cells"], r["clamped_low"]) == (0, RC.INF, 1, 5, 0)
    hit, cell, rng, m2, r = _cast1(rec, (-0.75, 1, 1), (3.25, 1, 1), min_range=50.0)  # longer than the ray: used, nothing can be hit
    assert (hit, r["n_used"], r["n_cells"]) == (0, 1, 5)
    # skips
    lim = float((1 << 20) - 4096)
    pts = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [-0.75, 1, 1], [200.0, 1, 1], [lim + 1.0, 1, 1], [lim, 1, 1], [3e38, 1, 1], [3.25, 1, 1]], np.float32)
    r = RC.cast(rec, 1.0, pts, None, (-0.75, 1, 1), max_range=float(1 << 21))
    assert r["hit"].tolist() == [-1, -1, -1, -1, 1, -1, 1, -1, 1] and (r["n_rays"], r["n_used"], r["n_hit"]) == (9, 3, 3)
    r = RC.cast(rec, 1.0, pts, None, (-0.75, 1, 1), max_range=100.0)
    assert r["hit"].tolist() == [-1, -1, -1, -1, -1, -1, -1, -1, 1]
    skipped = r["hit"] < 0
    assert np.isnan(r["range"][skipped]).all() and np.isnan(r["m2"][skipped]).all() and not r["cell"][skipped].any()
    r = RC.cast(rec, 1.0, pts[-1:], None, (lim + 1.0, 1, 1), max_range=float(1 << 21))  # the origin's cell is outside the index range
    assert r["hit"].tolist() == [-1] and r["n_used"] == 0
    assert RC.cast(rec, 1.0, np.zeros((0, 3), np.float32))["n_rays"] == 0


def test_the_walk_visits_the_cells_of_the_clear_rays_walk_with_contiguous_intervals():
    from tests import clearrays_ref as CR
    rng = np.random.default_rng(11)
    for _ in range(200):
        a, b = rng.uniform(-6, 6, 3), rng.uniform(-6, 6, 3)
        if rng.random() < 0.3:
            b[rng.integers(3)] = a[rng.integers(3)]
        cells = RC.walk_intervals(list(a), list(b))
        assert [c for c, _, _, _ in cells] == CR.walk(list(a), list(b), 1.0)
        assert cells[0][1] == 0.0 and all(t_in <= t_out <= 1.0 for _, t_in, t_out, _ in cells)
        assert all(cells[k][2] == cells[k + 1][1] for k in range(len(cells) - 1))  # (t_in < 1.0 for every visited cell, so no t_out before it was clamped)
        if tuple(math.floor(v) for v in b) == cells[-1][0]:
            assert cells[-1][2] == 1.0
    cells = RC.walk_intervals([0.5, 0.5, 0.5], [3.5, 3.5, 0.5])  # through cell corners: x before y
    assert [c for c, _, _, _ in cells] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0), (3, 2, 0), (3, 3, 0)]
    assert [t for _, _, _, t in cells] == [True, False, True, False, True, False, False]


SCENES = [(res, n, seed) for res in (1.0, 0.5) for n, seed in ((63, 1), (64, 2), (65, 3), (257, 4), (1000, 5))]


@pytest.mark.parametrize("res,n,seed", SCENES)
def test_the_gpu_scenes_exercise_every_rule_under_the_twin(res, n, seed):
    for pose in (True, False):
        sc = RC.ray_scene(res, n, seed, pose=pose)
        assert sc["scan"].shape == (n, 3) and RC.rounding_is_stable(sc["pose"], sc["scan"], sc["origin"])
        R, t = RC.pose_parts(sc["pose"])
        assert RC.transform_point(R, t, [float(v) for v in sc["origin"]]) == tuple(float(v) for v in sc["origin_map"])
        for p, q in zip(sc["scan"], sc["targets"]):  # every product and sum of R p + t is exact: p' is the intended point
            if np.all(np.isfinite(p)):
                assert RC.transform_point(R, t, [float(v) for v in p]) == tuple(float(v) for v in q)
                assert all((v / res * 32.0) % 2.0 == 1.0 for v in q) or abs(q[0]) > 1e5  # odd multiples of res / 32 (the index-limit row is half a cell off)
    sc = RC.ray_scene(res, n, seed)
    for kind in ("additive", "multiplicative", "ndt"):
        rec = RC.model_records(kind, res, sc["map_points"], sc["map_covs"])
        assert len(rec) == RC.NUM_VOXELS
        for mp in (1, 3):
            for min_range in (0.0, res):
                r = RC.cast(rec, res, sc["scan"], sc["pose"], sc["origin"], min_range, sc["max_range"], mp, 9.0)
                what = (kind, mp, min_range, {k: r[k] for k in RC.COUNTS + RC.COUNTERS})
                assert all(r[k] > 0 for k in RC.COUNTERS), what
                assert 0 < r["n_hit"] < r["n_used"] < r["n_rays"] and r["n_cells"] > r["n_used"], what
                assert r["hit"][:11].tolist() == [1, 1, 0, 0, 0, 0, -1, -1, -1, -1, -1] and r["hit"][13] == 0, what  # the hand-made rows (11, 12: hit or passed, by voxel type)
                assert r["n_cells"] >= 1 and r["hit"][2] == 0 and tuple(r["cell"][0][:2]) == (4, 4), what  # (row 0 comes straight down the column of cells (4, 4, .))
                inf = RC.cast(rec, res, sc["scan"], sc["pose"], sc["origin"], min_range, sc["max_range"], mp, RC.INF)
                assert inf["passed_through"] == 0 and inf["n_hit"] > r["n_hit"] and inf["n_cells"] < r["n_cells"], what
                assert inf["hit"][3] == 1 and math.isinf(inf["m2"][3]) and tuple(inf["cell"][3]) == (10, 0, 0), what  # the flat voxel stops the ray at its entry
                assert inf["hit"][4] == (1 if mp == 1 else 0), what                                                   # the single-point voxel: gone with min_points = 3
    ins = RC.ray_scene(res, n, seed, inside=True)
    r = RC.cast(RC.model_records("additive", res, ins["map_points"], ins["map_covs"]), res, ins["scan"], ins["pose"], ins["origin"], 0.0, ins["max_range"], 1, 9.0)
    assert r["n_hit_at_origin"] > 0


@pytest.mark.parametrize("capacity", [64, 1024])
def test_rays_through_the_wrap_scene_meet_the_wrapping_cells_and_the_absent_one(capacity):
    w = RC.wrap_scene(capacity)
    rec = RC.model_records("additive", 1.0, w["map_points"], w["map_covs"])
    pts, origin, max_range = RC.wrap_rays(w)
    r = RC.cast(rec, 1.0, pts, None, origin, 0.0, max_range, 1, 9.0)
    nv = len(w["voxels"])
    assert r["n_used"] == len(pts) == nv + 1 and r["hit"][nv] == 0  # the ray into the absent cell finds nothing there
    assert [tuple(c) for c in r["cell"][:4].tolist()] == [tuple(v) for v in w["voxels"][:4].tolist()] and r["hit"][:4].tolist() == [1] * 4  # the four wrapped voxels
    assert r["n_hit"] >= nv - 2 and r["n_cells"] > 10 * len(pts)


def test_a_dense_analytic_plane_is_hit_at_sub_voxel_range_error():
    """a condition, with a wide margin: every ray hits and its range is within half a voxel of the analytic range to the plane. The level plane
    lies an eighth of a cell above the floor of its cells: a range taken where the ray ENTERS the hit cell through its top would be 0.88 voxels short
    and more. On the tilted plane the same bound holds for every hit; there a few rays in a hundred pierce the plane in a sliver it leaves in
    the corner of a cell, more than three sigma of that sliver's small Gaussian from its mean, and go on into empty space -- what max_m2 = 9
    means, not an error: those are counted, and bounded by one ray in twenty."""
    for res in (1.0, 0.5):
        sc = RC.analytic_plane(res, 500, 3)
        r = RC.cast(sc["records"], res, sc["scan"], None, sc["origin"], 0.0, 100.0, 3, 9.0)
        err = np.abs(r["range"] - sc["ranges"])
        print("level, res %g: %d voxels, %d hits, max |range error| %.4g m, median %.3g m" % (res, len(sc["records"]), r["n_hit"], err.max(), np.median(err)))
        assert r["n_hit"] == r["n_used"] == 500
        assert err.max() < 0.5 * res, err.max()
        entry = np.array([RC.cast(sc["records"], res, sc["scan"][i:i + 1], None, sc["origin"], 0.0, 100.0, 3, RC.INF)["range"][0] for i in range(0, 500, 25)])
        assert np.max(sc["ranges"][::25] - entry) > 0.5 * res  # stopping at the first occupied cell would miss the bound
        sc = RC.analytic_plane(res, 500, 3, tilted=True)
        r = RC.cast(sc["records"], res, sc["scan"], None, sc["origin"], 0.0, 100.0, 3, 9.0)
        hits = r["hit"] == 1
        err = np.abs(r["range"] - sc["ranges"])[hits]
        print("tilted, res %g: %d voxels, %d hits, max |range error| %.4g m, median %.3g m" % (res, len(sc["records"]), r["n_hit"], err.max(), np.median(err)))
        assert r["n_used"] == 500 and r["n_hit"] >= 475
        assert err.max() < 0.5 * res, err.max()


def test_ray_endpoints_make_no_ray_that_is_skipped_for_range():
    from fast_gicp_amd import capi
    rng = np.random.default_rng(5)
    d = rng.normal(size=(400, 3)) * rng.uniform(0.1, 30.0, (400, 1))
    far = np.array([[1.0, 0, 0, 1e5], [0, 0.6, -0.8, -3e4], [0, 0.8, 0.6, 2e3], [0, 0, 0, 1]])
    for T in (None, RC.POSE, far):
        for length in (0.37, 59.99, rng.uniform(0.5, 80.0, 400)):
            for origin in ((0.0, 0.0, 0.0), (0.3, -1.7, 2.1)):
                xyz, max_range = capi.ray_endpoints(origin, d, length, T)
                assert xyz.dtype == np.float32 and xyz.shape == (400, 3)
                want = np.asarray(origin) + d / np.linalg.norm(d, axis=1)[:, None] * np.broadcast_to(length, (400,))[:, None]
                assert np.abs(xyz - want).max() <= 2.0 ** -23 * np.abs(want).max()
                assert max_range <= np.max(length) * (1.0 + 1e-4) + 1e-4 * (1.0 if T is not far else 2e3)  # (not simply a large number)
                r = RC.cast({}, 1.0, xyz, T, origin, 0.0, max_range)
                assert r["n_used"] == r["n_rays"] == 400, (length, origin)
    with pytest.raises(capi.FvhError):
        capi.ray_endpoints((0, 0, 0), [[0.0, 0.0, 0.0]], 1.0)
    with pytest.raises(capi.FvhError):
        capi.ray_endpoints((0, 0, 0), [[1.0, 0.0, 0.0]], -1.0)
    xyz, max_range = capi.ray_endpoints((0, 0, 0), np.zeros((0, 3)), 1.0)
    assert xyz.shape == (0, 3) and max_range == 0.0


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
        tail = (z, z, d, d, 0, d, z, z, z, z, z)
        assert (fn(z, *tail) if name.endswith("source") else fn(z, z, 0, 0, 0, *tail)) == 1  # a null handle is refused before anything else
    for cls in (capi.VGICPMapCore, capi.NDTMapCore):
        assert callable(cls.map_cast_rays)
    assert callable(capi.ray_endpoints)
    assert any(s.endswith(os.sep + "kernels_raycast.hpp") for s in build.SOURCES)


def test_the_struct_mirror_matches_the_header_field_by_field(tmp_path):
    from fast_gicp_amd import capi
    hdr = _header()
    body = hdr[hdr.index("typedef struct fvh_ray_cast {"):hdr.index("} fvh_ray_cast;")]
    assert re.findall(r"^\s+(int|long long|double)\s+(\w+);", body, flags=re.M) == FIELDS
    assert [(CTYPES.get(t, "?"), n) for n, t in capi.RayCast._fields_] == FIELDS
    src = tmp_path / "rc.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fast_vgicp_hip.h"\nint main(void) { printf("%zu", sizeof(fvh_ray_cast));\n'
                   + "".join('printf(" %%zu", offsetof(fvh_ray_cast, %s));\n' % n for _, n in FIELDS) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "rc"
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(exe), str(src)])
    vals = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert ctypes.sizeof(capi.RayCast) == vals[0] == 24
    assert [getattr(capi.RayCast, n).offset for _, n in FIELDS] == vals[1:]


class _Recorder:
    """stands in for _Core._call: keeps what the wrapper hands to the library and fills the struct as the library would"""

    def __init__(self, n_points):
        self.calls, self.n_points = [], n_points

    def __call__(self, name, *args):
        if name == "get_num_source_points":  # (the rows of a per-ray cast to the source)
            args[0]._obj.value = self.n_points
            return
        self.calls.append((name, args))
        out = args[-5]._obj  # byref(RayCast)
        out.n_rays, out.n_used, out.n_hit, out.n_hit_at_origin, out.n_cells = self.n_points, 4, 2, 1, 1 << 40


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
    r = core.map_cast_rays(np.eye(4), xyz=pts, origin=(0.5, 0.25, 2.0), min_range=0.5, max_range=60.0, min_points=3, max_m2=9.0)
    assert (r["n_rays"], r["n_used"], r["n_hit"], r["n_hit_at_origin"], r["n_cells"]) == (5, 4, 2, 1, 1 << 40)
    assert r["hit"].shape == r["range"].shape == r["m2"].shape == (5,) and r["cell"].shape == (5, 3)
    assert r["hit"].dtype == r["cell"].dtype == np.int32 and r["range"].dtype == r["m2"].dtype == np.float64 and r["cell"].flags.c_contiguous
    core.map_cast_rays(device_ptr=4096, n=7, stride=4, per_ray=False)
    core.map_cast_rays(per_ray=False)  # the source: no rows
    r = core.map_cast_rays()           # the source: rows sized by the handle's point count, one casting call
    assert len(r["hit"]) == len(r["cell"]) == len(r["range"]) == len(r["m2"]) == 5
    assert [c[0] for c in rec.calls] == ["cast_rays_cloud", "cast_rays_cloud", "cast_rays_source", "cast_rays_source"]
    for name, args in rec.calls:
        proto = protos[prefix + name][1:]
        assert len(args) == len(proto), (name, args)
        assert all(_ctype_ok(a, p) for a, p in zip(args, proto)), (name, args, proto)
    first, second = rec.calls[0][1], rec.calls[1][1]
    assert first[1:4] == (5, 3, 0) and first[5] is not None and (first[6].value, first[7].value, first[8], first[9].value) == (0.5, 60.0, 3, 9.0) and all(a is not None for a in first[-4:])
    assert (second[0].value, second[1:4]) == (4096, (7, 4, 1)) and second[5] is None and second[-4:] == (None,) * 4
    assert (second[6].value, second[7].value, second[8], second[9].value) == (0.0, 100.0, 1, float("inf"))
    assert rec.calls[2][1][-4:] == (None,) * 4 and all(a is not None for a in rec.calls[3][1][-4:])
    rec.n_points = 0
    r = core.map_cast_rays(xyz=np.zeros((0, 3), np.float32))
    assert rec.calls[-1][1][0] is None and rec.calls[-1][1][-4:] == (None,) * 4 and len(r["hit"]) == 0 and r["cell"].shape == (0, 3)
    assert "hit" not in core.map_cast_rays(xyz=pts, per_ray=False)


def test_registration_hpp_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "cast.cpp"
    src.write_text('#include <fast_gicp_amd/registration.hpp>\n'
                   'using namespace fast_gicp;\n'
                   'template <class R> int use(R& r) { const double o[3] = {0.0, 0.0, 1.5}; std::vector<float> e(30, 1.f);\n'
                   '  RayCast a = r.castRays(Matrix4f::Identity(), e, o, 0.5, 60.0, 3, 9.0, true);\n'
                   '  RayCast b = r.castRaysToSource(Matrix4f::Identity());\n'
                   '  return a.n_rays + b.n_used + a.n_hit + a.n_hit_at_origin + (int)a.n_cells + (int)a.hit.size() + (int)a.cell.size() + (int)a.range.size() + (int)a.m2.size() + (int)b.hitRatio(); }\n'
                   'template int use(FastVGICPCuda<PointXYZ, PointXYZ>&);\n'
                   'template int use(FastVGICP<PointXYZ, PointXYZ>&);\n'
                   'template int use(NDTCuda<PointXYZ, PointXYZ>&);\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-fopenmp", "-I", os.path.join(util.ROOT, "include"), str(src)])


def test_pygicp_binds_the_new_method():
    src = open(os.path.join(util.ROOT, "fast_gicp_amd", "python", "pygicp.cpp")).read()
    assert src.count('"cast_rays"') >= 1 and "castRaysToSource" in src and "castRays(" in src
