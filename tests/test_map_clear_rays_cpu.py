"""Free-space carving without a GPU: tests/clearrays_ref.py (the twin the GPU tests hold the kernel to) is itself held to GEOMETRY here,
independently of its walk -- every cell of a ray's bounding box is tested against the segment with a slab test in fp64 --, to the tie rule
and the step bound of the contract; the Python wrapper's argument checks; the four C symbols."""
import ctypes
import math

import numpy as np
import pytest

from tests import clearrays_ref as ref

EPS = 1e-9


def _random_rays(seed, n):
    """(o32, p32, res, end_margin) of short rays: a few cells long, some parallel to an axis or a plane, some with an end margin"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        res = (0.5, 1.0)[i % 2]
        o = rng.uniform(-3.0, 3.0, 3).astype(np.float32)
        p = (o + rng.uniform(-4.0, 4.0, 3)).astype(np.float32)
        if i % 5 == 0:
            k = int(rng.integers(3))
            p[k] = o[k]  # d == 0 on one axis
        if i % 11 == 0:
            k = int(rng.integers(3))
            p[(k + 1) % 3], p[(k + 2) % 3] = o[(k + 1) % 3], o[(k + 2) % 3]  # ... on two
        margin = (0.0, 0.0, 0.3, 0.75)[i % 4]
        out.append(([float(v) for v in o], [float(v) for v in p], res, margin))
    return out


def _slab(a, d, cell, t_end, grow):
    """[lo, hi] of the t in [0, t_end] at which a + t d lies in `cell` grown by `grow` per side (hi < lo: none)"""
    lo, hi = 0.0, t_end
    for k in range(3):
        c0, c1 = cell[k] - grow, cell[k] + 1.0 + grow
        if d[k] == 0.0:
            if not (c0 <= a[k] <= c1):
                return 1.0, 0.0
            continue
        t0, t1 = (c0 - a[k]) / d[k], (c1 - a[k]) / d[k]
        lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
    return lo, hi


def test_the_twin_crosses_the_cells_the_segment_crosses():
    checked = 0
    for o32, p32, res, margin in _random_rays(7, 400):
        ray = ref.ray_setup(o32, p32, res, 0.0, 1e3, margin)
        if ray is None:
            continue
        a, b, t_end = ray
        crossed = ref.walk(a, b, t_end)
        assert len(set(crossed)) == len(crossed)
        d = [b[k] - a[k] for k in range(3)]
        for cell in crossed:  # every crossed cell touches the segment t in [0, t_end]
            lo, hi = _slab(a, d, cell, t_end, EPS)
            assert lo <= hi, (o32, p32, res, margin, cell)
        lo_c = [min(math.floor(a[k]), math.floor(b[k])) - 1 for k in range(3)]
        hi_c = [max(math.floor(a[k]), math.floor(b[k])) + 1 for k in range(3)]
        got = set(crossed)
        for x in range(lo_c[0], hi_c[0] + 1):
            for y in range(lo_c[1], hi_c[1] + 1):
                for z in range(lo_c[2], hi_c[2] + 1):
                    lo, hi = _slab(a, d, (x, y, z), t_end, 0.0)
                    if hi - EPS > lo + EPS:  # the segment spends more than a touch inside the cell: it must be crossed
                        assert (x, y, z) in got, (o32, p32, res, margin, (x, y, z), lo, hi)
        checked += 1
    assert checked >= 350


def test_the_step_bound_ends_every_walk_in_the_endpoints_cell():
    """with no t_end to stop it the walk takes exactly N steps and stands in floor(b): it can never pass the endpoint's cell"""
    for o32, p32, res, _ in _random_rays(11, 300):
        ray = ref.ray_setup(o32, p32, res, 0.0, 1e3, 0.0)
        if ray is None:
            continue
        a, b, t_end = ray
        n_steps = sum(abs(math.floor(b[k]) - math.floor(a[k])) for k in range(3))
        free = ref.walk(a, b, ref.INF)
        assert len(free) == n_steps + 1 and free[-1] == tuple(math.floor(v) for v in b)
        assert free[0] == tuple(math.floor(v) for v in a)
        for u, v in zip(free, free[1:]):
            assert sum(abs(u[k] - v[k]) for k in range(3)) == 1  # one axis per step
        bounded = ref.walk(a, b, t_end)
        assert bounded == free[:len(bounded)] and len(bounded) <= n_steps + 1


def test_ties_on_corner_diagonals_step_x_then_y_then_z():
    # res 1: the cell centre (1, 1, 1) is grid coordinate 0.5; the diagonal meets every corner exactly (all values dyadic, every operation exact)
    a, b, t_end = ref.ray_setup((1.0, 1.0, 1.0), (3.0, 3.0, 3.0), 1.0, 0.0, 100.0, 0.0)
    assert a == [0.5, 0.5, 0.5] and b == [2.5, 2.5, 2.5] and t_end == 1.0
    assert ref.walk(a, b, t_end) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]
    # the same towards negative coordinates, res 0.5, coordinates multiples of 1/8
    a, b, t_end = ref.ray_setup((0.375, 0.375, 0.375), (-0.625, -0.625, -0.625), 0.5, 0.0, 100.0, 0.0)
    assert a == [0.25, 0.25, 0.25] and b == [-1.75, -1.75, -1.75]
    assert ref.walk(a, b, t_end) == [(0, 0, 0), (-1, 0, 0), (-1, -1, 0), (-1, -1, -1), (-2, -1, -1), (-2, -2, -1), (-2, -2, -2)]
    # a face diagonal: z never steps; ties between x and y only
    a, b, t_end = ref.ray_setup((1.0, 1.0, 1.0), (3.0, 3.0, 1.0), 1.0, 0.0, 100.0, 0.0)
    assert ref.walk(a, b, t_end) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)]
    # y and z tie, x is later: y before z
    a, b, t_end = ref.ray_setup((1.0, 1.0, 1.0), (1.5, 2.0, 2.0), 1.0, 0.0, 100.0, 0.0)
    assert ref.walk(a, b, t_end) == [(0, 0, 0), (0, 1, 0), (0, 1, 1)]  # (floor(b) = (1, 1, 1) is entered at t == 1: not before t_end)


def test_end_margin_and_skips_of_the_twin():
    # one ray along +x through cells 0..4 at res 1 (centres 1..5): r = 4, every entry time a multiple of 1/8
    o, p = (1.0, 1.0, 1.0), (5.0, 1.0, 1.0)
    cells = lambda m: ref.walk(*ref.ray_setup(o, p, 1.0, 0.0, 100.0, m))
    assert cells(0.0) == [(x, 0, 0) for x in range(5)]
    assert cells(0.5) == [(x, 0, 0) for x in range(4)]       # t_end = 0.875: cell 4 is entered at exactly 0.875, which is not before it
    assert cells(0.25) == [(x, 0, 0) for x in range(5)]
    assert cells(5.0) == []                                  # more than r: t_end < 0, not even the origin's cell
    assert cells(4.0) == []                                  # t_end == 0: 0 < 0 is false
    assert ref.ray_setup(o, o, 1.0, 0.0, 100.0, 0.0) is None                       # r == 0
    assert ref.ray_setup(o, p, 1.0, 4.5, 100.0, 0.0) is None                       # r < min_range
    assert ref.ray_setup(o, p, 1.0, 0.0, 3.5, 0.0) is None                         # r > max_range
    assert ref.ray_setup(o, p, 1.0, 4.0, 4.0, 0.0) is not None                     # both bounds are inclusive
    assert ref.ray_setup(o, (float(ref.LIM), 1.0, 1.0), 1.0, 0.0, 1e9, 0.0) is not None    # cell LIM - 1: the last one in range
    assert ref.ray_setup(o, (float(ref.LIM + 1), 1.0, 1.0), 1.0, 0.0, 1e9, 0.0) is None    # cell LIM: the endpoint's cell is out of range
    assert ref.ray_setup(o, (float("inf"), 1.0, 1.0), 1.0, 0.0, 1e9, 0.0) is None
    snap = dict(resolution=1.0, coords=np.array([[x, 0, 0] for x in range(5)], np.int32), sums=np.ones((5, 10)), ages=np.zeros(5, np.uint32))
    pts = np.array([p, (np.nan, 0, 0), (np.inf, 0, 0), o], np.float32)
    out, removed, used = ref.clear_rays(snap, pts, origin=o)
    assert (removed, used) == (4, 1) and out["coords"].tolist() == [[4, 0, 0]]  # the endpoint's voxel is crossed AND hit: it stays
    out, removed, used = ref.clear_rays(snap, np.array([p, p], np.float32), origin=o, min_misses=3)
    assert (removed, used) == (0, 2) and out["num_voxels"] == 5


REFUSED = [dict(min_range=-0.1), dict(min_range=float("nan")), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(min_range=2.0, max_range=1.0),
           dict(end_margin=-1.0), dict(end_margin=float("inf")), dict(end_margin=float("nan")), dict(min_misses=0), dict(min_misses=-3),
           dict(origin=[0.0, float("nan"), 0.0]), dict(origin=[0.0, 0.0, float("inf")]), dict(origin=[0.0, 0.0])]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_the_wrapper_refuses_before_it_calls(bad):
    from fast_gicp_amd import capi
    args = dict(min_range=0.0, max_range=50.0, end_margin=0.0, min_misses=1, origin=None)
    capi.clear_rays_check(**args)
    capi.clear_rays_check(**dict(args, origin=[0.0, 0.0, 1.7], min_range=1.0, max_range=1.0, min_misses=2))
    with pytest.raises(capi.FvhError):
        capi.clear_rays_check(**dict(args, **bad))
    for cls in (capi.VGICPMapCore, capi.NDTMapCore):
        core = object.__new__(cls)  # no handle, no GPU: the check comes before the call
        core.h = None
        with pytest.raises(capi.FvhError):
            core.map_clear_rays(**bad)


def test_the_library_declares_and_exports_the_four_entry_points():
    from fast_gicp_amd import build, capi
    names = ["fvh_%s_clear_rays_%s" % (k, f) for k in ("vgicp", "ndt") for f in ("source", "cloud")]
    lib = ctypes.CDLL(build.build_lib())
    for name in names:
        assert name in capi.declared_symbols() and hasattr(lib, name), name
    for name in names:  # a null handle is refused before anything else
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        z, d = ctypes.c_void_p(None), ctypes.c_double(0.0)
        assert fn(z, z, z, d, d, d, 0, z, z) == 1 if name.endswith("source") else fn(z, z, 0, 0, 0, z, z, d, d, d, 0, z, z) == 1
