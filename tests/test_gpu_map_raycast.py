"""Rays cast into the target voxel map (fvh_vgicp_cast_rays_* / fvh_ndt_cast_rays_*) against the twin of their contract.

The map's records come from the existing getters and go into tests/raycast_ref.py: hit, cell and the five counts must EQUAL the twin's, range
and m2 must be bit-equal, NaN compared as NaN (they are + - * / and one sqrt on exact widenings of floats, which the device rounds as Python
does). The one place where device and twin could differ is HOW the fp64 sum R p + t is formed before it is rounded to float32: the scenes use
poses whose products and sums are exact, and every case asserts rounding_is_stable for origin and endpoints.
(tests/test_map_raycast_cpu.py holds the twin itself to a second formulation and shows that the scenes exercise every rule.)"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import raycast_ref as RC
from tests import util

pytestmark = pytest.mark.gpu

KINDS = ("additive", "multiplicative", "ndt")
BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4
SIZES = (0, 1, 63, 64, 65, 257, 1000)


def _handle(kind, res, **params):
    from fast_gicp_amd import capi
    if kind == "ndt":
        c = capi.NDTMapCore(0)
        c.set_distance_mode(capi.NDT_P2D)
    else:
        c = capi.VGICPMapCore(0)
        c.set_voxel_accumulation_mode(capi.VOXEL_MULTIPLICATIVE if kind == "multiplicative" else capi.VOXEL_ADDITIVE)
    if params:
        c.set_engine_params(**params)
    c.set_resolution(res)
    c.set_neighbor_search_method(capi.DIRECT1)
    return c


def _build(c, kind, batch, pts, covs, expected_voxels=0, hint=None):
    """the target voxel map of (pts, covs): a batch build of the target cloud, or an incremental map with the points inserted"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    if batch:
        c.set_target_cloud(pts)
        if kind != "ndt":
            c.set_target_covariances(covs)
        if hint is not None:
            c.debug_set_voxel_hint(hint) if kind != "ndt" else c.debug_set_voxel_hint("target", hint)
        c.create_target_voxelmap()
    else:
        c.map_begin(expected_voxels)
        c.map_insert_cloud(pts) if kind == "ndt" else c.map_insert_cloud(pts, covs)
        assert c.map_info()["dropped"] == 0
    return c


def _records(c, kind):
    coords, num, means, covs = c.get_voxelmap("target") if kind == "ndt" else c.get_voxelmap()
    return RC.records_of(coords, num, means, covs)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(got, want, what):
    """one result of map_cast_rays(per_ray=True) against the twin's"""
    for k in RC.COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["hit"], want["hit"]), (what, "hit", np.flatnonzero(got["hit"] != want["hit"])[:8])
    assert np.array_equal(got["cell"], want["cell"]), (what, "cell", np.flatnonzero((got["cell"] != want["cell"]).any(axis=1))[:8])
    for k in ("range", "m2"):
        bad = np.flatnonzero((_bits(got[k]) != _bits(want[k])) & ~(np.isnan(got[k]) & np.isnan(want[k])))
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


def _same(a, b, what):
    for k in RC.COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    if "hit" in a and "hit" in b:
        assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["cell"], b["cell"]), what
        assert a["range"].tobytes() == b["range"].tobytes() and a["m2"].tobytes() == b["m2"].tobytes(), what


@pytest.fixture(scope="module")
def scene():
    sc = RC.ray_scene(1.0, 1000, 5)
    assert RC.rounding_is_stable(sc["pose"], sc["scan"], sc["origin"])
    return sc


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "incremental"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_scene_equals_the_twin_at_every_size_bound_min_points_and_min_range(kind, batch, scene):
    res, T, o = scene["res"], scene["pose"], scene["origin"]
    c = _build(_handle(kind, res), kind, batch, scene["map_points"], scene["map_covs"])
    rec = _records(c, kind)
    assert len(rec) == RC.NUM_VOXELS
    for mp in (1, 3):
        for max_m2 in (9.0, RC.INF):
            for min_range in (0.0, res):
                for n in SIZES:
                    pts = scene["scan"][:n]
                    want = RC.cast(rec, res, pts, T, o, min_range, scene["max_range"], mp, max_m2)
                    got = c.map_cast_rays(T, xyz=pts, origin=o, min_range=min_range, max_range=scene["max_range"], min_points=mp, max_m2=max_m2)
                    what = "%s %s min_points=%d max_m2=%g min_range=%g n=%d" % (kind, "batch" if batch else "incremental", mp, max_m2, min_range, n)
                    _check(got, want, what)
                    if n >= 63 and max_m2 == 9.0:  # the scene is not vacuous on the device's own records either
                        assert 0 < got["n_hit"] < got["n_used"] < got["n_rays"] and got["n_cells"] > got["n_used"], what
                        assert all(want[k] > 0 for k in RC.COUNTERS if k != "singular") and (want["singular"] > 0 or kind == "ndt"), (what, {k: want[k] for k in RC.COUNTERS})  # (NDT's MIN_EIG regularisation leaves no singular record)
                    if n == 0:
                        assert all(got[k] == 0 for k in RC.COUNTS) and len(got["hit"]) == 0
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_identity_pose_half_resolution_and_a_sensor_inside_map_matter(kind):
    for res, pose, inside in ((0.5, True, False), (1.0, False, False), (0.5, False, True)):
        sc = RC.ray_scene(res, 257, 4, pose=pose, inside=inside)
        assert RC.rounding_is_stable(sc["pose"], sc["scan"], sc["origin"])
        c = _build(_handle(kind, res), kind, False, sc["map_points"], sc["map_covs"])
        rec = _records(c, kind)
        for min_range in (0.0, res):
            want = RC.cast(rec, res, sc["scan"], sc["pose"], sc["origin"], min_range, sc["max_range"], 1, 9.0)
            got = c.map_cast_rays(sc["pose"], xyz=sc["scan"], origin=sc["origin"], min_range=min_range, max_range=sc["max_range"], max_m2=9.0)
            _check(got, want, "%s res=%g pose=%s inside=%s min_range=%g" % (kind, res, pose, inside, min_range))
            if inside and min_range == 0.0:
                assert got["n_hit_at_origin"] > 0
        if not pose and not inside:  # T = None and origin = None are the identity and (0, 0, 0): the scene shifted so that the sensor is the origin
            shift = sc["origin"].astype(np.float32)
            assert np.array_equal(shift.astype(np.float64), sc["origin"])
            T = np.eye(4); T[:3, 3] = sc["origin"]
            pts = np.delete(sc["scan"], 10, axis=0) - shift  # (without the index-limit row: 2^20 less five and a bit is no float32)
            assert RC.rounding_is_stable(T, pts)
            want = RC.cast(rec, res, pts, T, None, 0.0, sc["max_range"], 1, 9.0)
            _check(c.map_cast_rays(T, xyz=pts, max_range=sc["max_range"], max_m2=9.0), want, kind + " origin None")
            assert want["n_hit"] > 0
        c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_crowded_table_and_a_live_bitmap_change_nothing(kind, scene):
    res, T, o, pts = scene["res"], scene["pose"], scene["origin"], scene["scan"][:257]
    mp, mc = scene["map_points"], scene["map_covs"]

    def chunked(c):  # filled eight points at a time from the smallest table: the host never grows it past a load of about 0.4
        c.map_begin(1)
        for i in range(0, len(mp), 8):
            c.map_insert_cloud(mp[i:i + 8]) if kind == "ndt" else c.map_insert_cloud(mp[i:i + 8], mc[i:i + 8])
        return c

    builders = {"crowded incremental": chunked, "batch": lambda c: _build(c, kind, True, mp, mc)}
    for what, build in builders.items():
        outs = []
        for params in (dict(), dict(bitmap_min_points=1)):
            c = build(_handle(kind, res, **params))
            rec = _records(c, kind)
            assert len(rec) == RC.NUM_VOXELS
            if what == "crowded incremental":
                assert c.map_info()["capacity"] <= 512, c.map_info()
            got = c.map_cast_rays(T, xyz=pts, origin=o, max_range=scene["max_range"], max_m2=9.0)
            _check(got, RC.cast(rec, res, pts, T, o, 0.0, scene["max_range"], 1, 9.0), "%s %s bitmap=%s" % (kind, what, bool(params)))
            outs.append(got)
            c.close()
        _same(outs[1], outs[0], kind + " " + what + ": bitmap on vs off")


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "incremental"])
@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_probe_sequences_that_cross_the_end_of_the_table(kind, batch):
    """mapscore_ref.wrap_scene at the capacity the map has (incremental: 64 buckets; batch: 1,024): rays end in the four voxels whose probe
    sequence wraps and in the EMPTY cell with the same home slot; bitmap off and on give the same bits"""
    capacity = 1024 if batch else 64
    w = RC.wrap_scene(capacity)
    st = w["stats"]
    assert st["wraps"] and st["across_end"] >= 3 and st["displaced"] >= 4, st
    pts, origin, max_range = RC.wrap_rays(w)
    assert RC.rounding_is_stable(None, pts, origin)
    nv = len(w["voxels"])
    outs = []
    for params in (dict(), dict(bitmap_min_points=1)):
        c = _handle(kind, 1.0, **params)
        _build(c, kind, batch, w["map_points"], w["map_covs"], expected_voxels=1, hint=nv)
        if not batch:
            assert c.map_info()["capacity"] == capacity and c.map_info()["num_voxels"] == nv, c.map_info()
        rec = _records(c, kind)
        for max_m2 in (9.0, RC.INF):
            got = c.map_cast_rays(None, xyz=pts, origin=origin, max_range=max_range, max_m2=max_m2)
            _check(got, RC.cast(rec, 1.0, pts, None, origin, 0.0, max_range, 1, max_m2), "%s wrap capacity=%d bitmap=%s max_m2=%g" % (kind, capacity, bool(params), max_m2))
            assert got["hit"][nv] == 0 and got["n_used"] == nv + 1  # the ray into the absent cell walks to its end
            if max_m2 == RC.INF:
                assert got["hit"][:4].tolist() == [1] * 4 and got["cell"][:4].tolist() == w["voxels"][:4].tolist()  # the wrapped voxels are found
            outs.append(got)
        c.close()
    for off, on in zip(outs[:2], outs[2:]):
        _same(on, off, kind + " wrap: bitmap on vs off")


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_the_last_cell_inside_the_index_range(kind):
    """a voxel in cell 2^20 - 4097, the last one voxel_index_ok accepts: a ray into it hits it; one that ends a cell further is skipped, and so
    is every ray of a sensor that sits one cell further"""
    lim = float((1 << 20) - 4096)
    edge = np.array([[lim, 1.0, 1.0]], np.float32)  # floor(lim - 0.5) = lim - 1
    c = _build(_handle(kind, 1.0), kind, False, np.concatenate([edge, [[lim - 6.0, 1.0, 1.0]]]).astype(np.float32), np.repeat(RC.SPD[None], 2, axis=0))
    rec = _records(c, kind)
    assert (int(lim) - 1, 0, 0) in rec and len(rec) == 2
    origin = np.array([lim - 3.75, 1.25, 1.0])
    pts = np.array([[lim + 0.25, 1.0, 1.0], [lim + 1.0, 1.0, 1.0], [lim - 9.0, 1.0, 1.25], [-lim + 2.0, 1.0, 1.0]], np.float32)
    assert RC.rounding_is_stable(None, pts, origin)
    want = RC.cast(rec, 1.0, pts, None, origin, 0.0, 4096.0, 1, RC.INF)
    got = c.map_cast_rays(None, xyz=pts, origin=origin, max_range=4096.0)
    _check(got, want, kind + " index edge")
    assert got["hit"].tolist() == [1, -1, 1, -1] and got["cell"][0].tolist() == [int(lim) - 1, 0, 0] and got["n_used"] == 2
    outside = np.array([lim + 0.75, 1.0, 1.0])
    got = c.map_cast_rays(None, xyz=pts, origin=outside, max_range=4096.0)
    _check(got, RC.cast(rec, 1.0, pts, None, outside, 0.0, 4096.0, 1, RC.INF), kind + " sensor outside the index range")
    assert got["n_used"] == 0 and got["hit"].tolist() == [-1] * 4
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_a_batch_table_that_overflowed_is_rebuilt_before_it_is_cast_into(kind, scene):
    res, T, o, pts = scene["res"], scene["pose"], scene["origin"], scene["scan"][:257]
    c = _build(_handle(kind, res), kind, True, scene["map_points"], scene["map_covs"], hint=8)
    got = c.map_cast_rays(T, xyz=pts, origin=o, max_range=scene["max_range"], max_m2=9.0)
    rec = _records(c, kind)
    assert len(rec) == RC.NUM_VOXELS
    _check(got, RC.cast(rec, res, pts, T, o, 0.0, scene["max_range"], 1, 9.0), kind + " after an overflow")
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_every_route_to_the_same_endpoints_gives_the_same_bits(kind, scene):
    """_source before and after the source gets a Morton order, _cloud from the host, from the device at strides 3 and 4; with and without
    the per-ray arrays; twice"""
    import torch
    from fast_gicp_amd import capi
    res, T, o = scene["res"], scene["pose"], scene["origin"]
    pts = np.ascontiguousarray(np.delete(scene["scan"][:600], [6, 7], axis=0))  # finite rows only: the cloud is sorted below
    c = _build(_handle(kind, res), kind, False, scene["map_points"], scene["map_covs"])
    args = dict(origin=o, min_range=res, max_range=scene["max_range"], min_points=1, max_m2=9.0)
    ref_out = c.map_cast_rays(T, xyz=pts, **args)
    _check(ref_out, RC.cast(_records(c, kind), res, pts, T, o, res, scene["max_range"], 1, 9.0), kind + " host cloud")
    assert 0 < ref_out["n_hit"] < ref_out["n_used"] < ref_out["n_rays"]
    outs = {"host cloud again": c.map_cast_rays(T, xyz=pts, **args), "host cloud, no rows": c.map_cast_rays(T, xyz=pts, per_ray=False, **args)}
    d3 = torch.from_numpy(pts).cuda()
    p4 = np.zeros((len(pts), 4), np.float32); p4[:, :3] = pts; p4[:, 3] = np.nan
    d4 = torch.from_numpy(p4).cuda()
    torch.cuda.synchronize()
    outs["device cloud"] = c.map_cast_rays(T, device_ptr=d3.data_ptr(), n=len(pts), stride=3, **args)
    outs["device cloud, stride 4"] = c.map_cast_rays(T, device_ptr=d4.data_ptr(), n=len(pts), stride=4, **args)
    c.set_source_cloud(pts)
    outs["source, input order"] = c.map_cast_rays(T, **args)
    outs["source, no rows"] = c.map_cast_rays(T, per_ray=False, **args)
    before = c.map_export()
    # from here on the source HAS a Morton order and is large enough to be walked in it (coherent_min_points = 1). That the sort ran is read
    # from the profile class "sort": VGICP: the device neighbour search sorts the source; NDT: a fitness score sorts source and target cloud
    c.set_engine_params(coherent_min_points=1)
    c.profile_enable(True)
    c.profile_reset()
    c.set_source_cloud(pts)
    if kind == "ndt":
        c.target_from_map(1)
        c.fitness_score(np.eye(4))
    else:
        c.find_source_neighbors(10)
    c.synchronize()
    sorts = c.profile_get("sort")[1]
    assert sorts >= (2 if kind == "ndt" else 1), sorts
    c.profile_reset()
    outs["source, Morton order"] = c.map_cast_rays(T, **args)
    outs["source, Morton order, no rows"] = c.map_cast_rays(T, per_ray=False, **args)
    c.synchronize()
    assert c.profile_get("map_raycast")[1] == 2  # the profile scope of the kernel
    c.profile_enable(False)
    for what, got in outs.items():
        _same(got, ref_out, kind + " " + what)
        assert ("hit" in got) == ("no rows" not in what)
    after = c.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    c.close()


@pytest.fixture(scope="module")
def scans():
    """the bundled pair: the whole target with the engine's own covariances, every 16th source point"""
    tgt, src = util.bundled_pair()
    tgt, rays = np.ascontiguousarray(tgt), np.ascontiguousarray(src[::16])
    c = _handle("additive", 1.0)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances()
    Ct = c.get_covariances("target").astype(np.float64)
    c.close()
    return dict(tgt=tgt, src=np.ascontiguousarray(src[:1000]), rays=rays, Ct=Ct, T=util.relative_pose())


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "incremental"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_real_scan_cast_into_a_real_map_equals_the_twin(kind, batch, scans):
    """every 16th point of the bundled source as an endpoint into the map of the bundled target: identity pose, so every product is exact; the
    sensor at a dyadic point; resolution 1.0, max_range 60"""
    origin = np.array([0.25, -0.125, 0.5])
    assert RC.rounding_is_stable(None, scans["rays"], origin)
    c = _build(_handle(kind, 1.0), kind, batch, scans["tgt"], scans["Ct"])
    rec = _records(c, kind)
    assert len(rec) > 500, len(rec)
    for mp, max_m2, min_range in ((1, 9.0, 0.0), (3, 9.0, 1.0), (1, RC.INF, 0.0)):
        want = RC.cast(rec, 1.0, scans["rays"], None, origin, min_range, 60.0, mp, max_m2)
        got = c.map_cast_rays(None, xyz=scans["rays"], origin=origin, min_range=min_range, max_range=60.0, min_points=mp, max_m2=max_m2)
        what = "bundled %s %s min_points=%d max_m2=%g min_range=%g" % (kind, "batch" if batch else "incremental", mp, max_m2, min_range)
        print(what, {k: got[k] for k in RC.COUNTS})
        _check(got, want, what)
        assert 0 < got["n_hit"] <= got["n_used"] <= got["n_rays"] == len(scans["rays"]) and (got["n_hit"] < got["n_used"] or max_m2 == RC.INF), what
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_the_call_leaves_the_handle_as_it_was(kind, scans):
    """export byte-equal, stored correspondences unchanged, compute_error and align after a cast give the bits they gave without one, and a
    cast between prepare_source_device and adopt_prepared_source leaves the prepared pipeline's pose bit-identical"""
    from fast_gicp_amd import capi
    tgt, src, T = scans["tgt"][:2000], scans["src"], scans["T"]
    assert RC.rounding_is_stable(T, src)

    def fresh():
        c = _build(_handle(kind, 1.0), kind, False, tgt, scans["Ct"][:2000])
        c.set_neighbor_search_method(capi.DIRECT7)
        if kind == "ndt":
            c.set_source_cloud(src)
        else:
            c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
        return c

    def cast(c, **kw):
        return c.map_cast_rays(T, min_points=2, max_range=80.0, max_m2=9.0, **kw)

    a, b = fresh(), fresh()
    before, info = a.map_export(), a.map_info()
    for c in (a, b):
        c.update_correspondences(T)
    corr = a.get_voxel_correspondences().copy()
    s1 = cast(a)
    s2 = cast(a, xyz=src[:500], per_ray=False)
    assert s1["n_hit"] > 0 and s2["n_rays"] == 500 and len(s1["hit"]) == len(src)
    _check(s1, RC.cast(_records(a, kind), 1.0, src, T, None, 0.0, 80.0, 2, 9.0), kind + " source at the pair's pose")
    assert np.array_equal(a.get_voxel_correspondences(), corr)
    ea, eb = a.compute_error(T), b.compute_error(T)
    assert ea[0] == eb[0] and ea[1].tobytes() == eb[1].tobytes() and ea[2].tobytes() == eb[2].tobytes()
    after = a.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert a.map_info() == info
    ra = a.align(T)
    cast(a, per_ray=False)
    ra2 = a.align(T)
    rb = b.align(T)
    assert ra["T"].tobytes() == rb["T"].tobytes() == ra2["T"].tobytes() and ra["nr_iterations"] == rb["nr_iterations"] == ra2["nr_iterations"]
    # between prepare_source_device and adopt_prepared_source
    import torch
    d_src = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    for c, with_cast in ((a, True), (b, False)):
        c.prepare_source_device(d_src.data_ptr(), len(src), 3)
        if with_cast:
            _same(cast(c, xyz=src), s1, "cast beside a preparation")
        c.adopt_prepared_source()
    pa, pb = a.align(T), b.align(T)
    assert pa["T"].tobytes() == pb["T"].tobytes() and pa["nr_iterations"] == pb["nr_iterations"]
    a.close(); b.close()


def _raw_tail(T=None, origin=None, min_range=0.0, max_range=24.0, min_points=1, max_m2=9.0, out=True):
    from fast_gicp_amd import capi
    t = np.ascontiguousarray(np.eye(4)) if T is None or T is False else capi._colmajor16(T)
    o = None if origin is None else np.ascontiguousarray(origin, np.float64)
    s = capi.RayCast()
    keep = (t, s, o)
    return keep, (None if T is False else capi._p(t), None if o is None else capi._p(o), C.c_double(min_range), C.c_double(max_range), int(min_points), C.c_double(max_m2),
                  C.byref(s) if out else None, None, None, None, None)


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_every_refusal_is_followed_by_a_call_that_works(kind, scene, scans):
    from fast_gicp_amd import capi
    res, T, o, pts = scene["res"], scene["pose"], scene["origin"], np.ascontiguousarray(scene["scan"][:200])
    prefix = "fvh_ndt_" if kind == "ndt" else "fvh_vgicp_"

    def refused(c, code, word, name, *args):
        fn = getattr(c._lib, prefix + name)
        fn.restype = C.c_int
        rc = fn(c.h, *args)
        msg = getattr(c._lib, prefix + "last_error")(c.h).decode()
        assert rc == code and word in msg, (name, rc, msg)

    c = _handle(kind, res)
    keep, a = _raw_tail()
    cloud = (capi._p(pts), len(pts), 3, 0)
    refused(c, BAD_STATE, "no target voxel map", "cast_rays_source", *a)
    refused(c, BAD_STATE, "no target voxel map", "cast_rays_cloud", *cloud, *a)
    if kind != "ndt":  # (a handle with map sharding on cannot hold an incremental map: asked before one is live)
        c.set_target_map_sharding(True)
        refused(c, UNSUPPORTED, "multi-GPU", "cast_rays_source", *a)
        refused(c, UNSUPPORTED, "multi-GPU", "cast_rays_cloud", *cloud, *a)
        c.set_target_map_sharding(False)
    _build(c, kind, False, scene["map_points"], scene["map_covs"])
    want = RC.cast(_records(c, kind), res, pts, T, o, 0.0, scene["max_range"], 1, 9.0)

    def works():
        _check(c.map_cast_rays(T, xyz=pts, origin=o, max_range=scene["max_range"], max_m2=9.0), want, kind + " after a refusal")

    works()
    refused(c, BAD_STATE, "source cloud is not set", "cast_rays_source", *a)
    works()
    c.set_source_cloud(pts[11:])
    bad_T = np.eye(4); bad_T[2, 3] = np.nan
    nan, inf = float("nan"), float("inf")
    table = [("pose is not finite", dict(T=bad_T)), ("null pose", dict(T=False)), ("origin", dict(origin=(0.0, nan, 0.0))), ("origin", dict(origin=(inf, 0.0, 0.0))),
             ("null result", dict(out=False)), ("min_range", dict(min_range=-1.0)), ("min_range", dict(min_range=nan)), ("max_range", dict(max_range=inf)),
             ("max_range", dict(max_range=nan)), ("max_range", dict(min_range=5.0, max_range=4.0)), ("4096 voxels", dict(max_range=4096.0 * res + 1.0)),
             ("max_m2", dict(max_m2=nan)), ("max_m2", dict(max_m2=-1.0))]
    for word, kw in table:
        keep, bad = _raw_tail(**kw)
        refused(c, BAD_ARG, word, "cast_rays_source", *bad)
        refused(c, BAD_ARG, word, "cast_rays_cloud", *cloud, *bad)
        works()
    refused(c, BAD_ARG, "n < 0", "cast_rays_cloud", capi._p(pts), -1, 3, 0, *a)
    refused(c, BAD_ARG, "null points", "cast_rays_cloud", None, 5, 3, 0, *a)
    refused(c, BAD_ARG, "stride", "cast_rays_cloud", capi._p(pts), len(pts), 5, 0, *a)
    refused(c, BAD_ARG, "stride", "cast_rays_cloud", capi._p(pts), len(pts), 2, 1, *a)
    works()
    # n == 0, max_m2 = +inf, max_range == 4096 res and min_range == max_range are legal
    keep, ok = _raw_tail(max_m2=inf, max_range=4096.0 * res, min_range=4096.0 * res)
    fn = getattr(c._lib, prefix + "cast_rays_cloud"); fn.restype = C.c_int
    assert fn(c.h, None, 0, 3, 0, *ok) == 0 and (keep[1].n_rays, keep[1].n_used, keep[1].n_cells) == (0, 0, 0)
    assert fn(c.h, *cloud, *ok) == 0 and keep[1].n_rays == len(pts) and keep[1].n_hit == 0 and keep[1].n_used > 0
    # an align_async in flight
    c.close()
    c = _build(_handle(kind, 1.0), kind, False, scans["tgt"][:2000], scans["Ct"][:2000])
    c.set_neighbor_search_method(capi.DIRECT7)
    if kind == "ndt":
        c.set_source_cloud(scans["src"])
    else:
        c.set_source_cloud(scans["src"]); c.find_source_neighbors(20); c.calculate_source_covariances()
    before = c.map_export()
    c.align_async(scans["T"])
    refused(c, BAD_STATE, "align_async", "cast_rays_source", *a)
    refused(c, BAD_STATE, "align_async", "cast_rays_cloud", *cloud, *a)
    c.align_wait()
    got = c.map_cast_rays(scans["T"], max_range=80.0, max_m2=9.0)
    _check(got, RC.cast(_records(c, kind), 1.0, scans["src"], scans["T"], None, 0.0, 80.0, 1, 9.0), kind + " after align_wait")
    after = c.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    c.close()


def test_pygicp_and_the_cpp_class_give_what_the_c_abi_gives(scans):
    """pygicp.cast_rays goes through DeviceRegistration::castRays / castRaysToSource: on an NDT map (points only: both routes build the same
    map) the result equals capi.map_cast_rays to the bit; on a VGICP map the rows are consistent with the counts"""
    import pygicp
    from fast_gicp_amd import capi
    t, s, T = scans["tgt"][:2000], scans["src"], scans["T"]
    T = T.astype(np.float32).astype(np.float64)  # (the C++ classes take a float pose)
    origin = np.array([0.25, -0.125, 0.5])
    c = _build(_handle("ndt", 1.0), "ndt", False, t, None)
    c.set_source_cloud(s)
    args = dict(origin=origin, min_range=0.5, max_range=80.0, min_points=2, max_m2=9.0)
    want_src = c.map_cast_rays(T, **args)
    want_cloud = c.map_cast_rays(T, xyz=scans["rays"], **args)
    c.close()
    reg = pygicp.NDTCudaMap()
    reg.set_resolution(1.0)
    reg.begin_incremental_target()
    reg.set_input_source(t.astype(np.float64)); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s.astype(np.float64))
    got = reg.cast_rays(T, **args)
    _same(got, want_src, "pygicp NDT, source")
    assert got["cell"].shape == (len(s), 3) and got["hit"].dtype == np.int32 and got["hit_ratio"] == want_src["n_hit"] / want_src["n_used"] and want_src["n_hit"] > 0
    _same(reg.cast_rays(T, endpoints=scans["rays"], **args), want_cloud, "pygicp NDT, endpoints")
    assert "hit" not in reg.cast_rays(T, per_ray=False, **args)
    reg = pygicp.FastVGICPCuda()
    reg.set_resolution(1.0)
    reg.begin_incremental_target()
    reg.set_input_source(t.astype(np.float64)); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s.astype(np.float64))
    got = reg.cast_rays(T, max_m2=9.0)
    assert got["n_rays"] == len(s) == len(got["hit"]) and got["n_used"] == int((got["hit"] >= 0).sum()) and got["n_hit"] == int((got["hit"] == 1).sum()) > 0
    assert np.all(np.isfinite(got["range"][got["hit"] == 1])) and np.all(np.isinf(got["range"][got["hit"] == 0])) and not math.isnan(got["hit_ratio"])
    with pytest.raises(Exception):
        reg.cast_rays(T, max_range=-1.0)
