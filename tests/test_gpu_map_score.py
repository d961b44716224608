"""A posed scan scored against the target voxel map (fvh_vgicp_score_* / fvh_ndt_score_*) against the twin of its contract.

The map's records come from the existing getters and go into tests/mapscore_ref.py: found, best and every count must EQUAL the twin's, best_m2
must be bit-equal (it is + - * / on exact widenings of the record's floats, which the device rounds as Python does), sum_best_m2 is held to
n * 2^-53 * sum |term| of math.fsum (any order of n additions) and the two score sums to (n + 8) * 2^-53 * sum |term| (the 8: device exp and libm
exp, each within 1 ulp, taken twice over). The one place where device and twin could differ is HOW the fp64 sum R p + t is formed before it is
rounded to float32: the scenes use a pose whose products and sums are exact, and the bundled-scan case is screened by rounding_is_stable.
(tests/test_map_score_cpu.py holds the twin itself to a second formulation and shows that the scenes exercise every rule.)"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import mapscore_ref as M
from tests import util

pytestmark = pytest.mark.gpu

KINDS = ("additive", "multiplicative", "ndt")
BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4
SIZES = (0, 1, 63, 64, 65, 257, 1000)
MAX_M2 = 16.0
COUNTS = ("n_points", "n_used", "n_in_voxel", "n_near", "n_explained")
SUMS = ("sum_best_m2", "sum_score_max", "sum_score_all")


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
    c.set_neighbor_search_method(capi.DIRECT1)  # the handle's own search method plays no part in a score
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
    return M.records_of(coords, num, means, covs)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(got, want, what, sums=True):
    """one result of map_score(per_point=True) against the twin's"""
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["found"], want["found"]), (what, "found", np.flatnonzero(got["found"] != want["found"])[:8])
    assert np.array_equal(got["best"], want["best"]), (what, "best", np.flatnonzero(got["best"] != want["best"])[:8])
    bad = np.flatnonzero(_bits(got["best_m2"]) != _bits(want["best_m2"]))
    assert len(bad) == 0, (what, "best_m2", bad[:8], got["best_m2"][bad[:8]], want["best_m2"][bad[:8]])
    if sums:
        bounds = M.sum_bounds(want["terms"])
        for k, b in zip(SUMS, bounds):
            err = abs(got[k] - want[k])
            print("%s %s: device %.17g twin %.17g |diff| %.3g bound %.3g" % (what, k, got[k], want[k], err, b))
            assert err <= b, (what, k, got[k], want[k], err, b)


def _same_struct(a, b, what):
    for k in COUNTS:
        assert a[k] == b[k], (what, k)
    for k in SUMS:
        assert _bits([a[k]])[0] == _bits([b[k]])[0], (what, k, a[k], b[k])


@pytest.fixture(scope="module")
def scene():
    return M.plane_scene(1.0, 1000, 5)


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "incremental"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_scene_equals_the_twin_at_every_size_offset_set_and_min_points(kind, batch, scene):
    from fast_gicp_amd import capi
    res, T = scene["res"], scene["pose"]
    c = _build(_handle(kind, res), kind, batch, scene["map_points"], scene["map_covs"])
    rec = _records(c, kind)
    assert len(rec) == 100
    for nb in (capi.DIRECT1, capi.DIRECT7, capi.DIRECT27):
        for mp in (1, 3):
            for n in SIZES:
                pts = scene["scan"][:n]
                want = M.score(rec, res, pts, T, nb, mp, MAX_M2, 1.0)
                got = c.map_score(T, xyz=pts, neighbors=nb, min_points=mp, max_m2=MAX_M2, per_point=True)
                what = "%s %s nb=%d min_points=%d n=%d" % (kind, "batch" if batch else "incremental", nb, mp, n)
                _check(got, want, what)
                if n >= 63 and nb != capi.DIRECT1:  # the scene is not vacuous on the device's own records either
                    assert 0 < got["n_in_voxel"] < got["n_near"] < got["n_used"] < got["n_points"] and 0 < got["n_explained"] < got["n_near"], what
                    assert want["ties"] >= 1 and (want["singular_hits"] >= 1 or kind == "ndt"), what  # (NDT's MIN_EIG regularisation leaves no singular record)
                    assert got["best"][1] == (1 if nb == capi.DIRECT7 else 4) and got["found"][1] == 2, what  # the hand-made tie: first in offset order
                if n == 0:
                    assert all(got[k] == 0 for k in COUNTS + SUMS) and math.isnan(got["overlap"])
    # other parameters: an unbounded and a zero max_m2, another score_scale
    pts = scene["scan"][:257]
    for max_m2, scale in ((M.INF, 1.0), (0.0, 1.0), (MAX_M2, 0.125), (MAX_M2, 3.0)):
        want = M.score(rec, res, pts, T, capi.DIRECT27, 1, max_m2, scale)
        _check(c.map_score(T, xyz=pts, neighbors=capi.DIRECT27, max_m2=max_m2, score_scale=scale, per_point=True), want, "%s max_m2=%g scale=%g" % (kind, max_m2, scale))
    c.close()


def test_more_than_one_chunk_of_the_fixed_order_sum(scene):
    """the sums are added per chunk of 16,384 entries and then across chunks: one entry short of a chunk, a full chunk, and a chunk and five"""
    from fast_gicp_amd import capi
    res, T = scene["res"], scene["pose"]
    c = _build(_handle("additive", res), "additive", False, scene["map_points"], scene["map_covs"])
    rec = _records(c, "additive")
    big = np.ascontiguousarray(np.tile(scene["scan"], (17, 1))[:16384 + 5])
    want_all = M.score(rec, res, big, T, capi.DIRECT7, 1, MAX_M2, 1.0)
    for n in (16383, 16384, 16384 + 5):
        want = M.score(rec, res, big[:n], T, capi.DIRECT7, 1, MAX_M2, 1.0) if n != len(big) else want_all
        got = c.map_score(T, xyz=big[:n], neighbors=capi.DIRECT7, max_m2=MAX_M2, per_point=True)
        _check(got, want, "additive n=%d" % n)
        _same_struct(c.map_score(T, xyz=big[:n], neighbors=capi.DIRECT7, max_m2=MAX_M2), got, "n=%d, no rows" % n)
    c.close()


@pytest.fixture(scope="module")
def scans():
    """the bundled pair's first 2,000 target points with the engine's own covariances, 1,000 source points, the pose between the scans"""
    tgt, src = util.bundled_pair()
    tgt, src = np.ascontiguousarray(tgt[:2000]), np.ascontiguousarray(src[:1000])
    c = _handle("additive", 1.0)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances()
    Ct = c.get_covariances("target").astype(np.float64)
    c.close()
    T = util.relative_pose()
    assert M.rounding_is_stable(T, src)
    return dict(tgt=tgt, src=src, Ct=Ct, T=T)


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "incremental"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_real_scan_on_a_real_map_equals_the_twin(kind, batch, scans):
    from fast_gicp_amd import capi
    c = _build(_handle(kind, 1.0), kind, batch, scans["tgt"], scans["Ct"])
    rec = _records(c, kind)
    assert 30 <= len(rec) <= 900, len(rec)
    for nb in (capi.DIRECT1, capi.DIRECT7, capi.DIRECT27):
        for mp in (1, 3):
            want = M.score(rec, 1.0, scans["src"], scans["T"], nb, mp, 9.0, 1.0)
            got = c.map_score(scans["T"], xyz=scans["src"], neighbors=nb, min_points=mp, max_m2=9.0, per_point=True)
            _check(got, want, "bundled %s %s nb=%d min_points=%d" % (kind, "batch" if batch else "incremental", nb, mp))
            assert 0 < got["n_near"] <= got["n_used"] == 1000
    c.close()


def _chunked(c, kind, pts, covs, chunk=8):
    """an incremental map filled eight points at a time from the smallest table: the host then never has a reason to grow it past a load of
    about 0.4 (one insert of all the points would size the table for one voxel per point)"""
    c.map_begin(1)
    for i in range(0, len(pts), chunk):
        c.map_insert_cloud(pts[i:i + chunk]) if kind == "ndt" else c.map_insert_cloud(pts[i:i + chunk], covs[i:i + chunk])
    return c


@pytest.mark.parametrize("kind", KINDS)
def test_a_crowded_table_and_a_live_bitmap_change_nothing(kind, scene):
    """the scene's map in a roomy table, in the smallest table the host's load rule allows (load 0.39: probe sequences collide; the wrap has a test
    of its own below) and as a batch build, each with the occupancy bitmap off and forced on: every map equals the twin on its own records, and
    the bitmap changes no bit"""
    from fast_gicp_amd import capi
    res, T, pts = scene["res"], scene["pose"], scene["scan"]
    mp, mc = scene["map_points"], scene["map_covs"]
    builders = {"roomy incremental": lambda c: _build(c, kind, False, mp, mc, expected_voxels=4096), "crowded incremental": lambda c: _chunked(c, kind, mp, mc),
                "batch": lambda c: _build(c, kind, True, mp, mc), "batch, hint-sized table": lambda c: _build(c, kind, True, mp, mc, hint=100)}
    for what, build in builders.items():
        outs = []
        for params in (dict(), dict(bitmap_min_points=1)):
            c = build(_handle(kind, res, **params))
            rec = _records(c, kind)
            assert len(rec) == 100
            if what == "crowded incremental":
                assert c.map_info()["capacity"] <= 512, c.map_info()
            for nb in (capi.DIRECT7, capi.DIRECT27):
                got = c.map_score(T, xyz=pts, neighbors=nb, max_m2=MAX_M2, per_point=True)
                _check(got, M.score(rec, res, pts, T, nb, 1, MAX_M2, 1.0), "%s %s bitmap=%s nb=%d" % (kind, what, bool(params), nb))
                outs.append(got)
            c.close()
        for off, on in zip(outs[:2], outs[2:]):
            _same_struct(on, off, kind + " " + what + ": bitmap on vs off")
            assert np.array_equal(on["found"], off["found"]) and np.array_equal(on["best"], off["best"]) and np.array_equal(_bits(on["best_m2"]), _bits(off["best_m2"])), what


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "incremental"])
@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_probe_sequences_that_cross_the_end_of_the_table(kind, batch):
    """M.wrap_scene at the capacity the map has (incremental: 64 buckets, read back from the map; batch: the 1,024 of build_voxelmap's floor): four voxels whose home slot is the last one sit
    in slots capacity - 1, 0, 1, 2, and an EMPTY cell with the same home slot is looked up too -- hits and the miss are found by probes that
    wrap. tests/table_sim.py says so for the table scored; bitmap off and on give the same bits."""
    from fast_gicp_amd import capi
    capacity = 1024 if batch else 64
    w = M.wrap_scene(capacity)
    st = w["stats"]
    assert st["wraps"] and st["across_end"] >= 3 and st["displaced"] >= 4, st
    outs = []
    for params in (dict(), dict(bitmap_min_points=1)):
        c = _handle(kind, 1.0, **params)
        _build(c, kind, batch, w["map_points"], w["map_covs"], expected_voxels=1, hint=len(w["voxels"]))
        if not batch:  # the table table_sim filled. (A batch table's size is not reported: build_voxelmap gives a cloud of up to 512 points 1,024 buckets)
            assert c.map_info()["capacity"] == capacity and c.map_info()["num_voxels"] == len(w["voxels"]), c.map_info()
        rec = _records(c, kind)
        for nb in (capi.DIRECT1, capi.DIRECT27):
            got = c.map_score(None, xyz=w["scan"], neighbors=nb, max_m2=MAX_M2, per_point=True)
            _check(got, M.score(rec, 1.0, w["scan"], None, nb, 1, MAX_M2, 1.0), "%s wrap capacity=%d bitmap=%s nb=%d" % (kind, capacity, bool(params), nb))
            assert got["found"].tolist() == [1] * 36 + [0, 0] and got["best"][:4].tolist() == [0 if nb == capi.DIRECT1 else 13] * 4  # the wrapped voxels are found, the absent cell is not
            outs.append(got)
        c.close()
    for off, on in zip(outs[:2], outs[2:]):
        _same_struct(on, off, kind + " wrap: bitmap on vs off")
        assert np.array_equal(_bits(on["best_m2"]), _bits(off["best_m2"]))


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_the_last_cell_inside_the_index_range(kind):
    """a voxel and a point in cell 2^20 - 4097, the last one voxel_index_ok accepts: used and found; one cell further the point is skipped; one
    cell nearer it finds the voxel through +x. (A neighbour of a used point can never fail coord_in_range: the index rule leaves 4,096 cells.)"""
    from fast_gicp_amd import capi
    lim = float((1 << 20) - 4096)
    edge = np.array([[lim, 1.0, 1.0]], np.float32)  # floor(lim - 0.5) = lim - 1
    c = _build(_handle(kind, 1.0), kind, False, np.concatenate([edge, [[5.0, 1.0, 1.0]]]).astype(np.float32), np.repeat(M.SPD[None], 2, axis=0))
    rec = _records(c, kind)
    assert (int(lim) - 1, 0, 0) in rec and len(rec) == 2
    pts = np.array([[lim, 1.0, 1.0], [lim + 1.0, 1.0, 1.0], [lim - 1.0, 1.0, 1.0], [-lim + 2.0, 1.0, 1.0], [-lim + 1.0, 1.0, 1.0]], np.float32)  # cells lim - 1, lim (skipped), lim - 2, -lim + 1, -lim (skipped)
    for nb, found in ((capi.DIRECT1, [1, -1, 0, 0, -1]), (capi.DIRECT7, [1, -1, 1, 0, -1]), (capi.DIRECT27, [1, -1, 1, 0, -1])):
        got = c.map_score(None, xyz=pts, neighbors=nb, per_point=True)
        _check(got, M.score(rec, 1.0, pts, None, nb, 1, M.INF, 1.0), "%s index edge nb=%d" % (kind, nb))
        assert got["found"].tolist() == found and got["n_used"] == 3
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_a_batch_table_that_overflowed_is_rebuilt_before_it_is_scored(kind, scene):
    """a hint of 8 voxels for a map of 100: the build drops points, which nobody has noticed when the score is asked for -- the call rebuilds
    the map at the safe size, as align and the getters do, and scores that"""
    from fast_gicp_amd import capi
    res, T, pts = scene["res"], scene["pose"], scene["scan"][:257]
    c = _build(_handle(kind, res), kind, True, scene["map_points"], scene["map_covs"], hint=8)
    got = c.map_score(T, xyz=pts, neighbors=capi.DIRECT27, max_m2=MAX_M2, per_point=True)
    rec = _records(c, kind)
    assert len(rec) == 100
    _check(got, M.score(rec, res, pts, T, capi.DIRECT27, 1, MAX_M2, 1.0), kind + " after an overflow")
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_every_route_to_the_same_points_gives_the_same_bits(kind, scene):
    """_source before and after the source gets a Morton order, _cloud from the host, from the device and at stride 4; with and without the
    per-point arrays; twice"""
    import torch
    from fast_gicp_amd import capi
    res, T = scene["res"], scene["pose"]
    pts = np.ascontiguousarray(scene["scan"][M.SPECIAL_ROWS:])  # finite rows only: the cloud is sorted below
    c = _build(_handle(kind, res), kind, False, scene["map_points"], scene["map_covs"])
    args = dict(neighbors=capi.DIRECT27, min_points=1, max_m2=MAX_M2, score_scale=0.5)
    ref_out = c.map_score(T, xyz=pts, per_point=True, **args)
    _check(ref_out, M.score(_records(c, kind), res, pts, T, capi.DIRECT27, 1, MAX_M2, 0.5), kind + " host cloud")
    outs = {"host cloud again": c.map_score(T, xyz=pts, per_point=True, **args), "host cloud, no rows": c.map_score(T, xyz=pts, **args)}
    d3 = torch.from_numpy(pts).cuda()
    p4 = np.zeros((len(pts), 4), np.float32); p4[:, :3] = pts; p4[:, 3] = np.nan
    d4 = torch.from_numpy(p4).cuda()
    torch.cuda.synchronize()
    outs["device cloud"] = c.map_score(T, device_ptr=d3.data_ptr(), n=len(pts), stride=3, per_point=True, **args)
    outs["device cloud, stride 4"] = c.map_score(T, device_ptr=d4.data_ptr(), n=len(pts), stride=4, per_point=True, **args)
    c.set_source_cloud(pts)
    outs["source, input order"] = c.map_score(T, per_point=True, **args)
    outs["source, no rows"] = c.map_score(T, **args)
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
    c.profile_enable(False)
    assert sorts >= (2 if kind == "ndt" else 1), sorts
    outs["source, Morton order"] = c.map_score(T, per_point=True, **args)
    outs["source, Morton order, no rows"] = c.map_score(T, **args)
    for what, got in outs.items():
        _same_struct(got, ref_out, kind + " " + what)
        if "found" in got:
            assert np.array_equal(got["found"], ref_out["found"]) and np.array_equal(got["best"], ref_out["best"]), what
            assert np.array_equal(_bits(got["best_m2"]), _bits(ref_out["best_m2"])), what
    after = c.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_the_call_leaves_the_handle_as_it_was(kind, scans):
    """export byte-equal, stored correspondences unchanged, compute_error and align after a score give the bits they gave without one, and a score
    between prepare_source_device and adopt_prepared_source leaves the prepared pipeline's pose bit-identical"""
    from fast_gicp_amd import capi
    tgt, src, T = scans["tgt"], scans["src"], scans["T"]

    def fresh():
        c = _build(_handle(kind, 1.0), kind, False, tgt, scans["Ct"])
        c.set_neighbor_search_method(capi.DIRECT7)
        if kind == "ndt":
            c.set_source_cloud(src)
        else:
            c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
        return c

    def score(c, **kw):
        return c.map_score(T, neighbors=capi.DIRECT27, min_points=2, max_m2=9.0, **kw)

    a, b = fresh(), fresh()
    before, info = a.map_export(), a.map_info()
    for c in (a, b):
        c.update_correspondences(T)
    corr = a.get_voxel_correspondences().copy()
    s1 = score(a, per_point=True)
    s2 = score(a, xyz=src[:500])
    assert s1["n_near"] > 0 and s2["n_points"] == 500
    assert np.array_equal(a.get_voxel_correspondences(), corr)
    ea, eb = a.compute_error(T), b.compute_error(T)  # (the linearisation pose and the stored correspondences are what compute_error reads)
    assert ea[0] == eb[0] and ea[1].tobytes() == eb[1].tobytes() and ea[2].tobytes() == eb[2].tobytes()
    after = a.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert a.map_info() == info
    ra = a.align(T)
    score(a)
    ra2 = a.align(T)
    rb = b.align(T)
    assert ra["T"].tobytes() == rb["T"].tobytes() == ra2["T"].tobytes() and ra["nr_iterations"] == rb["nr_iterations"] == ra2["nr_iterations"]
    # between prepare_source_device and adopt_prepared_source
    import torch
    d_src = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    for c, with_score in ((a, True), (b, False)):
        c.prepare_source_device(d_src.data_ptr(), len(src), 3)
        if with_score:
            s3 = score(c, xyz=src, per_point=True)
            _same_struct(s3, s1, "score beside a preparation")
        c.adopt_prepared_source()
    pa, pb = a.align(T), b.align(T)
    assert pa["T"].tobytes() == pb["T"].tobytes() and pa["nr_iterations"] == pb["nr_iterations"]
    a.close(); b.close()


def _raw_tail(T=None, neighbors=1, min_points=1, max_m2=9.0, score_scale=1.0, out=True):
    from fast_gicp_amd import capi
    t = np.ascontiguousarray(np.eye(4)) if T is None or T is False else capi._colmajor16(T)
    s = capi.MapScore()
    keep = (t, s)
    return keep, (None if T is False else capi._p(t), int(neighbors), int(min_points), C.c_double(max_m2), C.c_double(score_scale), C.byref(s) if out else None, None, None, None)


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_every_refusal_is_followed_by_a_call_that_works(kind, scene, scans):
    from fast_gicp_amd import capi
    res, T, pts = scene["res"], scene["pose"], np.ascontiguousarray(scene["scan"][M.SPECIAL_ROWS:200])
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
    refused(c, BAD_STATE, "no target voxel map", "score_source", *a)
    refused(c, BAD_STATE, "no target voxel map", "score_cloud", *cloud, *a)
    if kind != "ndt":  # (a handle with map sharding on cannot hold an incremental map: asked before one is live)
        c.set_target_map_sharding(True)
        refused(c, UNSUPPORTED, "multi-GPU", "score_source", *a)
        refused(c, UNSUPPORTED, "multi-GPU", "score_cloud", *cloud, *a)
        c.set_target_map_sharding(False)
    _build(c, kind, False, scene["map_points"], scene["map_covs"])
    rec = _records(c, kind)
    want = M.score(rec, res, pts, T, capi.DIRECT7, 1, 9.0, 1.0)

    def works():
        _check(c.map_score(T, xyz=pts, neighbors=capi.DIRECT7, max_m2=9.0, per_point=True), want, kind + " after a refusal", sums=False)

    works()
    refused(c, BAD_STATE, "source cloud is not set", "score_source", *a)
    works()
    c.set_source_cloud(pts)
    bad_T = np.eye(4); bad_T[2, 3] = np.nan
    table = [("finite", dict(T=bad_T)), ("null pose", dict(T=False)), ("null result", dict(out=False)), ("neighbors", dict(neighbors=capi.DIRECT_RADIUS)), ("neighbors", dict(neighbors=7)),
             ("neighbors", dict(neighbors=-1)), ("max_m2", dict(max_m2=float("nan"))), ("max_m2", dict(max_m2=-1.0)), ("score_scale", dict(score_scale=0.0)),
             ("score_scale", dict(score_scale=-2.0)), ("score_scale", dict(score_scale=float("inf"))), ("score_scale", dict(score_scale=float("nan")))]
    for word, kw in table:
        keep, bad = _raw_tail(**kw)
        refused(c, BAD_ARG, word, "score_source", *bad)
        refused(c, BAD_ARG, word, "score_cloud", *cloud, *bad)
        works()
    refused(c, BAD_ARG, "n < 0", "score_cloud", capi._p(pts), -1, 3, 0, *a)
    refused(c, BAD_ARG, "null points", "score_cloud", None, 5, 3, 0, *a)
    refused(c, BAD_ARG, "stride", "score_cloud", capi._p(pts), len(pts), 5, 0, *a)
    refused(c, BAD_ARG, "stride", "score_cloud", capi._p(pts), len(pts), 2, 1, *a)
    works()
    # n == 0 and max_m2 = +inf are legal
    keep, ok = _raw_tail(max_m2=float("inf"))
    fn = getattr(c._lib, prefix + "score_cloud"); fn.restype = C.c_int
    assert fn(c.h, None, 0, 3, 0, *ok) == 0 and keep[1].n_points == 0 and keep[1].sum_score_all == 0.0
    # an align_async in flight
    c.close()
    c = _build(_handle(kind, 1.0), kind, False, scans["tgt"], scans["Ct"])
    c.set_neighbor_search_method(capi.DIRECT7)
    if kind == "ndt":
        c.set_source_cloud(scans["src"])
    else:
        c.set_source_cloud(scans["src"]); c.find_source_neighbors(20); c.calculate_source_covariances()
    before = c.map_export()
    c.align_async(scans["T"])
    refused(c, BAD_STATE, "align_async", "score_source", *a)
    refused(c, BAD_STATE, "align_async", "score_cloud", *cloud, *a)
    c.align_wait()
    got = c.map_score(scans["T"], neighbors=capi.DIRECT7, max_m2=9.0, per_point=True)
    _check(got, M.score(_records(c, kind), 1.0, scans["src"], scans["T"], capi.DIRECT7, 1, 9.0, 1.0), kind + " after align_wait")
    after = c.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    c.close()


def test_pygicp_and_the_cpp_class_give_what_the_c_abi_gives(scans):
    """pygicp.score_target goes through DeviceRegistration::scoreTarget: on an NDT map (points only: both routes build the same map) the
    result equals capi.map_score to the bit; on a VGICP map the rows are consistent with the counts"""
    import pygicp
    from fast_gicp_amd import capi
    t, s, T = scans["tgt"], scans["src"], scans["T"]
    T = T.astype(np.float32).astype(np.float64)  # (the C++ classes take a float pose)
    c = _build(_handle("ndt", 1.0), "ndt", False, t, None)
    c.set_source_cloud(s)
    want = c.map_score(T, neighbors=capi.DIRECT27, min_points=2, max_m2=9.0, score_scale=0.5, per_point=True)
    c.close()
    reg = pygicp.NDTCudaMap()
    reg.set_resolution(1.0)
    reg.begin_incremental_target()
    reg.set_input_source(t.astype(np.float64)); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s.astype(np.float64))
    got = reg.score_target(T, neighbors=capi.DIRECT27, min_points=2, max_m2=9.0, score_scale=0.5, per_point=True)
    _same_struct(got, want, "pygicp NDT")
    assert np.array_equal(got["found"], want["found"]) and np.array_equal(got["best"], want["best"]) and np.array_equal(_bits(got["best_m2"]), _bits(want["best_m2"]))
    assert got["overlap"] == want["overlap"] and got["nvtl"] == want["nvtl"] and got["tp"] == want["tp"]
    reg = pygicp.FastVGICPCuda()
    reg.set_resolution(1.0)
    reg.begin_incremental_target()
    reg.set_input_source(t.astype(np.float64)); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s.astype(np.float64))
    got = reg.score_target(T, per_point=True)
    assert got["n_points"] == len(s) == len(got["found"]) and got["n_used"] == int((got["found"] >= 0).sum()) and got["n_near"] == int((got["found"] > 0).sum()) > 0
    assert 0 < got["n_in_voxel"] <= got["n_near"] and got["n_in_voxel"] >= int((got["best"] == 0).sum())  # (DIRECT7: offset 0 is the point's own voxel)
    assert "found" not in reg.score_target(T)
    with pytest.raises(Exception):
        reg.score_target(T, neighbors=capi.DIRECT_RADIUS)
