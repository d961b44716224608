"""Free-space carving on the incremental map (fvh_vgicp_clear_rays_* / fvh_ndt_clear_rays_*) against the twin of its contract.

Every case exports the map, makes the call and exports again: the second export must be tests/clearrays_ref.py applied to the first -- the same
key set, the survivors' ten sums and ages bit for bit -- and the two counts the twin's. Equality, not a tolerance: the walk is single fp64
operations, which the device rounds as Python does. The one place where the two could differ is HOW the fp64 sum R p + t is formed before it
is rounded to float32 (the device compiler may contract it); the poses here are either exact in fp64 (identity, dyadic shifts) or checked
by clearrays_ref.rounding_is_stable, which says that no float32 rounding of the case can depend on it.
(tests/test_map_clear_rays_cpu.py holds the twin itself to geometry.)"""
import ctypes as C

import numpy as np
import pytest

from tests import clearrays_ref as ref
from tests import table_sim
from tests import util

pytestmark = pytest.mark.gpu

KINDS = ("additive", "multiplicative", "ndt")
POSE_TOL = 1e-9  # tests/test_gpu_incremental_map.py: what a rehashed (pruned) map's registration is held to
BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4
MIN_CAPACITY = 64  # INCMAP_MIN_CAPACITY


def _handle(kind, res, **params):
    from fast_gicp_amd import capi
    if kind == "ndt":
        c = capi.NDTMapCore(0)
        c.set_distance_mode(capi.NDT_D2D)
    else:
        c = capi.VGICPMapCore(0)
        c.set_voxel_accumulation_mode(capi.VOXEL_MULTIPLICATIVE if kind == "multiplicative" else capi.VOXEL_ADDITIVE)
    if params:
        c.set_engine_params(**params)
    c.set_resolution(res)
    c.set_neighbor_search_method(capi.DIRECT7)
    return c


def _covs(n):
    """n small symmetric positive definite covariances, float32-exact"""
    base = np.array([[0.03125, 0.0078125, 0.0], [0.0078125, 0.0625, 0.00390625], [0.0, 0.00390625, 0.046875]])
    return np.repeat(base[None], n, axis=0)


def _insert(c, kind, pts):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    if kind == "ndt":
        c.map_insert_cloud(pts)
    else:
        c.map_insert_cloud(pts, _covs(len(pts)))
    assert c.map_info()["dropped"] == 0


def _centres(coords, res):
    """one float32 point per voxel: its centre (c + 1) * res, which floor(x / res - 0.5) puts in voxel c"""
    return ((np.asarray(coords, np.float64) + 1.0) * res).astype(np.float32)


def _map_of(kind, res, coords, expected_voxels=0, **params):
    c = _handle(kind, res, **params)
    c.map_begin(expected_voxels)
    _insert(c, kind, _centres(coords, res))
    assert c.map_info()["num_voxels"] == len({tuple(v) for v in np.asarray(coords).tolist()})
    return c


def _same_map(got, want, what):
    assert got["coords"].shape == want["coords"].shape and np.array_equal(got["coords"], want["coords"]), "%s: key sets differ (%d vs %d voxels)" % (what, len(got["coords"]), len(want["coords"]))
    assert got["sums"].tobytes() == np.ascontiguousarray(want["sums"]).tobytes(), what + ": sums differ"
    assert np.array_equal(got["ages"], want["ages"]), what + ": ages differ"
    for k in ("resolution", "mode", "num_inserts", "num_points"):
        assert got[k] == want[k], (what, k)


def _call_and_check(c, what, twin_points, **kw):
    """export, call, export: the twin applied to the first export. kw: the arguments of map_clear_rays. -> (before, after, removed, used)"""
    before = c.map_export()
    twin_kw = {k: v for k, v in kw.items() if k in ("T", "origin", "min_range", "max_range", "end_margin", "min_misses")}
    want, want_removed, want_used = ref.clear_rays(before, twin_points, **twin_kw)
    removed, used = c.map_clear_rays(**kw)
    after = c.map_export()
    print("%s: %d voxels, %d rays used, %d removed (twin: %d used, %d removed)" % (what, before["num_voxels"], used, removed, want_used, want_removed))
    _same_map(after, want, what)
    assert (removed, used) == (want_removed, want_used), what
    assert c.map_info()["num_voxels"] == want["num_voxels"] and c.map_info()["dropped"] == 0
    return before, after, removed, used


def _records(c, kind):
    coords, num, means, covs = (np.asarray(a) for a in (c.get_voxelmap("target") if kind == "ndt" else c.get_voxelmap()))
    o = np.lexsort(coords.T[::-1]) if len(coords) else np.zeros(0, np.int64)
    return {tuple(k): (int(n), m.tobytes(), v.tobytes()) for k, n, m, v in zip(coords[o].tolist(), num[o], means[o], covs[o])}


@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("kind", KINDS)
def test_one_axis_aligned_ray_through_a_row_of_voxels(kind, res):
    """voxels (-3..5, -1, -1): r is 8 voxels and every entry time a multiple of 1/16. The ray runs from the centre of the first to the centre
    of the last: d == 0 on two axes, the origin inside an occupied voxel, negative coordinates. end_margin beyond r, 3.5 voxels, half a voxel, zero."""
    row = np.array([[x, -1, -1] for x in range(-3, 6)], np.int32)
    c = _map_of(kind, res, row)
    o, p = _centres(row[:1], res)[0], _centres(row[-1:], res)
    r = 8.0 * res
    _, after, removed, used = _call_and_check(c, "margin > r", p, xyz=p, origin=o, end_margin=r + res)
    assert (removed, used) == (0, 1)
    _, after, removed, used = _call_and_check(c, "margin 3.5 voxels", p, xyz=p, origin=o, end_margin=3.5 * res)
    assert (removed, used) == (5, 1) and after["coords"][:, 0].tolist() == [2, 3, 4, 5]  # t_end = 0.5625, exactly where cell 2 is entered: not before it
    c.map_begin()
    _insert(c, kind, _centres(row, res))
    _, after, removed, used = _call_and_check(c, "margin half a voxel", p, xyz=p, origin=o, end_margin=0.5 * res)
    assert (removed, used) == (8, 1) and after["coords"].tolist() == [[5, -1, -1]]  # the walk stops at the face of the endpoint's voxel
    c.map_begin()
    _insert(c, kind, _centres(row, res))
    _, after, removed, used = _call_and_check(c, "margin 0", p, xyz=p, origin=o)
    assert (removed, used) == (8, 1) and after["coords"].tolist() == [[5, -1, -1]]  # crossed and hit: the endpoint's voxel stays
    # the same ray backwards along -x, ending in an EMPTY cell beyond the row's first voxel: nothing is protected
    c.map_begin()
    _insert(c, kind, _centres(row[1:], res))
    _, after, removed, used = _call_and_check(c, "endpoint voxel absent", _centres(row[:1], res), xyz=_centres(row[:1], res), origin=p[0])
    assert (removed, used) == (8, 1) and after["num_voxels"] == 0
    c.close()


@pytest.mark.parametrize("res", [1.0, 0.5])
def test_corner_diagonals_on_dyadic_coordinates(res):
    """a 5 x 5 x 5 block of voxels around the origin; rays between points whose coordinates are multiples of 1/8 that pass exactly through cell
    corners and edges: from the first two origins every operation of the walk with no margin is exact and every tie is a real one (x
    before y before z)"""
    block = np.array([[x, y, z] for x in range(-2, 3) for y in range(-2, 3) for z in range(-2, 3)], np.int32)
    ends = np.array([[3, 3, 3], [-1, -1, -1], [3, 3, 1], [3, 1, 3], [1, 3, 3], [-1, 3, 3], [3, -1, 1], [2.5, 2.5, 2.5], [3, 2, 1.5]], np.float64) * res
    for k, o in enumerate(([1.0 * res] * 3, [0.5 * res] * 3, [0.625, 0.625, 0.625])):  # a cell centre, a cell corner, an off-centre dyadic point
        for margin in (0.0, 0.25):
            c = _map_of("additive", res, block)
            before, after, removed, used = _call_and_check(c, "diagonals from %s margin %g" % (o, margin), ends.astype(np.float32), xyz=ends.astype(np.float32), origin=o, end_margin=margin)
            assert used == len(ends) and 0 < removed < len(block)
            c.close()


def _random_case(seed, n_vox, n_rays, res):
    """n_vox distinct voxels in a 13^3 box, n_rays endpoints in a slightly larger one, a general rigid pose and an origin off the lattice"""
    rng = np.random.default_rng(seed)
    cells = np.array([[x, y, z] for x in range(-6, 7) for y in range(-6, 7) for z in range(-6, 7)], np.int32)
    vox = cells[rng.choice(len(cells), n_vox, replace=False)]
    ang = 0.3
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.31 * res, -0.17 * res, 0.23 * res]
    pts = rng.uniform(-7.5 * res, 7.5 * res, (n_rays, 3)).astype(np.float32)
    origin = [0.11 * res, 0.07 * res, -0.05 * res]
    assert ref.rounding_is_stable(T, pts, origin)
    return vox, T, pts, origin


@pytest.mark.parametrize("kind", KINDS)
def test_a_thousand_rays_in_a_table_that_grew_by_rehash(kind):
    """1,000 rays = four workgroups, the last one ragged; 300 voxels in a table that started at the smallest capacity: the live side is 1"""
    res = 0.5
    vox, T, pts, origin = _random_case(3, 300, 1000, res)
    c = _map_of(kind, res, vox, expected_voxels=1)
    rec0 = _records(c, kind)
    assert c.map_info()["capacity"] > MIN_CAPACITY
    before, after, removed, used = _call_and_check(c, "%s, grown table" % kind, pts, T=T, xyz=pts, origin=origin, max_range=100.0)
    assert used == 1000 and 0 < removed < 300
    rec1 = _records(c, kind)  # the survivors' records too, bit for bit
    assert set(rec1) == {tuple(v) for v in after["coords"].tolist()} and all(rec1[k] == rec0[k] for k in rec1)
    # a second call with a range window and a margin on what is left
    _call_and_check(c, "%s, range window" % kind, pts, T=T, xyz=pts, origin=origin, min_range=1.0, max_range=3.0, end_margin=0.75 * res)
    c.close()


@pytest.mark.parametrize("n_vox,expected", [(300, 150), (256, 128)])
def test_a_thousand_rays_in_a_crowded_table(n_vox, expected):
    """the fullest tables the host keeps: 300 voxels need 1,024 buckets (load 0.29); 256 voxels inserted in two halves stay in 512 (load 0.5,
    the limit -- one more point and the insert grows the table). Probe runs are long there and one crosses the table's end."""
    res = 1.0
    seed = {300: 1, 256: 15}[n_vox]  # (seeds whose voxel sets put a probe run across the table's end: asserted below)
    vox, T, pts, origin = _random_case(seed, n_vox, 1000, res)
    c = _handle("additive", res)
    c.map_begin(expected)
    half = n_vox // 2
    _insert(c, "additive", _centres(vox[:half], res)); _insert(c, "additive", _centres(vox[half:], res))
    info = c.map_info()
    assert info["num_voxels"] == n_vox and info["capacity"] == 4 * {150: 256, 128: 128}[expected]
    sim = table_sim.fill_table(vox, info["capacity"])
    print("table: load %.2f, longest run %d, runs across the end %d" % (sim["load"], sim["longest_run"], sim["across_end"]))
    assert sim["across_end"] > 0
    _, _, removed, used = _call_and_check(c, "crowded table %d / %d" % (n_vox, info["capacity"]), pts, T=T, xyz=pts, origin=origin)
    assert used == 1000 and 0 < removed < n_vox and c.map_info()["capacity"] == info["capacity"]
    c.close()


def test_min_misses_counts_the_rays_of_one_call():
    """three rows of voxels along +x, +y and +z from voxel (0, 0, 0), whose centre is the origin of every ray; the ray along axis j is sent
    j + 1 times: min_misses = k removes the voxels crossed at least k times"""
    res = 1.0
    unit = np.eye(3, dtype=np.int32)
    rows = np.concatenate([np.zeros((1, 3), np.int32)] + [unit[j][None] * np.arange(1, 6)[:, None] for j in range(3)])
    o = _centres([[0, 0, 0]], res)[0]
    ends = np.concatenate([np.repeat(_centres([5 * unit[j]], res), j + 1, axis=0) for j in range(3)])
    for k in (1, 2, 3, 4):
        c = _map_of("additive", res, rows)
        _, after, removed, used = _call_and_check(c, "min_misses %d" % k, ends, xyz=ends, origin=o, min_misses=k)
        assert used == 6
        left = {tuple(v) for v in after["coords"].tolist()}
        assert (0, 0, 0) not in left  # crossed by all six rays
        for j in range(3):  # a row's last voxel is hit and stays; the one before it is crossed by the j + 1 copies of its own ray only
            assert tuple(5 * unit[j]) in left
            assert (tuple(4 * unit[j]) in left) == (j + 1 < k), (k, j)
        c.close()


def test_a_voxel_crossed_and_hit_in_one_call_survives():
    res = 0.5
    row = np.array([[x, 0, 0] for x in range(8)], np.int32)
    c = _map_of("ndt", res, row)
    o = _centres([[0, 0, 0]], res)[0]
    ends = _centres([[7, 0, 0], [3, 0, 0]], res)  # the long ray crosses voxel 3, the short one ends in it
    _, after, removed, used = _call_and_check(c, "crossed and hit", ends, xyz=ends, origin=o)
    assert used == 2 and after["coords"][:, 0].tolist() == [3, 7] and removed == 6
    c.close()


def test_skipped_rays_are_not_counted():
    res = 1.0
    row = np.array([[x, 0, 0] for x in range(10)], np.int32)
    c = _map_of("additive", res, row)
    o = [1.0, 1.0, 1.0]
    good = _centres([[9, 0, 0]], res)[0]
    pts = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1, 1, 1],     # non-finite coordinates; p' == o'
                    [3, 1, 1], [8, 1, 1], good], np.float32)                        # r = 2 < min_range, r = 7 > max_range, r = 9... see below
    _, after, removed, used = _call_and_check(c, "range window", pts, xyz=pts, origin=o, min_range=2.5, max_range=6.5)
    assert (removed, used) == (0, 0)
    _, after, removed, used = _call_and_check(c, "inclusive bounds", pts, xyz=pts, origin=o, min_range=2.0, max_range=7.0)
    assert used == 2 and after["coords"][:, 0].tolist() == [2, 7, 8, 9]  # the rays to x = 3 and x = 8 (cells 2 and 7)
    # a point whose cell is beyond |c| < 2^20 - 4096, reached by a short ray from an origin just inside: skipped for its index, not its range
    far = float(ref.LIM)
    c.map_begin()
    _insert(c, "additive", np.array([[far - 2.0, 1.0, 1.0]], np.float32))
    pts = np.array([[far + 2.0, 1.0, 1.0], [far - 1.0, 1.0, 1.0]], np.float32)
    _, after, removed, used = _call_and_check(c, "beyond the key range", pts, xyz=pts, origin=[far - 4.0, 1.0, 1.0], max_range=50.0)
    assert (removed, used) == (1, 1)
    c.close()


def test_every_route_to_the_same_rays_gives_the_same_map():
    """_source without and with a Morton order, _cloud from the host and from the device at stride 3 and 4"""
    import torch
    res = 0.5
    vox, T, pts, origin = _random_case(21, 300, 1000, res)
    kw = dict(T=T, origin=origin, end_margin=0.5 * res)
    want = None
    dev = torch.device("cuda", 0)
    d3 = torch.from_numpy(pts).to(dev).contiguous()
    pts4 = np.concatenate([pts, np.full((len(pts), 1), 7.0, np.float32)], axis=1)
    d4 = torch.from_numpy(pts4).to(dev).contiguous()
    torch.cuda.synchronize()
    routes = [("source", {}), ("source, Morton order", dict(coherent_min_points=1)), ("cloud host", {}), ("cloud device stride 3", {}), ("cloud device stride 4", {})]
    for name, params in routes:
        c = _map_of("additive", res, vox, **params)
        call = dict(kw)
        if name.startswith("source"):
            c.set_source_cloud(pts)
            if params:
                c.find_source_neighbors(10)  # (the search sorts the cloud: the Morton order exists from here on)
        elif name == "cloud host":
            call["xyz"] = pts
        else:
            call.update(device_ptr=(d3 if name.endswith("3") else d4).data_ptr(), n=len(pts), stride=3 if name.endswith("3") else 4)
        _, after, removed, used = _call_and_check(c, name, pts, **call)
        if want is None:
            want = (after, removed, used)
        _same_map(after, want[0], name)
        assert (removed, used) == want[1:] and removed > 0
        c.close()
    n = _handle("ndt", res)
    n.map_begin()
    _insert(n, "ndt", _centres(vox, res))
    n.set_source_cloud(pts)
    _, after, removed, used = _call_and_check(n, "ndt source", pts, **kw)
    assert np.array_equal(after["coords"], want[0]["coords"]) and (removed, used) == want[1:]
    n.close()


def test_a_call_that_removes_nothing_leaves_the_map_untouched():
    res = 1.0
    vox, T, pts, origin = _random_case(33, 300, 200, res)
    c = _map_of("additive", res, vox, expected_voxels=1)
    src = _centres(vox[:64], res)
    c.set_source_cloud(src); c.set_source_covariances(_covs(len(src)))
    c.update_correspondences(np.eye(4))
    ncorr = c.get_num_correspondences()
    assert ncorr > 0
    info, before = c.map_info(), c.map_export()
    c.profile_enable(True); c.profile_reset()
    removed, used = c.map_clear_rays(T, xyz=pts, origin=origin, min_misses=len(pts) + 1)  # no voxel can collect that many misses
    c.synchronize()
    assert removed == 0 and used == len(pts)
    assert c.profile_get("map_rehash")[1] == 0 and c.profile_get("map_raymark")[1] == 1 and c.profile_get("map_raysweep")[1] == 1
    after = c.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert c.map_info() == info
    assert c.get_num_correspondences() == ncorr
    # n == 0: FVH_OK, nothing removed, nothing queued
    c.profile_reset()
    assert c.map_clear_rays(T, xyz=np.zeros((0, 3), np.float32)) == (0, 0)
    assert c.profile_get("map_raymark")[1] == 0 and c.get_num_correspondences() == ncorr
    # ... and a call that does remove: one rehash, at the same capacity, and the stored correspondences are gone
    c.profile_reset()
    removed, used = c.map_clear_rays(T, xyz=pts, origin=origin)
    c.synchronize()
    assert removed > 0 and c.profile_get("map_rehash")[1] == 1 and c.map_info()["capacity"] == info["capacity"]
    assert c.map_info()["num_inserts"] == info["num_inserts"] and c.map_info()["num_points"] == info["num_points"]
    c.profile_enable(False)
    c.close()


@pytest.fixture(scope="module")
def scans():
    """the bundled pair, the engine's own covariances of both scans, the pose between them"""
    tgt, src = util.bundled_pair()
    c = _handle("additive", 1.0)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
    Ct, Cs = c.get_covariances("target").astype(np.float64), c.get_covariances("source").astype(np.float64)
    c.close()
    return dict(tgt=tgt, src=src, Ct=Ct, Cs=Cs, T=util.relative_pose())


def test_align_after_a_removal_equals_align_on_the_surviving_rows(scans):
    """the map of the first scan, cleared along every 16th ray of the second at the pose between them (identity rotation would be exact; this
    pose is not, so the rays are screened), then align: the pose and iteration count of a fresh handle that imported the surviving rows"""
    a = _handle("additive", 1.0)
    a.map_begin()
    a.map_insert_cloud(scans["tgt"], scans["Ct"])
    rays = np.ascontiguousarray(scans["src"][::16])
    assert ref.rounding_is_stable(scans["T"], rays)
    _, after, removed, used = _call_and_check(a, "bundled scan", rays, T=scans["T"], xyz=rays, end_margin=2.0, min_misses=3, max_range=100.0)
    assert removed > 0 and used == len(rays)
    b = _handle("additive", 1.0)
    b.map_begin()
    b.map_import(after)
    out = []
    for c in (a, b):
        c.set_source_cloud(scans["src"]); c.set_source_covariances(scans["Cs"])
        out.append(c.align())
    ra, rb = out
    print("align after clear_rays vs fresh import: rel_err %.3g, iterations %d / %d" % (util.rel_err(ra["T"], rb["T"]), ra["nr_iterations"], rb["nr_iterations"]))
    assert ra["converged"] and rb["converged"] and ra["nr_iterations"] == rb["nr_iterations"]
    assert util.rel_err(ra["T"], rb["T"]) <= POSE_TOL
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_a_box_in_front_of_a_wall_is_carved_away(kind):
    """scan 1 sees a wall and a box in front of it; scan 2, from the same pose, sees only the wall (the box has left): after clear_rays the
    box's voxels are gone and every wall voxel is still there -- then the second scan is inserted, as the loop does it"""
    res = 0.5
    sensor = [0.0, 0.0, 1.0]
    ys, zs = np.arange(-3.0, 3.01, 0.125), np.arange(0.125, 3.0, 0.125)
    wall = np.array([[10.0, y, z] for y in ys for z in zs], np.float32)
    box = np.array([[4.0 + dx, y, z] for dx in (0.0, 0.25, 0.5) for y in np.arange(-0.5, 0.51, 0.125) for z in np.arange(0.375, 1.5, 0.125)], np.float32)  # (above the lowest ray: every box voxel is seen through)
    c = _handle(kind, res)
    c.map_begin()
    _insert(c, kind, np.concatenate([wall, box]))
    before = c.map_export()
    is_box = before["coords"][:, 0] < 12
    assert 0 < is_box.sum() < len(is_box)
    _, after, removed, used = _call_and_check(c, "wall and box, " + kind, wall, xyz=wall, origin=sensor, end_margin=res, max_range=50.0)
    assert removed == int(is_box.sum()) and used == len(wall)
    assert np.array_equal(after["coords"], before["coords"][~is_box])
    _insert(c, kind, wall)
    assert c.map_info()["num_voxels"] == int((~is_box).sum()) and c.map_info()["num_inserts"] == 2
    c.close()


def test_the_bitmap_changes_nothing():
    res = 0.5
    vox, T, pts, origin = _random_case(41, 300, 1000, res)
    origin2 = [2.3 * res, -1.7 * res, 0.9 * res]
    assert ref.rounding_is_stable(T, pts[:0], origin2)
    out = []
    for params in (dict(bitmap_min_points=1), dict()):
        c = _map_of("multiplicative", res, vox, **params)
        _, after, removed, used = _call_and_check(c, "bitmap %s" % bool(params), pts, T=T, xyz=pts, origin=origin)
        # once more on the rehashed map (its bitmap was rebuilt by the rehash), from another origin and with a margin
        _, after2, removed2, used2 = _call_and_check(c, "bitmap %s, second call" % bool(params), pts, T=T, xyz=pts, origin=origin2, end_margin=0.25)
        out.append((after, removed, used, after2, removed2, used2))
        c.close()
    _same_map(out[0][0], out[1][0], "bitmap on vs off")
    _same_map(out[0][3], out[1][3], "bitmap on vs off, second call")
    assert out[0][1:3] == out[1][1:3] and out[0][4:] == out[1][4:] and out[0][1] > 0 and out[0][4] > 0


def _raw_args(T=None, origin=None, min_range=0.0, max_range=50.0, end_margin=0.0, min_misses=1):
    from fast_gicp_amd import capi
    t = np.ascontiguousarray(np.eye(4)) if T is None else capi._colmajor16(T)
    o = None if origin is None else np.ascontiguousarray(origin, np.float64)
    keep = (t, o)
    return keep, (None if T is False else capi._p(t), None if o is None else capi._p(o), C.c_double(min_range), C.c_double(max_range), C.c_double(end_margin), int(min_misses), None, None)


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_refusals_leave_the_map_and_the_handle_as_they_were(kind, scans):
    from fast_gicp_amd import capi
    res = 1.0
    prefix = "fvh_ndt_" if kind == "ndt" else "fvh_vgicp_"
    vox, T, pts, origin = _random_case(55, 300, 100, res)

    def refused(c, code, word, name, *args):
        fn = getattr(c._lib, prefix + name)
        fn.restype = C.c_int
        rc = fn(c.h, *args)
        msg = getattr(c._lib, prefix + "last_error")(c.h).decode()
        assert rc == code and word in msg, (name, rc, msg)

    def source_args(**kw):
        keep, a = _raw_args(**kw)
        return a + (keep,)  # (the trailing tuple keeps the arrays alive; refused() drops it)

    # no live map; a multi-GPU handle; CUDA-compat arithmetic: refused before anything else (none of them can hold a live map)
    c = _handle(kind, res)
    keep, a = _raw_args()
    refused(c, BAD_STATE, "map_begin", "clear_rays_source", *a)
    refused(c, BAD_STATE, "map_begin", "clear_rays_cloud", capi._p(pts), len(pts), 3, 0, *a)
    c.set_precision(capi.COMPUTE_CUDA_COMPAT)
    refused(c, UNSUPPORTED, "CUDA_COMPAT", "clear_rays_source", *a)
    c.set_precision(capi.COMPUTE_FP64)
    if kind != "ndt":
        c.set_target_map_sharding(True)
        refused(c, UNSUPPORTED, "sharding", "clear_rays_source", *a)
        c.set_target_map_sharding(False)
    c.map_begin()
    _insert(c, kind, _centres(vox, res))
    before, info = c.map_export(), c.map_info()
    refused(c, BAD_STATE, "source cloud is not set", "clear_rays_source", *a)
    c.set_source_cloud(pts)
    bad_T = np.eye(4); bad_T[1, 3] = np.inf
    cloud = (capi._p(pts), len(pts), 3, 0)
    table = [("finite", dict(T=bad_T)), ("origin", dict(origin=[0.0, np.nan, 0.0])), ("min_range", dict(min_range=-1.0)), ("min_range", dict(min_range=float("nan"))),
             ("max_range", dict(max_range=float("inf"))), ("max_range", dict(min_range=5.0, max_range=4.0)), ("4096", dict(max_range=4096.5 * res)),
             ("end_margin", dict(end_margin=-0.5)), ("end_margin", dict(end_margin=float("inf"))), ("end_margin", dict(end_margin=float("nan"))),
             ("min_misses", dict(min_misses=0))]
    for word, kw in table:
        keep, a = _raw_args(**kw)
        refused(c, BAD_ARG, word, "clear_rays_source", *a)
        refused(c, BAD_ARG, word, "clear_rays_cloud", *cloud, *a)
    keep, a = _raw_args()
    refused(c, BAD_ARG, "null pose", "clear_rays_source", None, *a[1:])
    refused(c, BAD_ARG, "n < 0", "clear_rays_cloud", capi._p(pts), -1, 3, 0, *a)
    refused(c, BAD_ARG, "null points", "clear_rays_cloud", None, 5, 3, 0, *a)
    refused(c, BAD_ARG, "stride", "clear_rays_cloud", capi._p(pts), len(pts), 5, 0, *a)
    # an align_async in flight
    if kind == "ndt":
        c.set_source_cloud(scans["src"])
    else:
        c.set_source_cloud(scans["src"]); c.set_source_covariances(scans["Cs"])
    c.align_async()
    refused(c, BAD_STATE, "align_async", "clear_rays_source", *a)
    refused(c, BAD_STATE, "align_async", "clear_rays_cloud", *cloud, *a)
    c.align_wait()
    after = c.map_export()
    for k in ("coords", "sums", "ages"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert c.map_info() == info
    # the handle is usable: the largest legal max_range, then a call that removes
    assert c.map_clear_rays(T, xyz=pts, origin=origin, max_range=4096.0 * res, min_misses=1000)[0] == 0
    _, _, removed, used = _call_and_check(c, "after the refusals", pts, T=T, xyz=pts, origin=origin)
    assert removed > 0
    c.close()


def test_pygicp_clear_target_rays(scans):
    import pygicp
    t, s = scans["tgt"].astype(np.float64), scans["src"].astype(np.float64)
    for reg in (pygicp.FastVGICPCuda(), pygicp.NDTCudaMap()):
        reg.set_resolution(1.0)
        reg.begin_incremental_target()
        reg.set_input_source(t); reg.insert_source_into_target(np.eye(4))
        reg.set_input_source(s)
        T = reg.align().astype(np.float64)
        assert reg.has_converged()
        removed, used = reg.clear_target_rays(T, min_misses=len(s) + 1)
        assert removed == 0 and 0 < used <= len(s)
        removed2, used2 = reg.clear_target_rays(T, origin=[0.0, 0.0, 0.0], min_range=1.0, max_range=100.0, end_margin=1.0, min_misses=1)
        assert removed2 > 0 and 0 < used2 <= used
        reg.insert_source_into_target()
        reg.align(T)
        assert reg.has_converged()
        with pytest.raises(Exception):
            reg.clear_target_rays(T, min_misses=0)
