"""Incremental target voxel map (fvh_vgicp_map_begin / _insert_source / _insert_cloud / _prune / _get_info) through the C ABI.

Yardstick: the batch route on the same device -- set_target_cloud(P') + set_target_covariances(C') + create_target_voxelmap, itself pinned
to the oracle by the parity tests -- with P', C' formed in numpy as the contract words them (tests/incmap_ref.py: fp64 products, rounded to
float32 once). Voxel sets and point counts must be EQUAL; means and covariances may differ by the order of the fp64 sums only:

    |a - b| <= spacing_float32(entry) + EXCESS * scale          scale: largest |mean| component / largest covariance diagonal of the voxel

One float32 spacing because two fp64 values on either side of a rounding boundary round apart; EXCESS covers entries that are tiny
against their voxel's scale (cancelling off-diagonal sums), where the fp64 error itself shows: n * 2^-52 with n <= 4,096 points per voxel
= 9.1e-13 -> 1e-12 for additive voxels; multiplicative voxels pass the sums through one 3x3 inverse, which amplifies by the condition
number of PLANE-regularised covariances (eigenvalues 1e-3, 1, 1): 1e3 * 9.1e-13 -> 1e-9.
EXCESS is this ANALYTIC bound, not the measured spread, and lies above it (zero was measured for additive voxels; 1.6e-13 and 7.3e-12 in two runs
for multiplicative ones): the order of the atomics differs from run to run, so one measurement is no ceiling. In absolute terms both stay
below the last float bit of the voxel's scale (6e-8).
Measured on an MI355X (every test prints its figures before it asserts). Additive voxels: two BATCH builds of the bundled target are
bit-identical (resolution 1.0 and 0.5), and so is the incremental map against the batch map in every case here (one scan, two scans,
growth, both prunes). Multiplicative voxels: two batch builds differ by up to 7.0e-8 of the voxel's scale on a mean component that is
itself near zero (one spacing of the entry allowed: excess 7.3e-12); incremental vs batch shows the same figure, two scans 9.3e-8 /
excess 1.3e-15; covariances bit-identical.
Poses: the project holds rebuild-vs-rebuild to 1e-9 (relative); the same bound here (measured: 0 in every comparison)."""
import numpy as np
import pytest

from tests import incmap_ref as R
from tests import util

pytestmark = pytest.mark.gpu

EXCESS = {0: 1e-12, 2: 1e-9}
POSE_TOL = 1e-9


def _handle(mode=0, res=1.0, search=None, **params):
    from fast_gicp_amd import capi
    c = capi.VGICPCore(0)
    if params:
        c.set_engine_params(**params)
    c.set_resolution(res)
    c.set_voxel_accumulation_mode(mode)
    c.set_neighbor_search_method(capi.DIRECT7 if search is None else search)
    return c


@pytest.fixture(scope="module")
def scans():
    """bundled pair + the engine's own k-NN covariances (float32) of both scans + the pose of data/relative.txt moved off the voxel faces"""
    tgt, src = util.bundled_pair()
    c = _handle()
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
    Ct, Cs = c.get_covariances("target").copy(), c.get_covariances("source").copy()
    c.close()
    T, k = R.safe_pose(src, util.relative_pose(), (1.0, 0.5))
    print("general pose: relative.txt + %d steps; face margin %.3g / %.3g voxels" % (k, R.face_margin(src, T, 1.0), R.face_margin(src, T, 0.5)))
    return dict(tgt=tgt, src=src, Ct=Ct, Cs=Cs, T=T)


def _batch(c, P, Cov):
    c.set_target_cloud(P); c.set_target_covariances(Cov.astype(np.float64)); c.create_target_voxelmap()


def _insert(c, P, Cov, T=None):
    c.set_source_cloud(P); c.set_source_covariances(Cov.astype(np.float64)); c.map_insert_source(T)
    assert c.map_info()["dropped"] == 0


def _check_equal(got, ref, mode, what):
    s = R.map_spread(got, ref)
    print(what, "voxels", len(ref[0]), s)
    for k in ("mean", "cov"):
        assert s[k + "_excess"] <= EXCESS[mode], (what, k, s)
    return s


def _two_scan_world(scans):
    Ps, Cs = R.transform_cloud(scans["src"], scans["Cs"], scans["T"])
    return np.concatenate([scans["tgt"], Ps]), np.concatenate([scans["Ct"], Cs])


def _insert_two(c, scans):
    _insert(c, scans["tgt"], scans["Ct"])
    _insert(c, scans["src"], scans["Cs"], scans["T"])


@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("mode", [0, 2])
def test_one_scan_identity_pose_equals_batch_map(scans, mode, res):
    a, b, b2 = _handle(mode, res), _handle(mode, res), _handle(mode, res)
    _batch(b, scans["tgt"], scans["Ct"]); _batch(b2, scans["tgt"], scans["Ct"])
    ref = b.get_voxelmap()
    _check_equal(b2.get_voxelmap(), ref, mode, "batch vs batch mode %d res %g:" % (mode, res))  # the yardstick's own spread
    a.map_begin()
    _insert(a, scans["tgt"], scans["Ct"])
    info = a.map_info()
    assert info["incremental"] and info["num_inserts"] == 1 and info["num_points"] == len(scans["tgt"]) and info["num_voxels"] == len(ref[0])
    _check_equal(a.get_voxelmap(), ref, mode, "incremental vs batch mode %d res %g:" % (mode, res))
    # the same cloud through insert_cloud (not the source) into a restarted map
    a.map_begin()
    a.map_insert_cloud(scans["tgt"], scans["Ct"])
    _check_equal(a.get_voxelmap(), ref, mode, "insert_cloud vs batch:")
    for c in (a, b, b2):
        c.close()


@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("mode", [0, 2])
def test_two_scans_general_pose_equal_batch_map_of_concatenation(scans, mode, res):
    assert R.face_margin(scans["src"], scans["T"], res) > 1e-6
    P, Cov = _two_scan_world(scans)
    a, b = _handle(mode, res), _handle(mode, res)
    _batch(b, P, Cov)
    a.map_begin()
    _insert_two(a, scans)
    _check_equal(a.get_voxelmap(), b.get_voxelmap(), mode, "two scans mode %d res %g:" % (mode, res))
    assert a.map_info()["num_points"] == len(P)
    a.close(); b.close()


def test_growth_from_a_tiny_table_drops_nothing(scans):
    P, Cov = _two_scan_world(scans)
    a, b = _handle(), _handle()
    _batch(b, P, Cov)
    a.map_begin(expected_voxels=16)
    cap0 = a.map_info()["capacity"]
    _insert_two(a, scans)
    info = a.map_info()
    assert info["capacity"] > cap0 and info["capacity"] >= 2 * info["num_voxels"] and info["dropped"] == 0, (cap0, info)
    _check_equal(a.get_voxelmap(), b.get_voxelmap(), 0, "growth:")
    # a NaN and a far point mixed in: skipped and counted as the batch route counts them
    bad = scans["tgt"].copy()
    bad[5, 0] = np.nan
    bad[77] = [3e9, 0, 0]
    _batch(b, bad, scans["Ct"])
    ref = b.get_voxelmap()
    a.map_begin(expected_voxels=16)
    _insert(a, bad, scans["Ct"])
    assert a.debug_skipped_points() == b.debug_skipped_points() == 2
    _check_equal(a.get_voxelmap(), ref, 0, "skipped points:")
    a.close(); b.close()


def test_prune_by_distance_and_by_age(scans):
    P, Cov = _two_scan_world(scans)
    res = 1.0
    a, b = _handle(0, res), _handle(0, res)
    _batch(b, P, Cov)
    ref = R.sorted_map(b.get_voxelmap())
    a.map_begin()
    _insert_two(a, scans)
    center, radius = np.array([1.0, -2.0, 0.5]), 20.0
    keep, slack = R.prune_keep(ref[0], res, center, radius)
    assert slack > 1e-9 and 0 < keep.sum() < len(keep), (slack, keep.sum())
    removed = a.map_prune(center, radius, 0)
    assert removed == int((~keep).sum())
    info = a.map_info()
    assert info["num_voxels"] == int(keep.sum()) and info["dropped"] == 0
    _check_equal(a.get_voxelmap(), tuple(x[keep] for x in ref), 0, "distance prune:")
    # age: three inserts, max_age = 1 keeps exactly the voxels the last insert touched, with their full sums (older points included)
    a.map_begin()
    _insert(a, scans["tgt"], scans["Ct"])
    _insert(a, scans["src"], scans["Cs"], scans["T"])
    shift = np.eye(4); shift[:3, 3] = [0.25, 0.125, 0.0]  # (R = I and a dyadic shift: the fp64 sums are exact, so numpy and the device round the same values)
    _insert(a, scans["tgt"], scans["Ct"], shift)
    P3, C3 = R.transform_cloud(scans["tgt"], scans["Ct"], shift)
    _batch(b, np.concatenate([P, P3]), np.concatenate([Cov, C3]))
    ref3 = R.sorted_map(b.get_voxelmap())
    touched, ok = R.voxel_coords(P3, res)
    touched = {tuple(v) for v in touched[ok]}
    keep3 = np.array([tuple(v) in touched for v in ref3[0]])
    assert 0 < keep3.sum() < len(keep3)
    removed = a.map_prune(None, 0.0, 1)
    assert removed == int((~keep3).sum())
    _check_equal(a.get_voxelmap(), tuple(x[keep3] for x in ref3), 0, "age prune:")
    a.close(); b.close()


def _prepared_source(c, scans):
    c.set_source_cloud(scans["src"]); c.find_source_neighbors(20); c.calculate_source_covariances()


FIELDS = ("T", "H", "final_error", "converged", "nr_iterations", "num_linearize", "num_error_evals")


def test_registration_on_the_incremental_map(scans):
    from fast_gicp_amd import capi
    a, b = _handle(), _handle()
    _batch(b, scans["tgt"], scans["Ct"])
    a.map_begin()
    _insert(a, scans["tgt"], scans["Ct"])
    _prepared_source(a, scans); _prepared_source(b, scans)
    ra, rb = a.align(), b.align()
    print("align on incremental vs batch map: rel_err %.3g" % util.rel_err(ra["T"], rb["T"]), ra["nr_iterations"], ra["num_linearize"], ra["num_launches"])
    assert ra["converged"] and rb["converged"]
    assert ra["nr_iterations"] == rb["nr_iterations"] and ra["num_linearize"] == rb["num_linearize"]
    assert ra["num_launches"] == 1
    assert util.rel_err(ra["T"], rb["T"]) <= POSE_TOL
    te, re_ = util.pose_error(util.relative_pose(), ra["T"])
    assert te < 0.05 and re_ < np.radians(0.5)
    # align_async / _wait on it
    a.align_async()
    rw = a.align_wait()
    for f in FIELDS:
        assert np.array_equal(np.asarray(rw[f]), np.asarray(ra[f])), f
    # the correspondences at the converged pose: the same (source point, voxel coordinate) pairs
    a.update_correspondences(rb["T"]); b.update_correspondences(rb["T"])
    assert a.get_num_correspondences() == b.get_num_correspondences() > 0
    assert np.array_equal(util.sort_rows(util.engine_corr_rows(a)), util.sort_rows(util.engine_corr_rows(b)))
    ea, eb = a.compute_error(rb["T"], False), b.compute_error(rb["T"], False)
    assert abs(ea - eb) <= 1e-9 * abs(eb)
    # align_multi, K = 4 yaw guesses: each result is, bit for bit, the single align under the same grid plan (the map does not change in between)
    G = []
    for deg in (0.0, 15.0, -15.0, 30.0):
        g = np.eye(4); r = np.deg2rad(deg)
        g[:2, :2] = [[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]]
        G.append(g)
    ms = a.align_multi(np.stack(G), max_iterations=12)
    old = a.get_engine_params().cost_max_blocks
    a.set_engine_params(cost_max_blocks=ms[0]["grid_blocks"])
    for m, g in zip(ms, G):
        s = a.align(g, max_iterations=12)
        for f in FIELDS:
            assert np.array_equal(np.asarray(m[f]), np.asarray(s[f])), f
    a.set_engine_params(cost_max_blocks=old)
    assert a.map_info()["incremental"]
    a.close(); b.close()


def _frame_cloud(c, pts):
    c.set_source_cloud(pts); c.find_source_neighbors(20); c.calculate_source_covariances()
    return c.get_covariances("source").copy()


def test_scan_to_map_loop_matches_the_batch_route_and_ground_truth():
    """align frame k against the local map, insert it at the pose found, prune by radius -- against the same loop driven through host
    concatenation + a batch rebuild per frame (both loops keep the map in the frame of scan 0)"""
    from oracle import oracle as O
    n, radius, res = 6, 60.0, 1.0
    frames = [O.approx_voxelgrid(util.lidar_frame(i), 0.25) for i in range(n)]
    a, b = _handle(0, res), _handle(0, res)
    a.map_begin()
    poses_a, poses_b = [np.eye(4)], [np.eye(4)]
    world_P, world_C = [], []
    for k in range(n):
        # --- incremental ---
        Ck = _frame_cloud(a, frames[k])
        if k:
            r = a.align(poses_a[-1])
            assert r["converged"] and r["num_launches"] == 1, k
            poses_a.append(r["T"].copy())
        a.map_insert_source(poses_a[-1])
        a.map_prune(poses_a[-1][:3, 3], radius, 0)
        assert a.map_info()["dropped"] == 0
        # --- batch: the surviving input, rebuilt from scratch ---
        Cb = _frame_cloud(b, frames[k])
        assert np.array_equal(Cb, Ck)
        if k:
            r = b.align(poses_b[-1])
            assert r["converged"], k
            poses_b.append(r["T"].copy())
        Pk, Cpk = R.transform_cloud(frames[k], Cb, poses_b[-1])
        world_P.append(Pk); world_C.append(Cpk)
        P, Cov = np.concatenate(world_P), np.concatenate(world_C)
        # (the batch side prunes POINTS by their voxel: a voxel survives a prune whole or not at all, and a voxel dropped earlier restarts empty)
        coords, ok = R.voxel_coords(P, res)
        keep, _ = R.prune_keep(coords, res, poses_b[-1][:3, 3], radius)
        keep &= ok
        world_P, world_C = [P[keep]], [Cov[keep]]
        _batch(b, P[keep], Cov[keep])
    for k in range(1, n):
        print("frame %d: incremental vs batch rel_err %.3g" % (k, util.rel_err(poses_a[k], poses_b[k])))
    for k in range(1, n):
        assert util.rel_err(poses_a[k], poses_b[k]) <= POSE_TOL, k
    gt = np.linalg.inv(util.lidar_pose(0)) @ util.lidar_pose(n - 1)
    te, re_ = util.pose_error(gt, poses_a[-1])
    print("scan-to-map end pose vs ground truth: %.4f m %.4f deg" % (te, np.degrees(re_)))
    assert te < 0.15 and re_ < np.radians(1.0)  # (the bound test_gpu_streaming.py holds this generator's sequences to)
    a.close(); b.close()


def test_occupancy_bitmap_stays_correct(scans):
    """bitmap_min_points = 1: the map gets a bitmap after the first insert; the second insert creates voxels inside and outside its box. A stale
    bitmap shows up as lost correspondences."""
    P, Cov = _two_scan_world(scans)
    out = []
    for params in (dict(bitmap_min_points=1), dict()):
        a = _handle(**params)
        a.map_begin()
        _insert_two(a, scans)
        _prepared_source(a, scans)
        r = a.align()
        a.update_correspondences(r["T"])
        out.append((r, a.get_num_correspondences(), R.sorted_map(a.get_voxelmap())))
        a.close()
    (r1, n1, m1), (r0, n0, m0) = out
    print("bitmap: correspondences %d vs %d" % (n1, n0))
    assert n1 == n0 > 0
    assert r1["nr_iterations"] == r0["nr_iterations"] and util.rel_err(r1["T"], r0["T"]) <= POSE_TOL
    _check_equal(m1, m0, 0, "bitmap vs none:")
    # and with the bitmap rebuilt by a rehash (growth from a tiny table) + a batch map with a bitmap as the yardstick
    a, b = _handle(bitmap_min_points=1), _handle(bitmap_min_points=1)
    a.map_begin(expected_voxels=16)
    _insert_two(a, scans)
    _batch(b, P, Cov)
    _prepared_source(a, scans); _prepared_source(b, scans)
    ra, rb = a.align(), b.align()
    a.update_correspondences(rb["T"]); b.update_correspondences(rb["T"])
    assert a.get_num_correspondences() == b.get_num_correspondences() > 0
    assert util.rel_err(ra["T"], rb["T"]) <= POSE_TOL
    a.close(); b.close()


def test_refusals_leave_the_handle_usable(scans):
    from fast_gicp_amd import capi
    c = _handle()

    def refused(code, word, fn, *args, **kw):
        with pytest.raises(capi.FvhError) as ei:
            fn(*args, **kw)
        assert "status %d" % code in str(ei.value) and word in str(ei.value), str(ei.value)

    BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4
    refused(BAD_STATE, "map_begin", c.map_insert_source)            # no map yet
    refused(BAD_STATE, "map_begin", c.map_prune, None, 0.0, 1)
    assert not c.map_info()["incremental"]
    # a multi-GPU handle: two handles of this process attached as two ranks on one device (as tests/test_gpu_peer.py does)
    other = _handle()
    exports = [h.peer_export(len(scans["tgt"])) for h in (c, other)]
    for rank, h in enumerate((c, other)):
        h.peer_attach(2, rank, 2, [x for x, _ in exports], [p for _, p in exports])
    refused(UNSUPPORTED, "multi-GPU", c.map_begin)
    refused(UNSUPPORTED, "multi-GPU", c.map_insert_source)
    refused(UNSUPPORTED, "multi-GPU", c.map_insert_cloud, scans["tgt"], scans["Ct"])
    refused(UNSUPPORTED, "multi-GPU", c.map_prune, None, 0.0, 1)
    for h in (c, other):
        h.peer_detach()
    assert not c.map_info()["incremental"]
    c.set_precision(capi.COMPUTE_CUDA_COMPAT)
    refused(UNSUPPORTED, "CUDA_COMPAT", c.map_begin)
    c.set_precision(capi.COMPUTE_FP64)
    c.set_target_map_sharding(True)
    refused(UNSUPPORTED, "sharding", c.map_begin)
    c.set_target_map_sharding(False)
    c.map_begin()
    c.set_source_cloud(scans["tgt"])
    refused(BAD_STATE, "covariances", c.map_insert_source)         # source without covariances
    c.set_source_covariances(scans["Ct"].astype(np.float64))
    bad = np.eye(4); bad[0, 3] = np.nan
    refused(BAD_ARG, "finite", c.map_insert_source, bad)
    assert c._lib.fvh_vgicp_map_insert_source(c.h, None) == BAD_ARG
    c.map_insert_source()
    nv = c.map_info()["num_voxels"]
    # attaching peers to a handle whose incremental map is live is refused (every rank would grow a private map); the map stays
    refused(BAD_STATE, "incremental", c.peer_attach, 2, 0, 2, [x for x, _ in exports], [p for _, p in exports])
    # create_target_voxelmap without a target cloud fails AND leaves the mode as it was
    refused(BAD_STATE, "cloud not set", c.create_target_voxelmap)
    assert c.map_info()["incremental"] and c.map_info()["num_voxels"] == nv
    c.set_target_cloud(scans["tgt"])  # ... and without target covariances
    refused(BAD_STATE, "covariances", c.create_target_voxelmap)
    assert c.map_info()["incremental"] and c.map_info()["num_voxels"] == nv
    refused(BAD_STATE, "incremental", c.swap_source_and_target)
    refused(BAD_STATE, "map_begin", c.set_voxel_accumulation_mode, capi.VOXEL_MULTIPLICATIVE)
    refused(BAD_STATE, "map_begin", c.set_resolution, 0.5)
    refused(UNSUPPORTED, "CUDA_COMPAT", c.set_precision, capi.COMPUTE_CUDA_COMPAT)
    refused(UNSUPPORTED, "shard", c.set_target_map_sharding, True)
    _prepared_source(c, scans)
    c.align_async()
    refused(BAD_STATE, "align_async", c.map_insert_source)
    refused(BAD_STATE, "align_async", c.map_prune, None, 0.0, 1)
    r_inc = c.align_wait()
    assert c.map_info() == dict(incremental=True, num_voxels=nv, capacity=c.debug_table_capacity(), num_inserts=1, num_points=len(scans["tgt"]), dropped=0)
    # a target cloud may be set beside the map (fitness_score needs one); the map stays
    c.set_target_cloud(scans["tgt"])
    assert c.map_info()["incremental"] and c.fitness_score(r_inc["T"]) > 0
    # create_target_voxelmap replaces the incremental map by the batch map of the target cloud: the mode ends, and the plain route gives the parent's answer
    ref = _handle()
    _batch(ref, scans["tgt"], scans["Ct"]); _prepared_source(ref, scans)
    r_ref = ref.align()
    c.set_target_covariances(scans["Ct"].astype(np.float64)); c.create_target_voxelmap()
    assert not c.map_info()["incremental"]
    r = c.align()
    for f in ("nr_iterations", "num_linearize"):
        assert r[f] == r_ref[f] == r_inc[f]
    assert util.rel_err(r["T"], r_ref["T"]) <= POSE_TOL and util.rel_err(r_inc["T"], r_ref["T"]) <= POSE_TOL
    c.swap_source_and_target()  # legal again
    refused(BAD_STATE, "map_begin", c.map_insert_source)
    c.close(); ref.close(); other.close()


def test_pygicp_incremental_target(scans):
    import pygicp
    t, s = scans["tgt"].astype(np.float64), scans["src"].astype(np.float64)
    ref = pygicp.FastVGICPCuda()
    ref.set_input_target(t); ref.set_input_source(s)
    Tb = ref.align().astype(np.float64)
    reg = pygicp.FastVGICPCuda()
    reg.begin_incremental_target()
    reg.set_input_source(t); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s)
    Ta = reg.align().astype(np.float64)
    print("pygicp incremental vs batch target: rel_err %.3g" % util.rel_err(Ta, Tb))
    assert reg.has_converged() and ref.has_converged()
    # get_final_transformation() is float32: the fp64 poses agree to POSE_TOL, their float32 roundings to one spacing more
    assert util.rel_err(Ta, Tb) <= POSE_TOL + 2.0 ** -23
    # insert at the pose just found (the default), prune, align again: still a map, still no host target
    reg.insert_source_into_target()
    assert reg.prune_target(Ta[:3, 3], 1000.0) == 0
    assert reg.prune_target(None, 0.0, 1) > 0
    reg.align(Ta)
    assert reg.has_converged()
    with pytest.raises(Exception):
        reg.swap_source_and_target()
    reg.set_input_target(t)  # ends the mode: the batch route again
    assert util.rel_err(reg.align().astype(np.float64), Tb) <= POSE_TOL + 2.0 ** -23
