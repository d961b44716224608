"""Incremental NDT target map (fvh_ndt_map_begin / _insert_source / _insert_cloud / _prune / _get_info, fvh_ndt_voxelmap_export / _import /
_merge_from) through the C ABI (capi.NDTMapCore: an NDTCore with the map calls), and pygicp.NDTCudaMap on top.

Yardstick: the batch route on the same device -- set_target_cloud(P') + create_target_voxelmap, itself pinned to the oracle by the parity
tests -- with P' formed in numpy as the contract words it (tests/ndtmap_ref.py: R p + t in fp64, rounded to float32 once). General poses are
moved off the voxel faces (safe_pose, margin 1e-6 voxels). Voxel sets and point counts must be EQUAL; means and covariances may differ by
the order of the fp64 sums only:

    mean: |a - b| <= spacing_float32(entry) + 1e-12 * scale      scale: largest |mean| component of the voxel
    cov:  |a - b| <= spacing_float32(entry) + 8 * delta_v         delta_v = 8 n_v 2^-53 max |p'|^2 over the voxel's points

One float32 spacing because two fp64 values on either side of a rounding boundary round apart. The means are the same sums as those of
additive VGICP voxels: the bound tests/test_gpu_incremental_map.py derives (n 2^-52 with n <= 4,096 points per voxel -> 1e-12). delta_v
bounds a RAW covariance entry (sum pp^T - mean sum p^T) / n under a change of the summation order (ndtmap_ref.voxel_delta); the factor 8 in
front of it covers MIN_EIG's eigenvalue floor: a spectral clamp is Lipschitz with constant ~1 in the Frobenius norm, and sqrt(6) entries give
a Frobenius bound. Both are ANALYTIC bounds, not measured spreads: the order of the atomics differs from run to run, so one measurement is
no ceiling. Every test prints what it measured before it asserts, and the batch-vs-batch spread of two builds of the same cloud, which
must fit the same bound.
Poses: the project holds rebuild-vs-rebuild to 1e-9 (relative); the same bound here.

Measured on an MI355X (one run; every test prints its figures before it asserts): two BATCH builds of the same cloud are bit-identical in
every case here (mean and covariance spread 0 float32 spacings, excess 0), and so is the incremental map against the batch map: one scan
through insert_source / insert_cloud from the host and from a device pointer at resolution 1.0 (1,087 voxels) and 0.5 (2,587), two scans
(1,425 / 3,579), merge_from, growth from 16 expected voxels, the skipped-point cloud, 4,096 scattered voxels, 4,096 points in one voxel,
257 points, the single-point voxels (record: the point itself, covariance diag 1e-3 = MIN_EIG's floor), both prunes and the restored map.
Exported sums against numpy's: at most 0.10 of the 2 (n - 1) 2^-53 sum|x| bound. Poses: P2D rel_err 0 (9 iterations), D2D 6.9e-18
(5 iterations), pygicp 0. The fp64 sums do differ between the routes (hence the bounds); the float32 records did not in this run."""
import numpy as np
import pytest

from tests import ndtmap_ref as N
from tests import util

pytestmark = pytest.mark.gpu

MEAN_EXCESS = 1e-12
COV_FACTOR = 8.0
POSE_TOL = 1e-9
BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4


def _handle(res=1.0, mode=None, **params):
    from fast_gicp_amd import capi
    c = capi.NDTMapCore(0)
    if params:
        c.set_engine_params(**params)
    c.set_resolution(res)
    c.set_distance_mode(capi.NDT_D2D if mode is None else mode)
    c.set_neighbor_search_method(capi.DIRECT7)
    return c


@pytest.fixture(scope="module")
def scans():
    """bundled pair + the pose of data/relative.txt moved off the voxel faces + the second scan at that pose, as the contract forms it"""
    tgt, src = util.bundled_pair()
    T, k = N.safe_pose(src, util.relative_pose(), (1.0, 0.5))
    print("general pose: relative.txt + %d steps; face margin %.3g / %.3g voxels" % (k, N.face_margin(src, T, 1.0), N.face_margin(src, T, 0.5)))
    Ps = N.transform_points(src, T)
    return dict(tgt=tgt, src=src, T=T, Ps=Ps, world=np.concatenate([tgt, Ps]))


def _batch(c, P):
    c.set_target_cloud(P); c.create_target_voxelmap()


def _insert(c, P, T=None):
    c.set_source_cloud(P); c.map_insert_source(T)
    assert c.map_info()["dropped"] == 0


def _spread(got, ref, P, res):
    """two maps that must hold the same voxels with the same counts: the largest differences of means and covariances beyond one float32 spacing
    of the entry, the means' relative to the voxel's scale, the covariances' in units of delta_v (P: the float32 points the maps were built from)"""
    ca, na, ma, va = N.sorted_map(got)
    cb, nb, mb, vb = N.sorted_map(ref)
    assert ca.shape == cb.shape and np.array_equal(ca, cb), "voxel coordinate sets differ (%d vs %d voxels)" % (len(ca), len(cb))
    assert np.array_equal(na, nb), "num_points differ in %d voxels" % int((na != nb).sum())
    if len(ca) == 0:
        return dict(voxels=0, mean_ulps=0.0, mean_excess=0.0, cov_ulps=0.0, cov_excess_in_delta=0.0)
    delta = N.map_delta(cb, P, res)
    out = dict(voxels=len(cb))
    for name, x, y in (("mean", ma, mb), ("cov", va.reshape(-1, 9), vb.reshape(-1, 9))):
        d = np.abs(x.astype(np.float64) - y.astype(np.float64))
        ulp = np.spacing(np.maximum(np.abs(x), np.abs(y)).astype(np.float32)).astype(np.float64)
        over = np.maximum(d - ulp, 0.0)
        out[name + "_ulps"] = float((d / ulp).max())
        if name == "mean":
            out["mean_excess"] = float((over / np.maximum(np.abs(mb).max(axis=1)[:, None], 1e-300)).max())
        else:
            out["cov_excess_in_delta"] = float((over / delta[:, None]).max())
    return out


def _check_equal(got, ref, P, res, what):
    s = _spread(got, ref, P, res)
    print(what, s)
    assert s["mean_excess"] <= MEAN_EXCESS, (what, s)
    assert s["cov_excess_in_delta"] <= COV_FACTOR, (what, s)
    return s


def _reference(P, res, what):
    """the batch map of the float32 cloud P; printed and checked beside it: the spread of two batch builds of that cloud"""
    b, b2 = _handle(res), _handle(res)
    _batch(b, P); _batch(b2, P)
    ref = b.get_voxelmap("target")
    _check_equal(b2.get_voxelmap("target"), ref, P, res, "batch vs batch, %s:" % what)
    b.close(); b2.close()
    return ref


@pytest.mark.parametrize("res", [1.0, 0.5])
def test_one_scan_at_the_identity_equals_the_batch_map(scans, res):
    import torch
    tgt = scans["tgt"]
    ref = _reference(tgt, res, "bundled target res %g" % res)
    a = _handle(res)
    a.map_begin()
    _insert(a, tgt)
    info = a.map_info()
    assert info["incremental"] and info["num_inserts"] == 1 and info["num_points"] == len(tgt) and info["num_voxels"] == len(ref[0])
    _check_equal(a.get_voxelmap("target"), ref, tgt, res, "insert_source vs batch res %g:" % res)
    a.map_begin()  # restarted: the same cloud through insert_cloud, from the host ...
    a.map_insert_cloud(tgt)
    _check_equal(a.get_voxelmap("target"), ref, tgt, res, "insert_cloud (host) vs batch:")
    a.map_begin()  # ... and from a device pointer
    d = torch.from_numpy(tgt).to(torch.device("cuda", 0)).contiguous()
    torch.cuda.synchronize()
    a.map_insert_cloud(None, device_ptr=d.data_ptr(), n=len(tgt), stride=3)
    _check_equal(a.get_voxelmap("target"), ref, tgt, res, "insert_cloud (device) vs batch:")
    assert a.map_info()["num_inserts"] == 1
    a.close()


@pytest.mark.parametrize("res", [1.0, 0.5])
def test_two_scans_at_a_general_pose_equal_the_batch_map_of_the_concatenation(scans, res):
    assert N.face_margin(scans["src"], scans["T"], res) > 1e-6
    ref = _reference(scans["world"], res, "two scans res %g" % res)
    a = _handle(res)
    a.map_begin()
    _insert(a, scans["tgt"]); _insert(a, scans["src"], scans["T"])
    _check_equal(a.get_voxelmap("target"), ref, scans["world"], res, "two scans vs batch res %g:" % res)
    info = a.map_info()
    assert info["num_points"] == len(scans["world"]) and info["num_inserts"] == 2 and info["num_voxels"] == len(ref[0]) and info["dropped"] == 0
    a.close()


@pytest.fixture(scope="module")
def two_scan_snapshot(scans):
    """the snapshot of the two-scan map at resolution 1.0 (shared: export, round trip, merge, age prune of a restored map)"""
    a = _handle()
    a.map_begin()
    _insert(a, scans["tgt"]); _insert(a, scans["src"], scans["T"])
    snap = a.map_export()
    a.close()
    return snap


def test_exported_sums_equal_numpys_fp64_sums(scans, two_scan_snapshot):
    from fast_gicp_amd import capi
    snap = two_scan_snapshot
    ref = N.voxel_sums(scans["world"], 1.0)
    assert snap["mode"] == capi.VOXEL_NDT_SUMS == 3 and snap["resolution"] == 1.0 and snap["num_inserts"] == 2 and snap["num_points"] == len(scans["world"])
    assert np.array_equal(snap["coords"], ref["coords"])  # (both in ascending packed-key order)
    assert np.array_equal(snap["sums"][:, 9], ref["sums"][:, 9])
    d = np.abs(snap["sums"] - ref["sums"])
    bound = N.sum_order_bound(ref["sums"][:, 9], ref["abs_sums"])
    print("exported sums vs numpy: largest |difference| / (2 (n - 1) 2^-53 sum|x|) = %.3g over %d voxels" % (float((d / np.maximum(bound, 1e-300)).max()), len(d)))
    assert np.all(d <= bound)
    # the second scan touched its voxels last: age 0 there, 1 on the voxels only the first scan touched
    c2, ok = N.voxel_coords(scans["Ps"], 1.0)
    touched = {tuple(v) for v in c2[ok]}
    assert np.array_equal(snap["ages"], np.array([0 if tuple(v) in touched else 1 for v in snap["coords"]], np.uint32))


def test_export_import_export_is_byte_equal(two_scan_snapshot, tmp_path):
    from fast_gicp_amd import capi
    snap = two_scan_snapshot
    b = _handle()
    b.map_begin(snap["num_voxels"])
    b.map_import(snap)
    back = b.map_export()
    for k in ("resolution", "mode", "num_inserts", "num_points", "num_voxels"):
        assert back[k] == snap[k], k
    for k in ("coords", "sums", "ages"):
        assert back[k].tobytes() == snap[k].tobytes(), k
    # ... and through a file into a handle with no live map
    p1, p2 = str(tmp_path / "a.fvhmap"), str(tmp_path / "b.fvhmap")
    b.map_save(p1)
    c = _handle(0.5)  # (takes the file's resolution)
    c.map_load(p1)
    c.map_save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    assert capi.read_map_file(p1)["mode"] == 3
    b.close(); c.close()


def test_merge_from_adds_two_maps_to_the_bit(scans):
    a, b = _handle(), _handle()
    a.map_begin(); b.map_begin()
    _insert(a, scans["tgt"])
    _insert(b, scans["src"], scans["T"])
    sa, sb = a.map_export(), b.map_export()
    a.map_merge_from(b)
    merged = a.map_export()
    # numpy: the union of the rows, every sum of a shared voxel receiving ONE add (own + incoming)
    rows = {}
    for s in (sa, sb):
        for c, v in zip(map(tuple, s["coords"]), s["sums"]):
            rows[c] = rows[c] + v if c in rows else v.copy()
    keys = sorted(rows, key=lambda c: (c[2], c[1], c[0]))
    assert np.array_equal(merged["coords"], np.array(keys, np.int32))
    assert np.array_equal(merged["sums"], np.array([rows[k] for k in keys]))
    assert merged["num_points"] == len(scans["world"]) and merged["num_inserts"] == 1
    assert np.array_equal(b.map_export()["sums"], sb["sums"])  # `other` is unchanged
    # ... and the merged map is the batch map of both clouds
    _check_equal(a.get_voxelmap("target"), _reference(scans["world"], 1.0, "merge"), scans["world"], 1.0, "merge_from vs batch:")
    a.close(); b.close()


def test_growth_from_a_tiny_table_drops_nothing(scans):
    ref = _reference(scans["world"], 1.0, "growth")
    a = _handle()
    a.map_begin(expected_voxels=16)
    cap0 = a.map_info()["capacity"]
    _insert(a, scans["tgt"]); _insert(a, scans["src"], scans["T"])
    info = a.map_info()
    assert info["capacity"] > cap0 and info["capacity"] >= 2 * info["num_voxels"] and info["dropped"] == 0, (cap0, info)
    _check_equal(a.get_voxelmap("target"), ref, scans["world"], 1.0, "growth:")
    # a NaN and a far point mixed in: they belong to no voxel on either route, and the insert still counts them as offered
    bad = scans["tgt"].copy()
    bad[5, 0] = np.nan
    bad[77] = [3e9, 0, 0]
    b = _handle()
    _batch(b, bad)
    refb = b.get_voxelmap("target")
    a.map_begin(expected_voxels=16)
    _insert(a, bad)
    got = a.get_voxelmap("target")
    assert a.map_info()["num_points"] == len(bad)
    assert len(bad) - int(got[1].sum()) == len(bad) - int(refb[1].sum()) == 2
    ok = np.isfinite(bad).all(axis=1) & (np.abs(bad) < 1e9).all(axis=1)
    _check_equal(got, refb, bad[ok], 1.0, "skipped points:")
    a.close(); b.close()


def _crowded_clouds():
    rng = np.random.default_rng(7)
    spread = rng.uniform(-100.0, 100.0, (4096, 3)).astype(np.float32)       # 200 m cube at res 0.5: 6.4e7 voxels for 4,096 points
    one = (np.array([10.25, -3.25, 1.25]) + rng.uniform(0.0, 0.24, (4096, 3))).astype(np.float32)  # voxel (20, -7, 2) at res 0.5: [10.25, 10.5) ...
    ragged = rng.uniform(-20.0, 20.0, (257, 3)).astype(np.float32)          # the second workgroup holds one point
    return [("4096 points, each in its own voxel", spread), ("4096 points in one voxel", one), ("257 points", ragged)]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_crowded_lds_stage_same_address_contention_and_a_ragged_tail(case):
    what, P = _crowded_clouds()[case]
    res = 0.5
    coords, ok = N.voxel_coords(P, res)
    nv = len(np.unique(coords, axis=0))
    if case == 0:
        from tests import table_sim
        # every workgroup meets 256 distinct voxels in a 512-slot LDS table probed 8 deep: some points find no slot and go straight to the map
        assert nv == len(P) and table_sim.lds_spills(coords) > 0
    if case == 1:
        assert nv == 1
    ref = _reference(P, res, what)
    a = _handle(res)
    a.map_begin()
    _insert(a, P)
    assert a.map_info()["num_voxels"] == nv
    _check_equal(a.get_voxelmap("target"), ref, P, res, what + ":")
    a.close()


def test_a_voxel_with_a_single_point(scans):
    """raw covariance exactly zero on both routes: the records must be EQUAL, whatever MIN_EIG makes of a zero matrix"""
    P = np.concatenate([scans["tgt"][:2000], np.array([[250.3, -250.7, 40.1]], np.float32)])
    res = 1.0
    ref = N.sorted_map(_reference(P, res, "single-point voxel"))
    a = _handle(res)
    a.map_begin()
    _insert(a, P)
    got = N.sorted_map(a.get_voxelmap("target"))
    _check_equal(got, ref, P, res, "single-point voxel:")
    lone = np.flatnonzero((ref[0] == np.floor(P[-1].astype(np.float64) / res - 0.5).astype(np.int64)).all(axis=1))
    assert len(lone) == 1 and ref[1][lone[0]] == 1
    singles = ref[1] == 1
    print("single-point voxels: %d; record of the lone one: mean %s cov diag %s" % (int(singles.sum()), got[2][lone[0]], np.diagonal(got[3][lone[0]])))
    assert np.array_equal(got[2][singles], ref[2][singles]) and np.array_equal(got[3][singles], ref[3][singles])
    assert np.array_equal(got[2][lone[0]], P[-1])
    a.close()


def test_prune_by_distance_and_by_age(scans, two_scan_snapshot):
    res = 1.0
    P = scans["world"]
    ref = N.sorted_map(_reference(P, res, "prune"))
    a = _handle(res)
    a.map_begin()
    _insert(a, scans["tgt"]); _insert(a, scans["src"], scans["T"])
    center, radius = np.array([1.0, -2.0, 0.5]), 20.0
    keep, slack = N.prune_keep(ref[0], res, center, radius)
    assert slack > 1e-9 and 0 < keep.sum() < len(keep), (slack, keep.sum())
    removed = a.map_prune(center, radius, 0)
    assert removed == int((~keep).sum())
    info = a.map_info()
    assert info["num_voxels"] == int(keep.sum()) and info["dropped"] == 0
    _check_equal(a.get_voxelmap("target"), tuple(x[keep] for x in ref), P, res, "distance prune:")
    # age: max_age = 1 keeps exactly the voxels the last insert touched, with their FULL sums (older points included) -- on the original
    # and on a map restored from its snapshot
    touched, ok = N.voxel_coords(scans["Ps"], res)
    touched = {tuple(v) for v in touched[ok]}
    keep2 = np.array([tuple(v) in touched for v in ref[0]])
    assert 0 < keep2.sum() < len(keep2)
    a.map_begin()
    _insert(a, scans["tgt"]); _insert(a, scans["src"], scans["T"])
    b = _handle(res)
    b.map_begin()
    b.map_import(two_scan_snapshot)
    for h, what in ((a, "age prune:"), (b, "age prune of a restored map:")):
        assert h.map_prune(None, 0.0, 1) == int((~keep2).sum()), what
        _check_equal(h.get_voxelmap("target"), tuple(x[keep2] for x in ref), P, res, what)
    a.close(); b.close()


FIELDS = ("T", "H", "final_error", "converged", "nr_iterations", "num_linearize", "num_error_evals")


@pytest.mark.parametrize("mode", ["P2D", "D2D"])
def test_registration_on_the_incremental_map(scans, mode):
    from fast_gicp_amd import capi
    m = capi.NDT_P2D if mode == "P2D" else capi.NDT_D2D
    a, b = _handle(1.0, m), _handle(1.0, m)
    _batch(b, scans["tgt"])
    a.map_begin()
    _insert(a, scans["tgt"])
    a.set_source_cloud(scans["src"]); b.set_source_cloud(scans["src"])
    ra, rb = a.align(), b.align()  # (no target cloud was ever set on `a`)
    print("%s align on incremental vs batch map: rel_err %.3g" % (mode, util.rel_err(ra["T"], rb["T"])), ra["nr_iterations"], ra["num_linearize"], ra["num_launches"])
    assert ra["converged"] and rb["converged"]
    assert ra["nr_iterations"] == rb["nr_iterations"] and ra["num_linearize"] == rb["num_linearize"]
    assert util.rel_err(ra["T"], rb["T"]) <= POSE_TOL
    te, re_ = util.pose_error(util.relative_pose(), ra["T"])
    assert te < 0.1 and re_ < np.radians(0.5)
    # the pipelined route: prepare_source (the slot's cloud and, D2D, its map) -> adopt -> align_async / _wait
    a.prepare_source(scans["src"])
    a.adopt_prepared_source()
    a.align_async()
    rw = a.align_wait()
    assert rw["nr_iterations"] == ra["nr_iterations"] and util.rel_err(rw["T"], ra["T"]) <= POSE_TOL
    # the host-driven evaluations and the getters read the same map
    a.update_correspondences(rb["T"]); b.update_correspondences(rb["T"])
    assert a.get_num_correspondences() == b.get_num_correspondences() > 0
    ea, eb = a.compute_error(rb["T"], False), b.compute_error(rb["T"], False)
    assert abs(ea - eb) <= 1e-9 * abs(eb)
    ms = a.align_multi(np.stack([np.eye(4), np.eye(4)]))
    assert all(util.rel_err(x["T"], ra["T"]) <= POSE_TOL for x in ms)
    if mode == "D2D":
        # a source map whose hint-sized table overflows is rebuilt at the safe size and the align redone: that rebuild must leave the live
        # incremental target alone (there is no cloud to rebuild it from)
        a.debug_set_voxel_hint("source", 1)
        a.set_source_cloud(scans["src"])
        ro = a.align()
        assert a.debug_table_capacity("source") > 1024
        assert ro["nr_iterations"] == ra["nr_iterations"] and util.rel_err(ro["T"], ra["T"]) <= POSE_TOL
    info = a.map_info()
    assert info["incremental"] and info["num_inserts"] == 1 and info["num_points"] == len(scans["tgt"])
    a.close(); b.close()


def test_refusals_leave_the_handle_usable(scans, two_scan_snapshot):
    from fast_gicp_amd import capi
    c = _handle()

    def refused(code, word, fn, *args, **kw):
        with pytest.raises(capi.FvhError) as ei:
            fn(*args, **kw)
        assert "status %d" % code in str(ei.value) and word in str(ei.value), str(ei.value)
        return str(ei.value)

    empty = dict(resolution=1.0, mode=3, num_inserts=0, num_points=0, coords=np.zeros((0, 3), np.int32), sums=np.zeros((0, 10)))
    # no map yet
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_insert_source)
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_insert_cloud, scans["tgt"])
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_prune, None, 0.0, 1)
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_export)
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_import, empty)
    assert not c.map_info()["incremental"]
    # a tiled handle, FVH_COMPUTE_CUDA_COMPAT: no incremental map, in both orders
    c.set_source_tile(0, 2)
    refused(UNSUPPORTED, "multi-GPU", c.map_begin)
    c.set_source_tile(0, 1)
    c.set_precision(capi.COMPUTE_CUDA_COMPAT)
    refused(UNSUPPORTED, "CUDA_COMPAT", c.map_begin)
    c.set_precision(capi.COMPUTE_FP64)
    c.map_begin()
    refused(BAD_STATE, "cloud is not set", c.map_insert_source)  # no source yet
    c.set_source_cloud(scans["tgt"])
    bad = np.eye(4); bad[0, 3] = np.nan
    refused(BAD_ARG, "finite", c.map_insert_source, bad)
    assert c._lib.fvh_ndt_map_insert_source(c.h, None) == BAD_ARG
    c.map_insert_source()
    nv = c.map_info()["num_voxels"]
    refused(UNSUPPORTED, "CUDA_COMPAT", c.set_precision, capi.COMPUTE_CUDA_COMPAT)
    refused(BAD_STATE, "map_begin", c.set_resolution, 0.5)
    c.set_resolution(1.0)  # (the live map's own value: legal)
    refused(BAD_STATE, "incremental", c.swap_source_and_target)
    refused(BAD_STATE, "incremental", c.set_source_tile, 0, 2)
    refused(BAD_STATE, "incremental", c.comm_init, bytes(128), 2, 0)
    # snapshots of VGICP sums are refused by an NDT map, and NDT sums by a VGICP map: never added silently
    for mode in (0, 1, 2):
        refused(BAD_ARG, "mode", c.map_import, dict(two_scan_snapshot, mode=mode))
    v = capi.VGICPCore(0)
    v.map_begin()
    refused(BAD_ARG, "mode", v.map_import, two_scan_snapshot)
    assert v.map_info()["num_voxels"] == 0
    # fitness_score needs a target cloud: the answer of a VGICP handle in the same state
    v.set_source_cloud(scans["src"])
    c.set_source_cloud(scans["src"])
    msg_v = refused(BAD_STATE, "", v.fitness_score, np.eye(4))
    msg_c = refused(BAD_STATE, "", c.fitness_score, np.eye(4))
    assert msg_v.split("status")[1] == msg_c.split("status")[1], (msg_v, msg_c)
    v.close()
    other = _handle()
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_merge_from, other)  # the other handle has no live map
    refused(BAD_ARG, "itself", c.map_merge_from, c)
    other.close()
    assert c.map_info() == dict(incremental=True, num_voxels=nv, capacity=c.debug_table_capacity("target"), num_inserts=1, num_points=len(scans["tgt"]), dropped=0)
    # inserts, prunes and imports while an align is in flight
    c.align_async()
    refused(BAD_STATE, "align_async", c.map_insert_source)
    refused(BAD_STATE, "align_async", c.map_insert_cloud, scans["tgt"])
    refused(BAD_STATE, "align_async", c.map_prune, None, 0.0, 1)
    refused(BAD_STATE, "align_async", c.map_import, empty)
    r_inc = c.align_wait()
    # after all of it the handle aligns as a handle that was never refused anything
    ref = _handle()
    _batch(ref, scans["tgt"]); ref.set_source_cloud(scans["src"])
    r_ref = ref.align()
    r_again = c.align()
    for r in (r_inc, r_again):
        assert r["converged"] and r["nr_iterations"] == r_ref["nr_iterations"] and util.rel_err(r["T"], r_ref["T"]) <= POSE_TOL
    assert c.map_info()["incremental"] and c.map_info()["num_voxels"] == nv
    # set_target_cloud + create_target_voxelmap ends the mode: the plain route again
    c.set_target_cloud(scans["tgt"])
    assert c.map_info()["incremental"] and c.fitness_score(r_inc["T"]) > 0
    c.create_target_voxelmap()
    assert not c.map_info()["incremental"]
    r = c.align()
    assert r["nr_iterations"] == r_ref["nr_iterations"] and util.rel_err(r["T"], r_ref["T"]) <= POSE_TOL
    c.swap_source_and_target()  # legal again
    refused(BAD_STATE, "fvh_ndt_map_begin", c.map_insert_source)
    c.close(); ref.close()


def test_pygicp_ndt_incremental_target(scans, tmp_path):
    import pygicp
    t, s = scans["tgt"].astype(np.float64), scans["src"].astype(np.float64)
    ref = pygicp.NDTCuda()
    ref.set_input_target(t); ref.set_input_source(s)
    Tb = ref.align().astype(np.float64)
    reg = pygicp.NDTCudaMap()
    reg.begin_incremental_target()
    reg.set_input_source(t); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s)
    Ta = reg.align().astype(np.float64)
    print("pygicp NDTCudaMap incremental vs batch target: rel_err %.3g" % util.rel_err(Ta, Tb))
    assert reg.has_converged() and ref.has_converged()
    # get_final_transformation() is float32: the fp64 poses agree to POSE_TOL, their float32 roundings to one spacing more
    assert util.rel_err(Ta, Tb) <= POSE_TOL + 2.0 ** -23
    path = str(tmp_path / "ndt.fvhmap")
    reg.save_target_map(path)
    snap = reg.export_target_map()
    assert snap["mode"] == 3 and snap["num_inserts"] == 1 and snap["num_points"] == len(t)
    fresh = pygicp.NDTCudaMap()
    fresh.load_target_map(path)
    fresh.set_input_source(s)
    Tf = fresh.align().astype(np.float64)
    assert fresh.has_converged() and util.rel_err(Tf, Ta) <= POSE_TOL + 2.0 ** -23
    with pytest.raises(Exception):
        pygicp.FastVGICPCuda().load_target_map(path)  # NDT sums never enter a VGICP map
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
