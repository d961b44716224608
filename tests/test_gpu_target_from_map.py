"""The live incremental map as the handle's target cloud (fvh_vgicp_target_from_map / fvh_ndt_target_from_map, the two get_target_points
calls) through the C ABI, and the layers above it.

Yardsticks: the map's own getters put into key order by numpy (tests/targetmap_ref.py) -- the call moves floats, it computes none, so every
row is held to BIT equality -- and a second handle that received the same rows over the host route (set_target_cloud +
set_target_covariances): fitness scores, nearest-point correspondences and the point count must be exactly equal; FastGICP's sums and
poses are held to what two runs of the host-route handle show among themselves (bit equality is expected: the engine's sums are
order-fixed).
Synthetic maps come from map_begin + an import of chosen coordinates, sums and counts (cheap and exact); sizes sit either side of every
size at which the route changes: 64 (a wave), 256 (a workgroup of the key / gather kernels), 1,024 (a chunk of the select kernel),
65,536 (its grid cap: larger maps are walked grid-stride; also the engine's own sort routing), and 70,000. Boxes of exactly 32 and of 33
key bits sit either side of the compressed-key / two-sweep choice, and a map that spans the whole coordinate range takes the two sweeps."""
import numpy as np
import pytest

from tests import mapsnap_ref as S
from tests import targetmap_ref as TM
from tests import test_gpu_incremental_map as VG
from tests import test_gpu_ndt_map as ND
from tests import util
from tests.test_gpu_incremental_map import scans  # noqa: F401 (the module's fixture: bundled pair + covariances + a general pose)

pytestmark = pytest.mark.gpu

BAD_STATE = 2
KINDS = ("additive", "multiplicative", "ndt")
MIN_POINTS = (0, 1, 2, 4, 5)
SHIFT = np.eye(4)
SHIFT[:3, 3] = [0.25, 0.125, 0.0]


def _handle(kind, res=1.0):
    """the scan-to-map handle classes: capi.NDTMapCore, capi.VGICPMapCore (a VGICPCore + target_from_map / get_target_points)"""
    from fast_gicp_amd import capi
    if kind == "ndt":
        return ND._handle(res=res)
    c = capi.VGICPMapCore(0)
    c.set_resolution(res)
    c.set_voxel_accumulation_mode(2 if kind == "multiplicative" else 0)
    c.set_neighbor_search_method(capi.DIRECT7)
    return c


def _voxelmap(c, kind):
    return c.get_voxelmap("target") if kind == "ndt" else c.get_voxelmap()


def _sym6(rng, n):
    B = rng.normal(size=(n, 3, 3))
    A = np.einsum("nij,nkj->nik", B, B) + 0.1 * np.eye(3)
    return A, np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], axis=1)


def _snapshot(rng, coords, kind, res=1.0):
    """a map of the voxels `coords` (distinct), counts 1..4, in shuffled order: sums that give every voxel a mean inside it and an SPD covariance"""
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    coords = coords[rng.permutation(len(coords))]
    n = len(coords)
    cnt = rng.integers(1, 5, n).astype(np.float64)
    m = (coords + 0.5 + rng.uniform(0.05, 0.95, (n, 3))) * res
    A, A6 = _sym6(rng, n)
    sums = np.empty((n, 10))
    sums[:, 9] = cnt
    if kind == "additive":
        sums[:, :3], sums[:, 3:9] = m, A6
    elif kind == "multiplicative":
        sums[:, :3], sums[:, 3:9] = np.einsum("nij,nj->ni", A, m), A6
    else:
        mm = np.einsum("ni,nj->nij", m, m) + A
        sums[:, :3] = m
        sums[:, 3:9] = np.stack([mm[:, 0, 0], mm[:, 0, 1], mm[:, 0, 2], mm[:, 1, 1], mm[:, 1, 2], mm[:, 2, 2]], axis=1)
    sums[:, :9] *= cnt[:, None]
    return dict(resolution=res, mode={"additive": 0, "multiplicative": 2, "ndt": 3}[kind], num_inserts=1, num_points=int(cnt.sum()), num_voxels=n, coords=coords, sums=sums, ages=None)


def _random_coords(rng, n):
    if n == 1:
        return np.array([[-3, 2, -1]], np.int32)
    R = max(4, 2 * int(round(n ** (1.0 / 3.0))))
    c = np.unique(rng.integers(-R, R, (2 * n + 64, 3)), axis=0)
    assert len(c) >= n
    c = c[rng.permutation(len(c))[:n]]
    assert n < 8 or all((c[:, a] < 0).any() and (c[:, a] > 0).any() for a in range(3))
    return c.astype(np.int32)


def _imported(kind, snap):
    c = _handle(kind)
    c.map_begin(max(snap["num_voxels"], 1))
    c.map_import(snap)
    return c


def _refused(fn, *args):
    from fast_gicp_amd import capi
    with pytest.raises(capi.FvhError) as ei:
        fn(*args)
    assert "status %d" % BAD_STATE in str(ei.value), str(ei.value)


def _check_rows(c, kind, what, min_points=MIN_POINTS):
    """target_from_map against the getters, for every min_points: count, points and (VGICP) covariances to the bit"""
    vm = _voxelmap(c, kind)
    sizes = []
    for mp in min_points:
        rows, pts, cov = TM.from_voxelmap(vm, mp, with_cov=kind != "ndt")
        n = c.target_from_map(mp)
        sizes.append(n)
        assert n == len(rows), (what, mp, n, len(rows))
        if n == 0:
            _refused(c.get_target_points)  # no target cloud
            continue
        got = c.get_target_points()
        assert TM.same_bits(got, pts), (what, mp, "points", int((got != pts).any(axis=1).sum()))
        if kind != "ndt":
            assert c.num_points("target") == n
            gc = c.get_covariances("target")
            assert TM.same_bits(gc, cov), (what, mp, "covariances", int((gc != cov).any(axis=(1, 2)).sum()))
        if mp <= 1:
            assert np.array_equal(vm[0][rows], c.map_export()["coords"])  # index i is row i of an export
    print(what, kind, "voxels", len(vm[0]), "rows per min_points", dict(zip(min_points, sizes)))
    return vm


SIZE_GROUPS = [(1, 63, 64, 65, 255, 256, 257), (1023, 1024, 1025, 5000), (65536,), (65537,), (70000,)]


@pytest.mark.parametrize("sizes", SIZE_GROUPS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_rows_equal_the_getters_to_the_bit_at_ragged_sizes(kind, sizes):
    rng = np.random.default_rng(sizes[0] * 7 + len(kind))
    for n in sizes:
        c = _imported(kind, _snapshot(rng, _random_coords(rng, n), kind))
        assert c.map_info()["num_voxels"] == n
        vm = _check_rows(c, kind, "size %d:" % n)
        assert c.target_from_map(5) == 0 and vm[1].max() <= 4  # counts are 1..4: nothing qualifies, no target cloud
        if kind != "ndt":
            assert c.num_points("target") == 0
            c.set_source_cloud(np.zeros((4, 3), np.float32))
            _refused(c.fitness_score, np.eye(4))
        c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_wide_span_and_the_32_bit_box(kind):
    rng = np.random.default_rng(17)
    far = (1 << 20) - 5000
    clusters = [np.unique(rng.integers(-20, 21, (300, 3)), axis=0) + o for o in (-far, 0, far)]
    spans = {"whole range (63 key bits)": np.concatenate(clusters)}
    # boxes of exactly 32 and of 33 key bits: the corners pin the extent, both signs on every axis
    for zbits in (10, 11):
        ext = np.array([(1 << 11) - 1, (1 << 11) - 1, (1 << zbits) - 1])
        inner = np.unique(rng.integers(1, ext, (500, 3)), axis=0)
        spans["%d key bits" % (22 + zbits)] = np.concatenate([np.zeros((1, 3), np.int64), ext[None], inner]) - np.array([1000, 700, 300])
    for what, coords in spans.items():
        c = _imported(kind, _snapshot(rng, coords, kind))
        vm = _check_rows(c, kind, what + ":", (1, 3))
        rows = TM.from_voxelmap(vm, 1)[0]
        keys = S.packed_key(vm[0][rows])
        assert all(int(keys[i]) < int(keys[i + 1]) for i in range(len(keys) - 1))
        c.close()


def _real_map(kind, scans, res=1.0):
    c = _handle(kind, res=res)
    c.map_begin()
    if kind == "ndt":
        ND._insert(c, scans["tgt"], SHIFT)
        ND._insert(c, scans["src"], scans["T"])
    else:
        VG._insert(c, scans["tgt"], scans["Ct"], SHIFT)
        VG._insert(c, scans["src"], scans["Cs"], scans["T"])
    return c


@pytest.mark.parametrize("kind", KINDS)
def test_real_map_after_inserts_and_a_prune(scans, kind):
    c = _real_map(kind, scans)
    before = c.map_info()["num_voxels"]
    removed = c.map_prune(scans["T"][:3, 3], 25.0)
    assert 0 < removed < before
    vm = _check_rows(c, kind, "two scans, pruned (%d of %d voxels removed):" % (removed, before), (0, 1, 2, 4, 50))
    assert len(vm[0]) == before - removed and vm[1].max() > 4
    c.close()


def _spread(x, y):
    return max(float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) for a, b in zip(x, y))


def test_equivalence_with_the_host_route(scans):
    A, B = _real_map("additive", scans), VG._handle()
    vm = A.get_voxelmap()
    rows, pts, cov = TM.from_voxelmap(vm, 1)
    assert A.target_from_map(1) == len(rows)
    B.set_target_cloud(pts); B.set_target_covariances(cov.astype(np.float64))
    for c in (A, B):
        c.set_source_cloud(scans["src"]); c.set_source_covariances(scans["Cs"].astype(np.float64))
    assert A.num_points("target") == B.num_points("target") == len(rows)
    T0, T1 = scans["T"], scans["T"] @ SHIFT
    for T in (T0, T1):
        for max_range in (1.7976931348623157e308, 0.05):
            fa, fb = A.fitness_score(T, max_range), B.fitness_score(T, max_range)
            print("fitness at max_range %g: map target %.17g, host route %.17g" % (max_range, fa, fb))
            assert fa == fb and np.isfinite(fa)
    for d in (3.4028234663852886e38, 1.5):
        for c in (A, B):
            c.gicp_set_max_correspondence_distance(d); c.gicp_update_correspondences(T0)
        ca, cb = A.gicp_get_correspondences(), B.gicp_get_correspondences()
        assert np.array_equal(ca, cb) and (ca >= 0).sum() > len(ca) // 2 and ca.max() < len(rows)
    # FastGICP's sums and the LM loop: A against B is held to what B shows against itself
    eb1, eb2, ea = B.gicp_compute_error(T0), B.gicp_compute_error(T0), A.gicp_compute_error(T0)
    bb, ab = _spread(eb1, eb2), _spread(ea, eb1)
    print("gicp_compute_error: host route vs itself %.3g, map target vs host route %.3g" % (bb, ab))
    assert ab <= bb
    rb1, rb2, ra = B.gicp_align(T1), B.gicp_align(T1), A.gicp_align(T1)
    bb, ab = _spread([rb1["T"]], [rb2["T"]]), _spread([ra["T"]], [rb1["T"]])
    print("gicp_align: host route vs itself %.3g (%d / %d iterations), map target vs host route %.3g (%d iterations)" % (bb, rb1["nr_iterations"], rb2["nr_iterations"], ab, ra["nr_iterations"]))
    assert ra["converged"] and rb1["converged"] and ab <= bb
    assert ra["nr_iterations"] == rb1["nr_iterations"] or rb1["nr_iterations"] != rb2["nr_iterations"]
    # what else works on any target cloud
    A.find_target_neighbors(10); B.find_target_neighbors(10)
    assert np.array_equal(A.get_neighbors("target"), B.get_neighbors("target"))
    oa, ob = A.debug_spatial_order("target"), B.debug_spatial_order("target")
    assert np.array_equal(oa[0], ob[0]) and TM.same_bits(oa[1], ob[1]) and np.array_equal(np.sort(oa[0]), np.arange(len(rows)))
    A.close(); B.close()


FIELDS = ("T", "H", "final_error", "converged", "nr_iterations", "num_linearize", "num_error_evals")


def _same_result(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in FIELDS)


@pytest.mark.parametrize("kind", ["additive", "ndt-p2d", "ndt-d2d"])
def test_the_map_is_untouched_and_stays_the_align_target(scans, kind):
    from fast_gicp_amd import capi
    if kind == "additive":
        c = _real_map("additive", scans)
        c.set_source_cloud(scans["src"]); c.set_source_covariances(scans["Cs"].astype(np.float64))
        kind_ = "additive"
    else:
        c = _real_map("ndt", scans)
        c.set_distance_mode(capi.NDT_P2D if kind == "ndt-p2d" else capi.NDT_D2D)
        c.set_source_cloud(scans["src"])
        kind_ = "ndt"
    # (a handle's FIRST D2D align sizes its grid by the point count, later ones by the source-voxel count that align reported: another
    # partition of the same sums, equal to the last bit or so. Both aligns compared here run after that hint exists.)
    c.align(scans["T"])
    info, snap, r0 = c.map_info(), c.map_export(), c.align(scans["T"])
    vm0 = _voxelmap(c, kind_)
    c.update_correspondences(scans["T"])
    n_corr = c.get_num_correspondences()
    n = c.target_from_map(1)
    assert n == info["num_voxels"]
    assert c.get_num_correspondences() == n_corr  # stored voxel correspondences are kept
    assert c.map_info() == info and S.same(c.map_export(), snap)
    r1 = c.align(scans["T"])
    print(kind, "align before / after target_from_map: bit-identical", _same_result(r0, r1), "iterations", r0["nr_iterations"], r1["nr_iterations"])
    assert r0["converged"] and _same_result(r0, r1)
    assert c.map_info() == info and S.same(c.map_export(), snap)  # still incremental after the align: the cloud is not "newer" than the map
    assert all(TM.same_bits(x, y) for x, y in zip(_voxelmap(c, kind_), vm0))
    assert np.isfinite(c.fitness_score(r1["T"]))  # and the cloud made of the map serves the score
    c.close()


@pytest.mark.parametrize("kind", ["additive", "ndt"])
def test_snapshot_semantics_and_refusals(scans, kind):
    c = _handle(kind)
    _refused(c.target_from_map)  # no map_begin
    _refused(c.get_target_points)  # no target cloud
    c.map_begin()
    assert c.target_from_map() == 0  # an empty map: no voxel qualifies
    _refused(c.get_target_points)
    insert = (lambda P, Cv, T=None: ND._insert(c, P, T)) if kind == "ndt" else (lambda P, Cv, T=None: VG._insert(c, P, Cv, T))
    insert(scans["tgt"], scans["Ct"])
    n0 = c.target_from_map()
    p0 = c.get_target_points()
    assert n0 == c.map_info()["num_voxels"] == len(p0) > 0
    insert(scans["src"], scans["Cs"], scans["T"])
    assert c.map_info()["num_voxels"] > n0
    assert TM.same_bits(c.get_target_points(), p0)  # a snapshot: the insert left the cloud alone
    c.map_prune(None, 0.0, 1)
    assert TM.same_bits(c.get_target_points(), p0)
    # an align_async in flight: refused, the cloud stays, the handle stays usable
    if kind != "ndt":
        c.set_source_covariances(scans["Cs"].astype(np.float64))
    c.align_async(scans["T"])
    _refused(c.target_from_map)
    r = c.align_wait()
    assert r["converged"] and TM.same_bits(c.get_target_points(), p0)
    _check_rows(c, kind, "refreshed after insert + prune:", (1, 2))
    assert c.target_from_map() == c.map_info()["num_voxels"]
    c.close()


def test_between_prepare_and_adopt(scans):
    """a preparation on the second stream owns the Engine-wide sort scratch until it is adopted: the call must neither disturb it nor be disturbed"""
    import torch
    from fast_gicp_amd import capi
    d_src = torch.from_numpy(np.ascontiguousarray(scans["src"])).cuda()
    n = len(scans["src"])
    torch.cuda.synchronize()
    # a map large enough that its sort is still running when the preparation's does: the bundled scans + a synthetic 70,000-voxel field
    rng = np.random.default_rng(5)
    field = _snapshot(rng, _random_coords(rng, 70000) + np.array([400, 0, 0]), "additive")

    def handle():
        c = _real_map("additive", scans)
        c.map_import(field)
        return c

    quiet, busy = handle(), handle()
    rows, pts, cov = TM.from_voxelmap(quiet.get_voxelmap(), 1)
    assert quiet.target_from_map() == len(rows)
    p_quiet, c_quiet = quiet.get_target_points(), quiet.get_covariances("target")
    assert TM.same_bits(p_quiet, pts) and TM.same_bits(c_quiet, cov)
    quiet.prepare_source_device(d_src.data_ptr(), n, 3, 20, capi.REG_PLANE, False, 2)
    quiet.adopt_prepared_source()
    busy.synchronize()
    busy.prepare_source_device(d_src.data_ptr(), n, 3, 20, capi.REG_PLANE, False, 2)
    assert busy.target_from_map() == len(rows)
    busy.adopt_prepared_source()
    assert TM.same_bits(busy.get_target_points(), p_quiet) and TM.same_bits(busy.get_covariances("target"), c_quiet)
    # the adopted source is what a preparation with nothing beside it gives
    assert TM.same_bits(busy.get_covariances("source"), quiet.get_covariances("source"))
    assert np.array_equal(busy.get_neighbors("source"), quiet.get_neighbors("source"))
    ob, oq = busy.debug_spatial_order("source"), quiet.debug_spatial_order("source")
    assert np.array_equal(ob[0], oq[0]) and TM.same_bits(ob[1], oq[1])
    rb, rq = busy.align(scans["T"]), quiet.align(scans["T"])
    assert rq["converged"] and _same_result(rb, rq)
    quiet.close(); busy.close()


def test_through_the_classes(scans):
    import pygicp
    from fast_gicp_amd import capi
    t, s = scans["tgt"].astype(np.float64), scans["src"].astype(np.float64)
    reg = pygicp.FastVGICPCuda()
    reg.set_neighbor_search_method("DIRECT7")
    reg.begin_incremental_target()
    reg.set_input_source(t); reg.insert_source_into_target(np.eye(4))
    reg.set_input_source(s)
    T = reg.align(util.relative_pose())
    assert reg.has_converged()
    with pytest.raises(RuntimeError, match=r"fitness_score failed \(status %d\)" % BAD_STATE):  # no target cloud yet: as it is today
        reg.get_fitness_score()
    snap = reg.export_target_map()
    n = reg.target_cloud_from_map()
    assert n == snap["num_voxels"] > 0
    score = reg.get_fitness_score()
    # handle B: the same rows over the host route (the records of the exported sums are the map's: an import recomputes them to the bit)
    A = _imported("additive", dict(snap, ages=None))
    rows, pts, cov = TM.from_voxelmap(A.get_voxelmap(), 1)
    B = VG._handle()
    B.set_target_cloud(pts); B.set_source_cloud(scans["src"])
    ref = B.fitness_score(np.asarray(reg.get_final_transformation(), np.float64))
    print("pygicp fitness on the map %.17g, capi on the host-route handle %.17g (%d points)" % (score, ref, n))
    assert score == ref and len(rows) == n
    assert reg.target_cloud_from_map(2) < n
    reg.target_cloud_from_map()
    # relocalisation: four yaw guesses about the true pose, ranked on the map
    guesses = []
    for k in range(4):
        a = np.radians(90.0 * k)
        Rz = np.eye(4)
        Rz[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        guesses.append(util.relative_pose() @ Rz)
    Tb, best = reg.align_best(np.stack(guesses))
    print("align_best on the map: index %d, rel_err to align() %.3g" % (best, util.rel_err(Tb, T)))
    assert best == 0 and util.rel_err(Tb, T) <= 1e-6
    te, re_ = util.pose_error(util.relative_pose(), np.asarray(Tb, np.float64))
    assert te < 0.1 and re_ < np.radians(0.5)
    # the NDT class: the same loop
    nd = pygicp.NDTCudaMap()
    nd.begin_incremental_target()
    nd.set_input_source(t); nd.insert_source_into_target(np.eye(4))
    nd.set_input_source(s)
    nd.align(util.relative_pose())
    with pytest.raises(RuntimeError, match=r"fitness_score failed \(status %d\)" % BAD_STATE):
        nd.get_fitness_score()
    assert nd.target_cloud_from_map() == nd.export_target_map()["num_voxels"]
    assert np.isfinite(nd.get_fitness_score()) and 0 <= nd.align_best(np.stack(guesses))[1] < 4
    nd.align(util.relative_pose())  # still on the map: no target cloud was ever set through the class
    assert nd.has_converged()
    A.close(); B.close()
