"""The voxel-lookup cost kernel (cost_body, kernels_cost.hpp) where its hand-scheduled branches actually run: tables crowded enough that
continued probes are common and wrap around the end of the table, neighbour lists longer than the kernel's LDS copy, every ragged item
shape cost_shape() can produce, voxel coordinates at the limit of the 21-bit key, and a map scattered enough that the build's LDS stage
spills. The judge of the sums is the oracle fed the ENGINE'S OWN records (get_voxelmap -> set_voxelmap, the fp32-stored source
covariances, round_fp32=True): what is left is the lookup and the cost arithmetic, held to 1e-9 on err and H and util.sums_close on b --
the project's figure for exactly this comparison (test_gpu_parity.py, test_gpu_ndt.py). Correspondence PAIR SETS are compared exactly.
The crowding itself is asserted first, on the CPU, through tests/table_sim.py (checked against the C++ key functions by
test_table_sim_cpu.py), so that an input that stops exercising the branch fails instead of passing quietly."""
import numpy as np
import pytest

from fast_gicp_amd.workloads import se3_exp as _se3_exp
from tests import np_twin, table_sim, util

pytestmark = pytest.mark.gpu

TOL = 1e-9
LIMIT = table_sim.COORD_LIMIT  # voxel_index_ok refuses |index| >= LIMIT
BIG = LIMIT - 1                # the largest legal voxel index


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _capi():
    from fast_gicp_amd import capi
    return capi


def _search(O, name):
    """name -> (engine method, oracle method, radius, offsets)"""
    capi = _capi()
    table = {"DIRECT1": (capi.DIRECT1, O.DIRECT1, 0.0), "DIRECT7": (capi.DIRECT7, O.DIRECT7, 0.0), "DIRECT27": (capi.DIRECT27, O.DIRECT27, 0.0),
             "RADIUS1.5": (capi.DIRECT_RADIUS, O.DIRECT_RADIUS, 1.5), "RADIUS2.5": (capi.DIRECT_RADIUS, O.DIRECT_RADIUS, 2.5), "RADIUS3.0": (capi.DIRECT_RADIUS, O.DIRECT_RADIUS, 3.0)}
    em, om, radius = table[name]
    return em, om, radius, O.neighbor_offsets(om, radius)


N_OFFSETS = {"DIRECT1": 1, "DIRECT7": 7, "DIRECT27": 27, "RADIUS1.5": 19, "RADIUS2.5": 81, "RADIUS3.0": 123}


def _set_search(c, O, name):
    em, om, radius, offsets = _search(O, name)
    assert len(offsets) == N_OFFSETS[name]
    c.set_neighbor_search_method(em, radius if radius else -1.0)


def _vgicp_judge(O, c, tgt, src, name, res):
    """the oracle on the engine's records: fp32-stored covariances of both clouds, and the engine's voxel map in place of its own"""
    _, om, radius, _ = _search(O, name)
    g = O.FastVGICP(search=om, resolution=res, round_fp32=True, radius=radius)
    g.set_target(tgt); g.set_source(src)
    g.set_target_covs(c.get_covariances("target").astype(np.float64)); g.set_source_covs(c.get_covariances("source").astype(np.float64))
    g.prepare()
    coords, num, means, covs = c.get_voxelmap()
    g.set_voxelmap(coords, num, means.astype(np.float64), covs.astype(np.float64))
    return g


def _ndt_judge(O, c, tgt, src, name, mode, res=1.0):
    _, om, radius, _ = _search(O, name)
    g = O.NDT(mode=mode, search=om, radius=radius, resolution=res, round_fp32=True)
    g.set_target(tgt); g.set_source(src); g.prepare()
    for which in ("target",) + (("source",) if mode == O.D2D else ()):
        coords, num, means, covs = c.get_voxelmap(which)
        g.set_voxelmap(which, coords, num, means.astype(np.float64), covs.astype(np.float64))
    return g


def _check_sums(got, ref, tol, what):
    (e, H, b), (eo, Ho, bo) = got, ref
    figures = (abs(e - eo) / max(abs(eo), 1e-300), util.rel_err(H, Ho), float(np.max(np.abs(np.asarray(b) - bo) / np.maximum(np.sqrt(np.abs(np.diag(Ho)) * abs(eo)), 1e-300))))
    assert np.isfinite(e) and np.isfinite(H).all() and np.isfinite(b).all(), what
    assert util.sums_close(e, H, b, eo, Ho, bo, tol), (what, "rel err / H / b (Cauchy-Schwarz scale):", figures)


def _check_pose(c, g, T, T2, what, d2d=False, tol=TOL, after=lambda: None):
    """linearize at T against the judge, the pair sets, and compute_error at the trial pose T2 (correspondences and M stay those of T) with and
    without derivatives. `after` runs behind every engine call. -> the engine's sums at T"""
    got = c.linearize(T); after()
    ref = g.linearize(T)
    assert c.get_num_correspondences() == g.num_correspondences() and g.num_correspondences() > 0, (what, c.get_num_correspondences(), g.num_correspondences())
    _check_sums(got, ref, tol, what)
    util.assert_same_correspondences(c, g, d2d=d2d); after()
    e2o = g.compute_error(T2)
    e2 = c.compute_error(T2, derivatives=False); after()
    e3, H3, b3 = c.compute_error(T2, derivatives=True); after()
    assert abs(e2 - e2o) <= tol * abs(e2o), (what, "trial error", abs(e2 - e2o) / abs(e2o))
    assert abs(e3 - e2o) <= tol * abs(e2o) and np.isfinite(H3).all() and np.isfinite(b3).all(), (what, "trial error with derivatives", abs(e3 - e2o) / abs(e2o))
    return got


def _poses(Tgt, seed, angle_deg=1.0, trans=0.2):
    """identity, ground truth, ground truth composed with a perturbation; each with its trial pose"""
    rng = np.random.default_rng(seed)
    out = []
    for T in (np.eye(4), Tgt, util.random_pose(rng, angle_deg, trans) @ Tgt):
        out.append((T, util.random_pose(rng, 0.2 * angle_deg, 0.25 * trans) @ T))
    return out


def _assert_crowded(coords, capacity, wraps):
    """the table_sim conditions of a crowded table that does not overflow. -> the figures"""
    f = table_sim.fill_table(coords, capacity)
    assert f["load"] >= 0.5 and f["displaced"] >= 500 and f["longest_run"] < table_sim.MAX_PROBE, f
    if wraps:
        assert f["wraps"], f
    return f


def _same_align(r, r0):
    assert r["converged"] == r0["converged"] and r["num_linearize"] == r0["num_linearize"] and r["num_error_evals"] == r0["num_error_evals"], (r, r0)
    assert util.rel_err(r["T"], r0["T"]) < 1e-12 and util.rel_err(r["H"], r0["H"]) < 1e-12, (util.rel_err(r["T"], r0["T"]), util.rel_err(r["H"], r0["H"]))


def _same_sums(a, b, tol, what):
    assert abs(a[0] - b[0]) <= tol * abs(b[0]) and util.rel_err(a[1], b[1]) <= tol and util.rel_err(a[2], b[2]) <= tol, (what, abs(a[0] - b[0]) / abs(b[0]), util.rel_err(a[1], b[1]), util.rel_err(a[2], b[2]))


# ---- a. crowded tables ----------------------------------------------------------------------------------------------------------------
CROWDED_CAPACITY = 8192
CROWDED_HINT = 2048  # 4 x the hint, rounded up to a power of two: 8,192 buckets


@pytest.mark.parametrize("name", ["DIRECT1", "DIRECT7", "DIRECT27"])
def test_vgicp_crowded_table(O, name):
    """6,641 voxels in 8,192 buckets (load 0.81; simulated: 2,559 keys away from their home slot, longest occupied run 115 of the 255 a
    probe may walk, one run across the end of the table). Every lookup that misses its home slot continues the probe; with cost_group_max = 1
    the one-lookup instantiation has requested the HOME slot's record with the key and must not use it for a hit found further on."""
    capi = _capi()
    tgt, src, Tgt = util.synthetic_pair(9000, 9000, seed=7, extent=20.0)
    res = 0.5
    f = _assert_crowded(table_sim.voxel_coords(tgt, res), CROWDED_CAPACITY, wraps=True)
    assert f["across_end"] >= 1  # whatever order the device inserts in, a voxel sits past the end of the table: finding it takes a probe that wraps
    c = capi.VGICPCore(0)
    c.set_resolution(res)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(capi.REG_PLANE)
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances(capi.REG_PLANE)
    c.debug_set_voxel_hint(CROWDED_HINT)
    c.create_target_voxelmap()

    def still_crowded():
        assert c.debug_table_capacity() == CROWDED_CAPACITY, "the table was rebuilt"

    still_crowded()
    coords, num, _, _ = c.get_voxelmap(); still_crowded()
    assert int(num.sum()) == len(tgt) and len(coords) == f["voxels"]
    assert _assert_crowded(coords, CROWDED_CAPACITY, wraps=True) == f  # the handle's voxels are the simulated ones
    poses = _poses(Tgt, 21)
    fixed = {}
    _set_search(c, O, name); still_crowded()
    g = _vgicp_judge(O, c, tgt, src, name, res); still_crowded()
    for pi, (T, T2) in enumerate(poses):
        for gm in (1, 4):
            c.set_engine_params(cost_group_max=gm); still_crowded()
            fixed[pi, gm] = _check_pose(c, g, T, T2, (name, pi, gm), after=still_crowded)
    # a second handle on the same inputs at the default (safe) capacity
    d = capi.VGICPCore(0)
    d.set_resolution(res)
    d.set_target_cloud(tgt); d.set_target_covariances(c.get_covariances("target").astype(np.float64))
    d.set_source_cloud(src); d.set_source_covariances(c.get_covariances("source").astype(np.float64))
    d.create_target_voxelmap()
    assert d.debug_table_capacity() > CROWDED_CAPACITY
    _set_search(d, O, name)
    for gm in (1, 4):
        c.set_engine_params(cost_group_max=gm); d.set_engine_params(cost_group_max=gm)
        _same_align(c.align(), d.align()); still_crowded()
        _same_sums(d.linearize(poses[2][0]), fixed[2, gm], 1e-12, (name, gm))
    c.close(); d.close()


@pytest.mark.parametrize("name", ["DIRECT1", "DIRECT7", "DIRECT27"])
@pytest.mark.parametrize("mode", ["P2D", "D2D"])
def test_ndt_crowded_tables(O, mode, name):
    """NDT on two crowded maps (target: 6,292 voxels, 2,881 of them with more than 6 points, load 0.77, longest run 75, one run across the end of
    the table; source: about 6,340 voxels, load 0.77, longest run 78): P2D looks up the target table per point, D2D per source voxel -- whose
    list comes from the crowded source table."""
    capi = _capi()
    tgt, src, Tgt = util.synthetic_pair(40000, 40000, seed=7, extent=25.0)
    d2d = mode == "D2D"
    ft = _assert_crowded(table_sim.voxel_coords(tgt, 1.0), CROWDED_CAPACITY, wraps=True)
    fs = _assert_crowded(table_sim.voxel_coords(src, 1.0), CROWDED_CAPACITY, wraps=False)

    def make(hint):
        h = capi.NDTCore(0)
        h.set_distance_mode(capi.NDT_D2D if d2d else capi.NDT_P2D); h.set_resolution(1.0)
        h.set_target_cloud(tgt); h.set_source_cloud(src)
        if hint:
            h.debug_set_voxel_hint("target", hint); h.debug_set_voxel_hint("source", hint)
        h.create_voxelmaps()
        return h

    c = make(CROWDED_HINT)
    maps = ("target",) + (("source",) if d2d else ())

    def still_crowded():
        for which in maps:
            assert c.debug_table_capacity(which) == CROWDED_CAPACITY, "the %s table was rebuilt" % which

    still_crowded()
    tc, tn, _, _ = c.get_voxelmap("target"); still_crowded()
    assert int(tn.sum()) == len(tgt) and _assert_crowded(tc, CROWDED_CAPACITY, wraps=True) == ft and int((tn > 6).sum()) > 2000
    if d2d:
        sc, sn, _, _ = c.get_voxelmap("source"); still_crowded()
        assert int(sn.sum()) == len(src) and _assert_crowded(sc, CROWDED_CAPACITY, wraps=False) == fs
    poses = _poses(Tgt, 22)
    fixed = {}
    _set_search(c, O, name); still_crowded()
    g = _ndt_judge(O, c, tgt, src, name, O.D2D if d2d else O.P2D); still_crowded()
    for pi, (T, T2) in enumerate(poses):
        for gm in (1, 4):
            c.set_engine_params(cost_group_max=gm); still_crowded()
            fixed[pi, gm] = _check_pose(c, g, T, T2, (mode, name, pi, gm), d2d=d2d, after=still_crowded)
    d = make(0)
    assert d.debug_table_capacity("target") > CROWDED_CAPACITY
    _set_search(d, O, name)
    for gm in (1, 4):
        c.set_engine_params(cost_group_max=gm); d.set_engine_params(cost_group_max=gm)
        _same_align(c.align(), d.align()); still_crowded()
        _same_sums(d.linearize(poses[2][0]), fixed[2, gm], 1e-12, (mode, name, gm))
    c.close(); d.close()


# ---- b. more than 64 offsets ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_bundled():
    tgt, src = util.bundled_pair()
    return tgt[:6000], src[:3000]


@pytest.mark.parametrize("name", ["RADIUS2.5", "RADIUS3.0"])
def test_vgicp_offset_lists_past_the_lds_copy(O, small_bundled, name):
    """81 and 123 neighbour offsets: the kernel's LDS copy holds 64, longer lists are read from global memory (offsets_packed)."""
    capi = _capi()
    tgt, src = small_bundled
    c = capi.VGICPCore(0)
    _set_search(c, O, name)
    assert N_OFFSETS[name] > 64
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(capi.REG_PLANE); c.create_target_voxelmap()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances(capi.REG_PLANE)
    g = _vgicp_judge(O, c, tgt, src, name, 1.0)
    for pi, (T, T2) in enumerate(_poses(util.relative_pose(), 23)):
        _check_pose(c, g, T, T2, (name, pi))
    r, ro = c.align(), g.align()
    assert r["converged"] and ro["converged"] and r["num_linearize"] == ro["num_linearize"]
    assert util.rel_err(r["T"], ro["T"]) < 1e-4
    c.close()


@pytest.mark.parametrize("name", ["RADIUS2.5", "RADIUS3.0"])
def test_ndt_d2d_offset_lists_past_the_lds_copy(O, small_bundled, name):
    capi = _capi()
    tgt, src = small_bundled
    c = capi.NDTCore(0)
    c.set_distance_mode(capi.NDT_D2D)
    _set_search(c, O, name)
    assert N_OFFSETS[name] > 64
    c.set_target_cloud(tgt); c.set_source_cloud(src); c.create_voxelmaps()
    g = _ndt_judge(O, c, tgt, src, name, O.D2D)
    for pi, (T, T2) in enumerate(_poses(util.relative_pose(), 24)):
        _check_pose(c, g, T, T2, (name, pi), d2d=True)
    r, ro = c.align(), g.align()
    assert r["converged"] and ro["converged"]
    assert util.rel_err(r["T"], ro["T"]) < 1e-4
    c.close()


# ---- c. item shapes -------------------------------------------------------------------------------------------------------------------
SHAPE_N_SRC = (1, 63, 64, 65, 255, 257, 1025)


@pytest.mark.parametrize("name", ["DIRECT1", "DIRECT7", "DIRECT27", "RADIUS1.5", "RADIUS2.5"])
def test_every_item_shape_gives_the_same_sums(O, name):
    """A work item is (source element, group of at most 4 offsets); cost_shape() picks the group size and the grid from cost_group_max,
    cost_target_items and cost_max_blocks. The full grid of those three, at source sizes around one wave and one workgroup: ragged last groups
    (27 = 6 x 4 + 3, 19 = 4 x 4 + 3, 81 = 20 x 4 + 1; groups of 2 and 3), one and three workgroups walking every item, the item -> element
    division by multiplication. Every shape against the judge (1e-9, pair sets exactly) and against the default shape (1e-11: the same terms
    summed in another order, the bound of test_cost_shard_additivity_and_determinism_100k)."""
    capi = _capi()
    defaults = capi.default_engine_params()
    shapes = [(gm, ti, mb) for gm in (1, 2, 3, 4) for ti in (1, defaults.cost_target_items, 1 << 40) for mb in (1, 3, defaults.cost_max_blocks)]
    default_shape = (defaults.cost_group_max, defaults.cost_target_items, defaults.cost_max_blocks)
    assert default_shape in shapes and len(shapes) == 36
    rng = np.random.default_rng(31)
    c = capi.VGICPCore(0)
    _set_search(c, O, name)
    tgt = None
    for n_src in SHAPE_N_SRC:
        t, src, Tgt = util.synthetic_pair(3000, n_src, seed=5, extent=15.0)
        if tgt is None:
            tgt = t
            c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(capi.REG_PLANE); c.create_target_voxelmap()
        assert np.array_equal(t, tgt)  # (the target of the pair does not depend on the source size)
        c.set_source_cloud(src)
        if n_src >= 20:
            c.find_source_neighbors(20); c.calculate_source_covariances(capi.REG_PLANE)
        else:  # too few points for 20 neighbours: injected
            a = rng.normal(size=(n_src, 3, 3)) * 0.2
            c.set_source_covariances(a @ a.transpose(0, 2, 1) + 1e-3 * np.eye(3))
        g = _vgicp_judge(O, c, tgt, src, name, 1.0)
        for pi, (T, T2) in enumerate(_poses(Tgt, 25)[1:]):
            ref = g.linearize(T)
            ref_rows = util.sort_rows(util.oracle_corr_rows(g))
            e2o = g.compute_error(T2)
            assert g.num_correspondences() > 0 or n_src == 1  # (a single point may have no voxel under DIRECT1)
            c.set_engine_params(cost_group_max=default_shape[0], cost_target_items=default_shape[1], cost_max_blocks=default_shape[2])
            base = c.linearize(T)
            for gm, ti, mb in shapes:
                what = (name, n_src, pi, gm, ti, mb)
                c.set_engine_params(cost_group_max=gm, cost_target_items=ti, cost_max_blocks=mb)
                got = c.linearize(T)
                assert c.get_num_correspondences() == g.num_correspondences(), what
                _check_sums(got, ref, TOL, what)
                _same_sums(got, base, 1e-11, what)
                rows = util.engine_corr_rows(c)
                assert len(np.unique(rows, axis=0)) == len(rows) and np.array_equal(util.sort_rows(rows), ref_rows), what
                e2 = c.compute_error(T2, derivatives=False)
                assert abs(e2 - e2o) <= TOL * abs(e2o), what
    c.close()


# ---- d. the coordinate limit ----------------------------------------------------------------------------------------------------------
def limit_scene():
    """Target: clusters of 7 .. 12 points per voxel in voxels whose index reaches BIG = 2^20 - 4097 on +x, -y and -z (and all three at once),
    and points in voxels AT and BEYOND the limit, which belong to no voxel. Coordinates are multiples of 1/16, exact in fp32 below 2^20.
    Source: S1 around the clusters (legal base voxels only: the outward neighbours of a cluster voxel are refused as a BASE); S2 = S1 - t,
    which the translation pose T = (I, t) puts on the clusters -- its -z part is out of range at the identity; S3, legal at the identity and
    more than 600 voxels beyond the limit under T; and non-finite points.
    -> dict(tgt, tgt_cov, n_bad, voxels {coord: count}, src, src_cov, n_s1, T, T2)"""
    rng = np.random.default_rng(41)

    def in_voxel(idx, k):  # k points of voxel idx: idx + 0.5 + u, u in [0, 1) in sixteenths
        return np.asarray(idx, np.float64) + 0.5 + rng.integers(0, 16, (k, 3)) / 16.0

    clusters = [(BIG, 3, -2), (BIG - 1, 3, -2), (BIG, 4, -2), (5, -BIG, 1), (5, -BIG + 1, 1), (6, -BIG, 0), (-4, 2, -BIG), (-4, 2, -BIG + 1), (-3, 3, -BIG), (BIG, -BIG, -BIG), (BIG - 1, -BIG + 1, -BIG + 1)]
    good, voxels = [], {}
    for idx in clusters:
        k = int(rng.integers(7, 13))
        good.append(in_voxel(idx, k)); voxels[idx] = k
    bad_idx = [(LIMIT, 3, -2), (5, -LIMIT, 1), (-4, 2, -LIMIT), (LIMIT + 3, 0, 0), (0, -LIMIT - 700, 0), (0, 0, LIMIT + 1500)]
    bad = [in_voxel(idx, 3) for idx in bad_idx] + [np.array([[2.0 ** 20 + 8.5, 0.5, 0.5], [0.5, 0.5, -(2.0 ** 20) - 8.5]])]  # (the last two: outside the 21 bits)
    tgt = np.concatenate(good + bad)
    n_bad = sum(len(b) for b in bad)
    perm = rng.permutation(len(tgt))
    tgt = tgt[perm]
    assert np.array_equal(tgt.astype(np.float32).astype(np.float64), tgt)

    def spd(n):
        a = rng.normal(size=(n, 3, 3)) * 0.2
        return a @ a.transpose(0, 2, 1) + 1e-2 * np.eye(3)

    # S1: base voxels = a cluster voxel or one of its neighbours, kept legal (an outward neighbour of a voxel at the limit is refused as a BASE)
    s1 = []
    for idx in clusters:
        for _ in range(6):
            s1.append(in_voxel(np.clip(np.asarray(idx) + rng.integers(-1, 2, 3), -BIG, BIG), 1))
    s1 = np.concatenate(s1)
    assert (np.abs(np.floor(s1 - 0.5)) <= BIG).all()
    t = np.array([0.0, 0.0, 700.0])
    s2 = s1 - t
    s3 = np.concatenate([in_voxel((7, -9, BIG - 50), 4), in_voxel((-20, 30, BIG - 80), 4)])
    assert (np.floor(s3 + t - 0.5)[:, 2] > LIMIT + 600).all() and (np.abs(np.floor(s3 - 0.5)) <= BIG).all()
    nonfinite = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf], [np.nan, np.nan, np.nan]])
    src = np.concatenate([s1, s2, s3, nonfinite])
    T = np.eye(4); T[:3, 3] = t
    T2 = T.copy(); T2[:3, 3] += (0.125, -0.0625, 0.25)
    # the same translation behind a rotation of 1e-7 rad (a tenth of a voxel at 1e6 m): q = R p + t is no longer exact in fp64
    Tr = T.copy(); Tr[:3, :3] = _se3_exp(np.array([1.0, 1.0, 1.0, 0, 0, 0]) * (1e-7 / np.sqrt(3.0)))[:3, :3]
    return dict(Tr=Tr, tgt=tgt.astype(np.float32), tgt_cov=spd(len(tgt)), n_bad=n_bad, voxels=voxels, src=src.astype(np.float32), src_cov=spd(len(src)), n_s1=len(s1), T=T, T2=T2)


# Measured on the CPU: np_twin on limit_scene() in float64 against np.longdouble (fp32-rounded voxel records, DIRECT27 and radius 2.5). At the
# identity and under the pure translation q = p + t is exact in fp64 (coordinates in sixteenths) and the two differ by 6e-16; behind the
# 1e-7 rad rotation the rounding of q at 1e6 m shows: the largest relative difference of err / H / b (b on its Cauchy-Schwarz scale) is
# 1.11e-11 for VGICP and 1.23e-11 for NDT P2D. Eight times that is 1e-10, below the 1e-9 of every other comparison here, which therefore stands.
LIMIT_TWIN_DIFF = {"vgicp": 1.11e-11, "ndt": 1.23e-11}


def _limit_tol(kind):
    return max(8.0 * LIMIT_TWIN_DIFF[kind], TOL)


def _limit_poses(s):
    T0 = np.eye(4); T0[:3, 3] = (0.0625, 0.125, -0.1875)
    T2r = s["Tr"].copy(); T2r[:3, 3] += (-0.0625, 0.125, 0.0625)
    return [("identity", np.eye(4), T0), ("translation", s["T"], s["T2"]), ("rotation", s["Tr"], T2r)]


def _limit_checks(c, g, s, kind, name):
    n1 = s["n_s1"]
    for pname, T, T2 in _limit_poses(s):
        _check_pose(c, g, T, T2, (kind, name, pname), tol=_limit_tol(kind))
        elems = util.engine_corr_rows(c)[:, 0]
        # at the identity only S1 has neighbours; under the translation only S2 -- never S3 (beyond the limit there) or a non-finite point
        lo, hi = (0, n1) if pname == "identity" else (n1, 2 * n1)
        assert len(elems) and elems.min() >= lo and elems.max() < hi, (kind, name, pname, elems.min(), elems.max())


def _assert_exact_zeros(c, s):
    """a source of nothing but points that have no voxel under T (S3: more than 600 voxels beyond the limit; non-finite): exact zeros"""
    bad = s["src"][2 * s["n_s1"]:]
    assert len(bad) >= 8 and not np.isfinite(bad).all()
    c.set_source_cloud(bad)
    if hasattr(c, "set_source_covariances"):
        c.set_source_covariances(s["src_cov"][2 * s["n_s1"]:])
    for T in (s["T"], s["Tr"]):
        e, H, b = c.linearize(T)
        assert c.get_num_correspondences() == 0
        assert e == 0.0 and not H.any() and not b.any(), (e, H, b)
        assert c.compute_error(s["T2"], derivatives=False) == 0.0


def test_vgicp_at_the_coordinate_limit(O):
    """Voxels whose index reaches 2^20 - 4097, the largest voxel_index_ok accepts, on +x, -y, -z and all three: their neighbours pass the
    limit (coord_in_range lets them: they stay inside the 21-bit key) and are looked up as misses; points at or beyond the limit, of the
    map or of the source under the pose, and non-finite points belong to no voxel and contribute exact zeros.
    Tolerance: np_twin on this input in float64 against np.longdouble differs by 1.11e-11 (VGICP) / 1.23e-11 (NDT P2D) at worst (the pose with
    a rotation: the fp64 rounding of q at 1e6 m); 8 x that is 1e-10 < 1e-9, so the 1e-9 of the other comparisons holds here too."""
    capi = _capi()
    s = limit_scene()
    c = capi.VGICPCore(0)
    c.set_resolution(1.0)
    c.set_target_cloud(s["tgt"]); c.set_target_covariances(s["tgt_cov"]); c.create_target_voxelmap()
    coords, num, _, _ = c.get_voxelmap()
    assert c.debug_skipped_points() == s["n_bad"]
    assert {tuple(k): int(n) for k, n in zip(coords.tolist(), num)} == s["voxels"]  # (none at or beyond the limit, the others with every point)
    assert max(abs(v) for k in s["voxels"] for v in k) == BIG
    c.set_source_cloud(s["src"]); c.set_source_covariances(s["src_cov"])
    for name in ("DIRECT27", "RADIUS2.5"):
        _set_search(c, O, name)
        _limit_checks(c, _vgicp_judge(O, c, s["tgt"], s["src"], name, 1.0), s, "vgicp", name)
    _assert_exact_zeros(c, s)
    c.close()


def test_ndt_p2d_at_the_coordinate_limit(O):
    """The same scene through NDT P2D (every cluster has more than 6 points). See test_vgicp_at_the_coordinate_limit for the tolerance."""
    capi = _capi()
    s = limit_scene()
    c = capi.NDTCore(0)
    c.set_distance_mode(capi.NDT_P2D); c.set_resolution(1.0)
    c.set_target_cloud(s["tgt"]); c.set_source_cloud(s["src"]); c.create_voxelmaps()
    coords, num, _, _ = c.get_voxelmap("target")
    assert {tuple(k): int(n) for k, n in zip(coords.tolist(), num)} == s["voxels"] and min(s["voxels"].values()) > 6
    assert int(num.sum()) == len(s["tgt"]) - s["n_bad"]
    for name in ("DIRECT27", "RADIUS2.5"):
        _set_search(c, O, name)
        _limit_checks(c, _ndt_judge(O, c, s["tgt"], s["src"], name, O.P2D), s, "ndt", name)
    _assert_exact_zeros(c, s)
    c.close()


# ---- e. scattered map -----------------------------------------------------------------------------------------------------------------
def test_scattered_map_takes_the_spill_path_of_the_build(O):
    """4,096 points over 400 m: every point its own voxel, so a workgroup's 256 points are 256 keys in the 512-slot LDS stage of
    vm_accumulate_kernel, and some (22 in the simulation) find no slot within 8 probes and go straight to the global table as visitors.
    The map must still hold every point exactly once."""
    capi = _capi()
    rng = np.random.default_rng(1)
    pts = rng.uniform(-200, 200, (4096, 3)).astype(np.float32)
    assert capi.default_engine_params().coherent_min_points > len(pts)  # the build walks the points in input order, as the simulation does
    vc = table_sim.voxel_coords(pts, 1.0)
    assert len(np.unique(vc, axis=0)) == len(pts) and table_sim.lds_spills(vc) >= 10
    eye = np.tile(np.eye(3), (len(pts), 1, 1))
    twin = np_twin.voxelmap(pts, eye, 1.0)
    by_coord = {tuple(k): p for k, p in zip(vc.tolist(), pts)}
    assert set(twin) == set(by_coord)

    def check_map(coords, num, means, covs):
        assert len(coords) == len(pts) and set(map(tuple, coords.tolist())) == set(twin)
        assert (num == 1).all() and int(num.sum()) == len(pts)
        want = np.array([by_coord[tuple(k)] for k in coords.tolist()])
        assert (np.abs(means.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()  # one point, divided by 1: the fp32 point itself
        if covs is not None:
            assert np.abs(covs.astype(np.float64) - np.eye(3)).max() <= 1.2e-7

    c = capi.VGICPCore(0)
    c.set_resolution(1.0)
    c.set_target_cloud(pts); c.set_target_covariances(eye); c.create_target_voxelmap()
    check_map(*c.get_voxelmap())
    assert c.debug_skipped_points() == 0
    n = capi.NDTCore(0)
    n.set_resolution(1.0)
    n.set_target_cloud(pts); n.set_source_cloud(pts[:64]); n.create_voxelmaps()
    coords, num, means, _ = n.get_voxelmap("target")
    check_map(coords, num, means, None)
    n.close()
    # a source on that map: a third of the points, moved by a few centimetres
    src = (pts[:1400].astype(np.float64) + rng.normal(size=(1400, 3)) * 0.05).astype(np.float32)
    a = rng.normal(size=(len(src), 3, 3)) * 0.2
    c.set_source_cloud(src); c.set_source_covariances(a @ a.transpose(0, 2, 1) + 1e-3 * np.eye(3))
    _set_search(c, O, "DIRECT7")
    g = _vgicp_judge(O, c, pts, src, "DIRECT7", 1.0)
    # (poses within a fraction of a voxel at 200 m: each of these voxels has empty neighbours all around)
    for pi, (T, T2) in enumerate(_poses(util.random_pose(np.random.default_rng(2), 0.02, 0.05), 26, angle_deg=0.01, trans=0.03)):
        _check_pose(c, g, T, T2, ("scattered", pi))
    c.close()
