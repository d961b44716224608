"""A live map added under a rigid pose, and re-anchored in place (fvh_*_posed_merge_from / fvh_*_transform_map), through the C ABI.

Yardstick: the numpy statement of the contract (tests/posedmerge_ref.py) applied to the DEVICE'S OWN exported snapshots. Keys, counts and ages
must equal the twin's; a sum must lie within 2 gamma 2^-53 abs_bound of it, gamma = 64 + rows landed in the voxel (the twin's docstring derives the
bound: it is not measured), and be bit-equal where that is provable. Records are held, bit for bit, to the existing routes fed with the device's
own sums. Every general-pose input is first checked against near_face (a row whose mean lies within 4 float spacings of a voxel face could
change voxel with the last bit of the mean): a flagged row fails the test as an input defect. Every comparison prints its figures first.

Not reachable in a test: more than 2^28 voxels (FVH_ERR_UNSUPPORTED; the shared capacity check of merge_from / import refuses it), and
handles on different devices when only one is visible (checked when there are two)."""
import numpy as np
import pytest

from tests import mapsnap_ref as S
from tests import posedmerge_ref as P
from tests import util

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4
POSE_TOL = 1e-9  # the header's figure for routes that differ only in the order of fp64 sums
KINDS3 = list(P.KINDS)  # additive, ndt, multiplicative
KINDS2 = ["additive", "ndt"]


def _handle(kind, **params):
    from fast_gicp_amd import capi
    if kind == "ndt":
        c = capi.NDTMapCore(0)
        c.set_distance_mode(capi.NDT_P2D)
    else:
        c = capi.VGICPMapCore(0)
        c.set_voxel_accumulation_mode(P.KINDS[kind])
    if params:
        c.set_engine_params(**params)
    c.set_resolution(P.RES)
    c.set_neighbor_search_method(capi.DIRECT7)
    return c


def _source(c, kind, pts, cov=None):
    c.set_source_cloud(pts)
    if kind != "ndt":
        c.set_source_covariances((P.cloud_covariances(pts) if cov is None else cov).astype(np.float64))


def _insert(c, kind, pts, cov=None, T=None):
    _source(c, kind, pts, cov)
    c.map_insert_source(T)


def _map(kind, pts=None, cov=None, T=None, expected=0, **params):
    c = _handle(kind, **params)
    c.map_begin(expected)
    if pts is not None:
        _insert(c, kind, pts, cov, T)
    return c


def _getters(c, kind):
    vm = c.get_voxelmap("target") if kind == "ndt" else c.get_voxelmap()
    o = S.key_order(vm[0])
    return tuple(np.asarray(x)[o] for x in vm)


def _bits_equal(a, b):
    return all(np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _guard(snap, T, what):
    near = P.transform_rows(snap, T)[5]
    assert not near.any(), "input defect: %s: rows %s lie within the guard of a voxel face" % (what, np.flatnonzero(near))


def _twin(dst_snap, other_snap, T, what):
    _guard(other_snap, T, what)
    return P.posed_merge(dst_snap, other_snap, T)


def _check(got, ref, info, what, exact=None):
    """keys, counts, ages and the header equal; sums within the derived bound; `exact`: a mask of voxels whose ten sums must be bit-equal"""
    assert np.array_equal(got["coords"], ref["coords"]), "%s: voxel sets differ (%d vs %d)" % (what, got["num_voxels"], ref["num_voxels"])
    assert np.array_equal(got["sums"][:, 9], ref["sums"][:, 9]), what
    assert np.array_equal(got["ages"], ref["ages"]), what
    assert all(got[k] == ref[k] for k in ("resolution", "mode", "num_inserts", "num_points", "num_voxels")), what
    d, tol = np.abs(got["sums"] - ref["sums"]), P.sums_tolerance(info)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(tol > 0, d / tol, np.where(d > 0, np.inf, 0.0)))) if d.size else 0.0
    same = int((got["sums"].view(np.uint64) == ref["sums"].view(np.uint64)).all(axis=1).sum())
    print("%s: %d voxels (%d received two or more rows), largest |device - twin| / bound %.3g, %d voxels bit-equal" % (what, got["num_voxels"], int((info["landed"] >= 2).sum()), worst, same))
    assert np.all(d <= tol), (what, worst)
    if exact is not None:
        assert got["sums"][exact].tobytes() == ref["sums"][exact].tobytes(), "%s: %d single-row voxels, not all bit-equal" % (what, int(exact.sum()))


def _check_records(c, kind, what):
    """the records against the existing routes applied to the device's own exported sums, bit for bit: a fresh handle that imports the export
    (every kind), mapsnap_ref.records (additive), the NDT mean (float)(sum p * (1 / n))"""
    e = c.map_export()
    vm = _getters(c, kind)
    twin = _map(kind)
    twin.map_import(e)
    assert _bits_equal(_getters(twin, kind), vm), what
    twin.close()
    assert np.array_equal(vm[0], e["coords"]) and np.array_equal(vm[1].astype(np.float64), e["sums"][:, 9])
    if kind == "additive":
        assert _bits_equal(S.records(e), vm), what
    elif kind == "ndt":
        assert P.row_means(e["sums"], 3).tobytes() == vm[2].tobytes(), what


@pytest.fixture(scope="module")
def data():
    return P.bundled()


@pytest.mark.parametrize("kind", KINDS2)
def test_identity_pose_is_merge_from_to_the_byte(data, kind):
    """The float32 mean of a voxel's points lies in that voxel: the fp64 mean lies between the smallest and the largest point (both float32, both in
    the voxel) up to 2^-52 relative, rounding to float32 is monotone, so the rounded mean lies between them too, and so does its voxel
    coordinate (floor is monotone). With R = I, t = 0 every product is exact and x + 0 = x: no key moves, every sum receives own + incoming."""
    a1, b1 = _map(kind, data["tgt"], data["Ct"]), _map(kind, data["src"], data["Cs"])
    ea, eb = a1.map_export(), b1.map_export()
    # the twin pair holds the SAME sums (two inserts of one scan may differ in the order of their atomics): restored from the exports
    a2, b2 = _map(kind), _map(kind)
    a2.map_import(ea); b2.map_import(eb)
    assert S.same(a2.map_export(), ea) and S.same(b2.map_export(), eb)
    assert a1.map_merge_from_posed(b1, P.IDENTITY) == 0
    a2.map_merge_from(b2)
    got, ref = a1.map_export(), a2.map_export()
    shared = ea["num_voxels"] + eb["num_voxels"] - got["num_voxels"]
    print("identity pose, %s: %d + %d voxels, %d shared, byte-equal to merge_from: %s" % (kind, ea["num_voxels"], eb["num_voxels"], shared, S.same(got, ref)))
    assert 0 < shared < min(ea["num_voxels"], eb["num_voxels"])  # voxels of both kinds: added into and created
    assert S.same(got, ref)
    assert S.same(b1.map_export(), eb) and a1.map_info()["dropped"] == 0
    assert _bits_equal(_getters(a1, kind), _getters(a2, kind))
    for h in (a1, b1, a2, b2):
        h.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_exact_pose_into_an_empty_map(data, kind):
    """90 degrees about z and whole voxels: R has entries 0 / +-1 and n t is exact, so every product is exact and a voxel that received one row
    holds the twin's sums to the bit"""
    other, dst = _map(kind, data["src"], data["Cs"]), _map(kind)
    eo = other.map_export()
    ref, info = _twin(dst.map_export(), eo, P.EXACT, "bundled source, exact pose")
    assert dst.map_merge_from_posed(other, P.EXACT) == 0
    got = dst.map_export()
    _check(got, ref, info, "exact pose, %s" % kind, exact=info["landed"] == 1)
    assert (info["landed"] == 1).sum() > 0.9 * len(info["landed"])
    assert got["sums"][:, 9].sum() == eo["sums"][:, 9].sum() == len(data["src"])
    _check_records(dst, kind, "exact pose, %s" % kind)
    other.close(); dst.close()


@pytest.mark.parametrize("kind", KINDS3)
def test_general_pose_into_a_non_empty_map(data, kind):
    other, dst = _map(kind, data["src"], data["Cs"]), _map(kind, data["tgt"], data["Ct"])
    eo, ed = other.map_export(), dst.map_export()
    ref, info = _twin(ed, eo, P.GENERAL, "bundled source, general pose")
    assert 0 < ref["num_voxels"] - ed["num_voxels"] < eo["num_voxels"]  # voxels of both kinds: added into and created
    assert dst.map_merge_from_posed(other, P.GENERAL) == 0
    _check(dst.map_export(), ref, info, "general pose, %s" % kind)
    _check_records(dst, kind, "general pose, %s" % kind)
    assert S.same(other.map_export(), eo) and dst.map_info()["dropped"] == 0 and dst.map_info()["num_voxels"] == ref["num_voxels"]
    other.close(); dst.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_rows_that_collide_add_up(kind):
    other, dst = _map(kind, P.lattice_cloud()), _map(kind)
    eo = other.map_export()
    assert eo["num_voxels"] == len(P.lattice_cloud())
    ref, info = _twin(dst.map_export(), eo, P.DIAGONAL, "lattice, 45 degrees")
    assert (info["landed"] >= 2).mean() >= 0.10
    assert dst.map_merge_from_posed(other, P.DIAGONAL) == 0
    _check(dst.map_export(), ref, info, "collisions, %s" % kind)
    _check_records(dst, kind, "collisions, %s" % kind)
    other.close(); dst.close()


@pytest.mark.parametrize("n", P.EDGE_SIZES)
@pytest.mark.parametrize("kind", KINDS3)
def test_workgroup_edges(kind, n):
    other, dst = _map(kind), _map(kind, P.voxel_cloud(100, 5))
    _insert(dst, kind, P.voxel_cloud(40, 6))
    if n:
        _insert(other, kind, P.voxel_cloud(n, 100 + n))
    else:  # an `other` with inserts and points but no voxel: three inserts of a point that belongs to none
        for _ in range(3):
            _insert(other, kind, np.array([[np.nan, 0.0, 0.0]], np.float32))
    eo, ed = other.map_export(), dst.map_export()
    assert eo["num_voxels"] == n and ed["num_inserts"] == 2
    ref, info = _twin(ed, eo, P.GENERAL, "%d voxels, general pose" % n)
    assert dst.map_merge_from_posed(other, P.GENERAL) == 0
    got = dst.map_export()
    _check(got, ref, info, "%d voxels, %s" % (n, kind))
    if n == 0:  # only the insert count and num_points move (and with the insert count every age)
        assert got["sums"].tobytes() == ed["sums"].tobytes() and np.array_equal(got["coords"], ed["coords"]) and np.array_equal(got["ages"], ed["ages"] + 1)
        assert got["num_inserts"] == 3 and got["num_points"] == ed["num_points"] + 3
    _check_records(dst, kind, "%d voxels, %s" % (n, kind))
    other.close(); dst.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_out_of_range_rows_are_skipped_and_counted(data, kind):
    other, dst = _map(kind, data["src"], data["Cs"]), _map(kind, data["tgt"], data["Ct"])
    eo, before, skipped0 = other.map_export(), dst.map_export(), dst.debug_skipped_points()
    _, info = P.posed_merge(before, eo, P.FAR)
    assert info["rows_skipped"] == eo["num_voxels"]
    assert dst.map_merge_from_posed(other, P.FAR) == eo["num_voxels"]
    assert dst.debug_skipped_points() - skipped0 == int(eo["sums"][:, 9].sum()) == info["skipped_points"]
    after = dst.map_export()
    assert S.same(dict(after, num_points=before["num_points"]), before) and after["num_points"] == before["num_points"] + eo["num_points"]
    assert dst.map_info()["dropped"] == 0
    # rows_skipped may be NULL
    from fast_gicp_amd import capi
    t = capi._colmajor16(P.FAR)
    assert getattr(dst._lib, dst._prefix + "posed_merge_from")(dst.h, other.h, capi._p(t), None) == 0
    assert dst.debug_skipped_points() - skipped0 == 2 * info["skipped_points"]
    other.close(); dst.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_the_table_grows_before_the_launch(data, kind):
    other, dst = _map(kind, data["src"], data["Cs"]), _map(kind, P.voxel_cloud(5, 77), expected=16)
    cap0 = dst.map_info()["capacity"]
    eo, ed = other.map_export(), dst.map_export()
    ref, info = _twin(ed, eo, P.GENERAL, "bundled source, general pose")
    assert dst.map_merge_from_posed(other, P.GENERAL) == 0
    now = dst.map_info()
    print("growth, %s: capacity %d -> %d for %d voxels" % (kind, cap0, now["capacity"], now["num_voxels"]))
    assert now["capacity"] > cap0 and now["capacity"] >= 2 * now["num_voxels"] and now["dropped"] == 0 and now["num_voxels"] == ref["num_voxels"]
    _check(dst.map_export(), ref, info, "growth, %s" % kind)
    _check_records(dst, kind, "growth, %s" % kind)
    other.close(); dst.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_ages_follow_the_stamp_rule(kind):
    other, dst = _map(kind), _map(kind)
    for seed in P.AGE_SEEDS:
        _insert(other, kind, P.voxel_cloud(300, seed))
    for seed in (41, 42, 43, 44, 45):
        _insert(dst, kind, P.voxel_cloud(200, seed))
    eo, ed = other.map_export(), dst.map_export()
    assert sorted(set(eo["ages"])) == [0, 1, 2] and sorted(set(ed["ages"])) == [0, 1, 2, 3, 4]
    ref, info = _twin(ed, eo, P.GENERAL, "ages")
    assert dst.map_merge_from_posed(other, P.GENERAL) == 0
    got = dst.map_export()
    _check(got, ref, info, "ages, %s" % kind)
    assert got["num_inserts"] == 5
    for max_age in (3, 1):
        gone = int((ref["ages"] >= max_age).sum())
        assert 0 < gone < ref["num_voxels"]
        assert dst.map_prune(None, 0.0, max_age) == gone
        ref = dict(ref, coords=ref["coords"][ref["ages"] < max_age], ages=ref["ages"][ref["ages"] < max_age])
        e = dst.map_export()
        assert np.array_equal(e["coords"], ref["coords"]) and np.array_equal(e["ages"], ref["ages"])
    other.close(); dst.close()


def _host_route(kind, dst_snap, other_snap, T):
    """export -> transform_rows -> voxelmap_import (which accepts repeated keys): what the device call replaces"""
    coords, sums, ages, skipped, _, _ = P.transform_rows(other_snap, T)
    keep = ~skipped
    c = _map(kind)
    c.map_import(dst_snap)
    c.map_import(dict(other_snap, coords=coords[keep], sums=sums[keep], ages=ages[keep], num_voxels=int(keep.sum())))
    return c


@pytest.mark.parametrize("kind", KINDS2)
def test_align_on_the_result_equals_the_host_route(data, kind):
    T = P.relative()
    other, dst = _map(kind, data["src"], data["Cs"]), _map(kind)
    eo, ed = other.map_export(), dst.map_export()
    _guard(eo, T, "bundled source, relative pose")
    assert dst.map_merge_from_posed(other, T) == 0
    host = _host_route(kind, ed, eo, T)
    eh, eg = host.map_export(), dst.map_export()
    assert np.array_equal(eh["coords"], eg["coords"]) and np.array_equal(eh["sums"][:, 9], eg["sums"][:, 9]) and np.array_equal(eh["ages"], eg["ages"])
    out = []
    for c in (dst, host):
        _source(c, kind, data["tgt"], data["Ct"])
        out.append(c.align())
    (rd, rh) = out
    print("align on the posed merge vs the host route, %s: rel_err %.3g, iterations %d / %d" % (kind, util.rel_err(rd["T"], rh["T"]), rd["nr_iterations"], rh["nr_iterations"]))
    assert rd["converged"] and rh["converged"] and rd["nr_iterations"] == rh["nr_iterations"]
    assert util.rel_err(rd["T"], rh["T"]) <= POSE_TOL
    for c in (other, dst, host):
        c.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_the_occupancy_bitmap_follows_the_insert_rule(data, kind):
    """bitmap_min_points = 1: the restored map has a live bitmap. A posed merge under whole voxels (no two rows meet, so every sum is own + one row:
    bit-equal on both handles) creates voxels inside its box, a second one far outside it switches it off. A stale bitmap shows as lost
    correspondences and another pose."""
    first = _map(kind, data["tgt"], data["Ct"])
    base = first.map_export()
    first.close()
    other = _map(kind, data["src"], data["Cs"], P.before_shift())
    far = _map(kind, P.voxel_cloud(5, 77))
    eo, ef = other.map_export(), far.map_export()
    _guard(eo, P.SHIFT, "bundled source before the shift")
    _guard(ef, P.OUTSIDE, "5 voxels, far outside")
    moved = P.transform_rows(eo, P.SHIFT)[0]
    lo, hi = base["coords"].min(axis=0), base["coords"].max(axis=0)
    inside = np.all((moved >= lo) & (moved <= hi), axis=1) & ~np.isin(S.packed_key(moved), S.packed_key(base["coords"]))
    assert inside.sum() > 100 and len(np.unique(S.packed_key(moved))) == len(moved)  # voxels the merge CREATES inside the box; no two rows meet
    out = []
    for params in (dict(bitmap_min_points=1), dict()):
        c = _map(kind, **params)
        c.map_import(base)
        _source(c, kind, data["tgt"], data["Ct"])
        stages = []
        for o, T in ((other, P.SHIFT), (far, P.OUTSIDE)):
            assert c.map_merge_from_posed(o, T) == 0
            r = c.align()
            c.update_correspondences(r["T"])
            stages.append((r, c.get_num_correspondences()))
        out.append((stages, c.map_export()))
        c.close()
    (with_bitmap, e1), (without, e0) = out
    assert S.same(e1, e0) and e1["num_voxels"] > base["num_voxels"] + 100
    for what, (r1, n1), (r0, n0) in zip(("voxels inside the box", "voxels outside it"), with_bitmap, without):
        print("bitmap, %s, %s: correspondences %d vs %d, pose bit-identical %s" % (kind, what, n1, n0, np.array_equal(r1["T"], r0["T"])))
        assert n1 == n0 > 0 and r1["nr_iterations"] == r0["nr_iterations"]
        assert np.array_equal(r1["T"], r0["T"]) and r1["final_error"] == r0["final_error"]
    other.close(); far.close()


@pytest.mark.parametrize("kind", KINDS3)
def test_map_transform_is_a_posed_merge_into_a_fresh_map(data, kind):
    c = _map(kind, data["tgt"], data["Ct"])
    _insert(c, kind, data["src"], data["Cs"], P.relative())
    before, info0 = c.map_export(), c.map_info()
    _source(c, kind, data["tgt"], data["Ct"])
    c.update_correspondences(np.eye(4))
    assert c.get_num_correspondences() > 0
    fresh = _map(kind)
    ref, info = _twin(fresh.map_export(), before, P.GENERAL, "two scans, general pose")
    assert fresh.map_merge_from_posed(c, P.GENERAL) == 0
    assert c.map_transform(P.GENERAL) == 0
    got, ef = c.map_export(), fresh.map_export()
    _check(got, ref, info, "map_transform vs the twin, %s" % kind)
    # against the device's own posed merge into a fresh handle: the same arithmetic per row, so bit-equal wherever one row landed
    assert np.array_equal(got["coords"], ef["coords"]) and np.array_equal(got["ages"], ef["ages"]) and np.array_equal(got["sums"][:, 9], ef["sums"][:, 9])
    one = info["landed"] == 1
    assert got["sums"][one].tobytes() == ef["sums"][one].tobytes() and one.sum() > 0
    info1 = c.map_info()
    assert (info1["num_inserts"], info1["num_points"], info1["dropped"]) == (info0["num_inserts"], info0["num_points"], 0) and info1["num_voxels"] == ref["num_voxels"]
    assert got["num_inserts"] == before["num_inserts"] == 2 and got["num_points"] == before["num_points"]
    _check_records(c, kind, "map_transform, %s" % kind)
    # stored correspondences are gone
    from fast_gicp_amd import capi
    with pytest.raises(capi.FvhError):
        c.compute_error(np.eye(4), False)
    # a following insert and export match the twin: single-point voxels, so every touched sum receives exactly one add -- own + the point's terms
    ins = P.voxel_cloud(200, 41, per_voxel=1)
    _insert(c, kind, ins)
    single = _map(kind, ins)
    es = single.map_export()
    assert np.all(es["sums"][:, 9] == 1.0)
    e2 = c.map_export()
    assert S.same(e2, S.merge(got, dict(es, num_inserts=got["num_inserts"] + 1)))
    assert e2["num_inserts"] == 3 and e2["num_points"] == got["num_points"] + len(ins)
    # a second transform moves the moved map (and an empty map transforms to itself)
    _guard(e2, P.SECOND, "the transformed map, second pose")
    ref2, info2 = P.posed_merge(S.empty_snapshot(P.RES, P.KINDS[kind]), e2, P.SECOND)
    assert c.map_transform(P.SECOND) == 0
    _check(c.map_export(), dict(ref2, num_inserts=3, num_points=e2["num_points"]), info2, "second transform, %s" % kind)
    empty = _map(kind)
    assert empty.map_transform(P.GENERAL) == 0 and empty.map_info()["num_voxels"] == 0
    for h in (c, fresh, single, empty):
        h.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_against_the_map_of_the_moved_points(data, kind):
    """scan inserted at T (map A) vs the identity map of the scan posed-merged under T: the same points, each rounded to float32 once on its way
    into A -- |difference of a summed first moment| <= N 2^-24 max |p'| (half a float32 spacing per point), the counts equal"""
    T = P.GENERAL
    A, B, Cm = _map(kind, data["src"], data["Cs"], T), _map(kind, data["src"], data["Cs"]), _map(kind)
    _guard(B.map_export(), T, "bundled source, general pose")
    assert Cm.map_merge_from_posed(B, T) == 0
    ea, ec = A.map_export(), Cm.map_export()
    moved = data["src"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    bound = len(moved) * 2.0 ** -24 * np.abs(moved).max()
    d = np.abs(ea["sums"][:, :3].sum(axis=0) - ec["sums"][:, :3].sum(axis=0))
    print("moved points vs moved voxels, %s: %d / %d voxels, first moments differ by %s (bound %.3g)" % (kind, ea["num_voxels"], ec["num_voxels"], d, bound))
    assert ea["sums"][:, 9].sum() == ec["sums"][:, 9].sum() == len(moved)
    assert np.all(d <= bound)
    for h in (A, B, Cm):
        h.close()


@pytest.mark.parametrize("kind", KINDS2)
def test_refusals_leave_both_maps_as_they_were(data, kind):
    from fast_gicp_amd import capi
    c, good = _map(kind, data["tgt"], data["Ct"]), _map(kind, data["src"], data["Cs"])
    before, snap = c.map_export(), good.map_export()
    T = P.GENERAL

    def refused(code, word, fn, *args):
        with pytest.raises(capi.FvhError) as ei:
            fn(*args)
        msg = str(ei.value)
        assert "status %d: " % code in msg and word in msg and len(msg.split("status %d: " % code, 1)[1]) > 0, msg
        assert S.same(c.map_export(), before) and S.same(good.map_export(), snap), word

    def raw(h, name, *args):
        rc = getattr(h._lib, h._prefix + name)(h.h, *args)
        msg = getattr(h._lib, h._prefix + "last_error")(h.h)
        assert rc == 0 or (msg and len(msg) > 0)
        return rc

    t = capi._colmajor16(T)
    # invalid arguments
    assert raw(c, "posed_merge_from", None, capi._p(t), None) == BAD_ARG
    assert raw(c, "posed_merge_from", good.h, None, None) == BAD_ARG
    assert raw(c, "transform_map", None, None) == BAD_ARG
    bad = []
    for k, v in (((0, 3), np.nan), ((1, 1), np.inf)):
        x = T.copy(); x[k] = v; bad.append(("rigid", x))
    x = T.copy(); x[:3, :3] *= 1.001; bad.append(("rigid", x))                # scaled
    x = T.copy(); x[:3, 0] *= -1.0; bad.append(("rigid", x))                  # a reflection: det < 0
    x = T.copy(); x[3, 1] = 1e-6; bad.append(("rigid", x))                    # last row
    x = T.copy(); x[0, 1] += 1e-5; bad.append(("rigid", x))                   # sheared
    for word, x in bad:
        refused(BAD_ARG, word, c.map_merge_from_posed, good, x)
        refused(BAD_ARG, word, c.map_transform, x)
    refused(BAD_ARG, "transform_map", c.map_merge_from_posed, c, T)  # other == h: the message points to the in-place call
    half = _handle(kind); half.set_resolution(0.5); half.map_begin(); _insert(half, kind, data["src"], data["Cs"])
    refused(BAD_ARG, "resolution", c.map_merge_from_posed, half, T)
    half.close()
    if kind != "ndt":  # (an NDT handle has one voxel type)
        mult = _map("multiplicative", data["src"], data["Cs"])
        refused(BAD_ARG, "mode", c.map_merge_from_posed, mult, T)
        mult.close()
    if capi.device_count() > 1:
        away = capi.NDTMapCore(1) if kind == "ndt" else capi.VGICPMapCore(1)
        away.set_resolution(P.RES); away.map_begin()
        refused(BAD_ARG, "devices", c.map_merge_from_posed, away, T)
        away.close()
    # no live map on either handle
    bare = _handle(kind)
    refused(BAD_STATE, "map_begin", bare.map_merge_from_posed, good, T)
    refused(BAD_STATE, "map_begin", bare.map_transform, T)
    refused(BAD_STATE, "other handle", c.map_merge_from_posed, bare, T)
    # multi-GPU handles and FVH_COMPUTE_CUDA_COMPAT, as the destination and as the source
    if kind == "ndt":
        bare.set_source_tile(0, 2)
    else:
        bare.set_target_map_sharding(True)
    for fn, args in ((bare.map_merge_from_posed, (good, T)), (bare.map_transform, (T,)), (c.map_merge_from_posed, (bare, T))):
        refused(UNSUPPORTED, "multi-GPU" if kind == "ndt" else "shard", fn, *args)
    if kind == "ndt":
        bare.set_source_tile(0, 1)
    else:
        bare.set_target_map_sharding(False)
    bare.set_precision(capi.COMPUTE_CUDA_COMPAT)
    for fn, args in ((bare.map_merge_from_posed, (good, T)), (bare.map_transform, (T,)), (c.map_merge_from_posed, (bare, T))):
        refused(UNSUPPORTED, "CUDA_COMPAT", fn, *args)
    bare.close()
    # an align_async in flight on either handle
    _source(c, kind, data["tgt"], data["Ct"])
    c.align_async()
    for fn, args in ((c.map_merge_from_posed, (good, T)), (c.map_transform, (T,)), (good.map_merge_from_posed, (c, T))):
        with pytest.raises(capi.FvhError) as ei:
            fn(*args)
        assert "status %d: " % BAD_STATE in str(ei.value) and "align_async" in str(ei.value), str(ei.value)
    assert c.align_wait()["converged"]
    assert S.same(c.map_export(), before) and S.same(good.map_export(), snap)
    # the handle is usable: an align succeeds, and the refused merge now goes through
    assert c.align()["converged"]
    ref, info = _twin(before, snap, T, "bundled source, general pose")
    assert c.map_merge_from_posed(good, T) == 0
    _check(c.map_export(), ref, info, "after the refusals, %s" % kind)
    c.close(); good.close()


def test_pygicp_and_cpp_reach_the_same_calls(data):
    import pygicp
    a, b = _map("additive", data["tgt"], data["Ct"]), _map("additive", data["src"], data["Cs"])
    ea, eb = a.map_export(), b.map_export()
    ra, rb = pygicp.FastVGICPCuda(), pygicp.FastVGICPCuda()
    ra.begin_incremental_target(); ra.import_target_map(ea)
    rb.begin_incremental_target(); rb.import_target_map(eb)
    assert ra.merge_target_from_posed(rb, P.GENERAL) == 0 and a.map_merge_from_posed(b, P.GENERAL) == 0
    ep, ec = ra.export_target_map(), a.map_export()
    assert np.array_equal(np.asarray(ep["coords"]), ec["coords"]) and np.array_equal(np.asarray(ep["ages"]), ec["ages"]) and np.array_equal(np.asarray(ep["sums"])[:, 9], ec["sums"][:, 9])
    _, info = P.posed_merge(ea, eb, P.GENERAL)
    assert np.all(np.abs(np.asarray(ep["sums"]) - ec["sums"]) <= P.sums_tolerance(info))  # (two device runs: the adds may arrive in another order)
    assert ra.transform_target_map(P.SECOND) == 0 and a.map_transform(P.SECOND) == 0
    ep, ec = ra.export_target_map(), a.map_export()
    assert np.array_equal(np.asarray(ep["coords"]), ec["coords"]) and ep["num_points"] == ec["num_points"]
    with pytest.raises(Exception):
        ra.transform_target_map(np.diag([2.0, 2.0, 2.0, 1.0]))
    a.close(); b.close()
