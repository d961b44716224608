"""Snapshots of the incremental target map (fvh_vgicp_voxelmap_export / _import / _merge_from) through the C ABI, and the layers above it.

Yardsticks: the map's own getters, the numpy statement of the contract (tests/mapsnap_ref.py) and a handle that received the same scans
as inserts. Inputs, the pose and the bounds are those of tests/test_gpu_incremental_map.py (its docstring derives them): EXCESS -- what a
different ORDER of the fp64 sums may move a float32 record entry beyond one spacing, relative to the voxel's scale -- and POSE_TOL.
Everything that does not reorder sums is held to byte equality: export -> import -> export, device merge vs numpy merge vs host-route merge,
file round trips, additive records recomputed from the exported sums. Every comparison prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import incmap_ref as R
from tests import mapsnap_ref as S
from tests import util
from tests.test_gpu_incremental_map import EXCESS, POSE_TOL, _check_equal, _handle, _insert, _prepared_source, scans  # noqa: F401 (scans: the module's fixture)

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE, UNSUPPORTED = 1, 2, 4
SHIFT = np.eye(4)
SHIFT[:3, 3] = [0.25, 0.125, 0.0]


def _two(c, scans):
    c.map_begin()
    _insert(c, scans["tgt"], scans["Ct"])
    _insert(c, scans["src"], scans["Cs"], scans["T"])
    return c


def _by_key(vm):
    o = S.key_order(vm[0])
    return tuple(np.asarray(x)[o] for x in vm)


def _bits_equal(a, b):
    return all(np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _restored(snap, mode, res, expected_voxels=0, **params):
    c = _handle(mode, res, **params)
    c.map_begin(expected_voxels)
    c.map_import(snap)
    return c


@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("mode", [0, 2])
def test_export_equals_the_map(scans, mode, res):
    a = _two(_handle(mode, res), scans)
    snap, info = a.map_export(), a.map_info()
    vm = _by_key(a.get_voxelmap())
    keys = S.packed_key(snap["coords"])
    assert snap["coords"].dtype == np.int32 and snap["sums"].dtype == np.float64 and snap["ages"].dtype == np.uint32
    assert np.all(keys[1:] > keys[:-1])  # ascending packed key: z-major, then y, then x
    assert np.array_equal(snap["coords"], vm[0])
    assert np.array_equal(snap["sums"][:, 9], vm[1].astype(np.float64))
    rec = S.records(snap)
    s = R.map_spread(rec, vm)
    print("export mode %d res %g: %d voxels, records from the exported sums vs the getters:" % (mode, res, len(keys)), s)
    if mode == 0:
        assert _bits_equal(rec, vm)
    else:
        assert s["mean_excess"] <= EXCESS[2] and s["cov_excess"] <= EXCESS[2]
    Ps, _ = R.transform_cloud(scans["src"], scans["Cs"], scans["T"])
    touched, ok = R.voxel_coords(Ps, res)
    last = np.isin(keys, S.packed_key(touched[ok]))
    assert 0 < last.sum() < len(keys)
    assert np.array_equal(snap["ages"], np.where(last, 0, 1).astype(np.uint32))
    assert (snap["num_voxels"], snap["num_inserts"], snap["num_points"]) == (info["num_voxels"], info["num_inserts"], info["num_points"]) == (len(keys), 2, len(scans["tgt"]) + len(scans["src"]))
    assert snap["resolution"] == res and snap["mode"] == mode
    a.close()


@pytest.mark.parametrize("mode", [0, 2])
def test_restore_on_a_fresh_handle(scans, mode):
    a = _two(_handle(mode), scans)
    snap = a.map_export()
    b = _restored(snap, mode, 1.0)
    assert S.same(b.map_export(), snap)
    assert b.map_info()["dropped"] == 0
    assert _bits_equal(R.sorted_map(b.get_voxelmap()), R.sorted_map(a.get_voxelmap()))
    _prepared_source(a, scans); _prepared_source(b, scans)
    ra, rb = a.align(), b.align()
    print("align on the restored map vs the original: rel_err %.3g, bit-identical %s, iterations %d / %d" % (util.rel_err(rb["T"], ra["T"]), np.array_equal(rb["T"], ra["T"]), rb["nr_iterations"], ra["nr_iterations"]))
    assert ra["converged"] and rb["converged"] and rb["nr_iterations"] == ra["nr_iterations"]
    assert util.rel_err(rb["T"], ra["T"]) <= POSE_TOL
    assert S.same(b.map_export(), snap)  # an align leaves the map alone
    a.close(); b.close()


@pytest.mark.parametrize("mode", [0, 2])
def test_merge_is_exact(scans, mode):
    A, B, one = _handle(mode), _handle(mode), _two(_handle(mode), scans)
    A.map_begin(); _insert(A, scans["tgt"], scans["Ct"])
    B.map_begin(); _insert(B, scans["src"], scans["Cs"], scans["T"])
    ea, eb = A.map_export(), B.map_export()
    ref = S.merge(ea, eb)
    shared = ea["num_voxels"] + eb["num_voxels"] - ref["num_voxels"]
    assert 0 < shared < min(ea["num_voxels"], eb["num_voxels"])  # voxels of both kinds: added into and created
    A.map_merge_from(B)
    em = A.map_export()
    print("merge mode %d: %d + %d voxels, %d shared; sums equal %s, ages equal %s" % (mode, ea["num_voxels"], eb["num_voxels"], shared, np.array_equal(em["sums"], ref["sums"]), np.array_equal(em["ages"], ref["ages"])))
    assert np.array_equal(em["coords"], ref["coords"]) and np.array_equal(em["sums"], ref["sums"]) and np.array_equal(em["ages"], ref["ages"])
    assert S.same(em, ref)
    assert A.map_info()["dropped"] == 0 and A.map_info()["num_voxels"] == ref["num_voxels"]
    assert S.same(B.map_export(), eb)  # the other map is unchanged
    # the host route: a copy of A that imports B's export
    A2 = _restored(ea, mode, 1.0)
    A2.map_import(eb)
    assert S.same(A2.map_export(), em)
    assert _bits_equal(R.sorted_map(A2.get_voxelmap()), R.sorted_map(A.get_voxelmap()))
    # against ONE handle that received both inserts: only the order of the fp64 sums differs
    _check_equal(A.get_voxelmap(), one.get_voxelmap(), mode, "merged vs inserted mode %d:" % mode)
    eo = one.map_export()
    assert np.array_equal(eo["coords"], em["coords"]) and np.array_equal(eo["sums"][:, 9], em["sums"][:, 9])
    # B inserted after the merge: the streams were ordered around the read, B grows, A does not
    _insert(B, scans["tgt"], scans["Ct"], SHIFT)
    assert S.same(A.map_export(), em) and B.map_info()["num_inserts"] == 2
    for c in (A, B, A2, one):
        c.close()


def test_import_grows_a_tiny_table(scans):
    a = _two(_handle(), scans)
    snap = a.map_export()
    b = _handle()
    b.map_begin(expected_voxels=16)
    cap0 = b.map_info()["capacity"]
    b.map_import(snap)
    info = b.map_info()
    print("growth: capacity %d -> %d for %d voxels" % (cap0, info["capacity"], info["num_voxels"]))
    assert info["capacity"] > cap0 and info["capacity"] >= 2 * info["num_voxels"] and info["dropped"] == 0 and info["num_voxels"] == snap["num_voxels"]
    assert S.same(b.map_export(), snap)
    # ... and merge_from into a tiny table
    c = _handle()
    c.map_begin(expected_voxels=16)
    c.map_merge_from(a)
    info = c.map_info()
    assert info["capacity"] >= 2 * info["num_voxels"] and info["dropped"] == 0
    assert S.same(c.map_export(), snap)
    for h in (a, b, c):
        h.close()


def test_duplicate_rows_add_up(scans):
    a = _handle()
    a.map_begin(); _insert(a, scans["tgt"], scans["Ct"])
    snap = a.map_export()
    twice = dict(snap, coords=np.concatenate([snap["coords"], snap["coords"][::-1]]), sums=np.concatenate([snap["sums"], snap["sums"][::-1]]),
                 ages=np.concatenate([snap["ages"], snap["ages"][::-1]]), num_points=2 * snap["num_points"])
    b = _restored(twice, 0, 1.0)
    e2 = b.map_export()
    assert np.array_equal(e2["coords"], snap["coords"]) and np.array_equal(e2["sums"], 2.0 * snap["sums"]) and np.array_equal(e2["ages"], snap["ages"])
    assert e2["num_points"] == 2 * snap["num_points"] and b.map_info()["num_voxels"] == snap["num_voxels"] and b.map_info()["dropped"] == 0
    va, vb = R.sorted_map(a.get_voxelmap()), R.sorted_map(b.get_voxelmap())
    assert np.array_equal(vb[1], 2 * va[1])
    assert _bits_equal((va[0], va[2], va[3]), (vb[0], vb[2], vb[3]))  # 2s * 1/(2n) is exact
    a.close(); b.close()


def test_ages_survive(scans):
    def three(c):
        _two(c, scans)
        _insert(c, scans["tgt"], scans["Ct"], SHIFT)
        return c

    for max_age in (1, 2):
        # (a fresh original per rule, restored from ITS snapshot: two runs of the same inserts differ in the order of their fp64 atomics)
        a = three(_handle())
        snap = a.map_export()
        assert sorted(set(snap["ages"])) == [0, 1, 2]
        b = _restored(snap, 0, 1.0)
        ra, rb = a.map_prune(None, 0.0, max_age), b.map_prune(None, 0.0, max_age)
        print("age prune max_age %d: removed %d (original) / %d (restored)" % (max_age, ra, rb))
        assert ra == rb == int((snap["ages"] >= max_age).sum()) > 0
        ea, eb = a.map_export(), b.map_export()
        assert np.array_equal(ea["coords"], snap["coords"][snap["ages"] < max_age])
        assert S.same(ea, eb)
        a.close(); b.close()
    # a distance prune after a merge keeps exactly prune_keep's set
    A, B = _handle(), _handle()
    A.map_begin(); _insert(A, scans["tgt"], scans["Ct"])
    B.map_begin(); _insert(B, scans["src"], scans["Cs"], scans["T"])
    A.map_merge_from(B)
    em = A.map_export()
    center, radius = np.array([1.0, -2.0, 0.5]), 20.0
    keep, slack = R.prune_keep(em["coords"], 1.0, center, radius)
    assert slack > 1e-9 and 0 < keep.sum() < len(keep)
    assert A.map_prune(center, radius, 0) == int((~keep).sum())
    ep = A.map_export()
    assert np.array_equal(ep["coords"], em["coords"][keep]) and np.array_equal(ep["sums"], em["sums"][keep]) and np.array_equal(ep["ages"], em["ages"][keep])
    A.close(); B.close()


def test_import_keeps_the_occupancy_bitmap_right(scans):
    """bitmap_min_points = 1: the first insert gives the map a bitmap; imported voxels inside its box set their bit, one outside it switches the
    bitmap off. A stale bitmap shows as lost correspondences and another pose."""
    src_map = _handle()
    src_map.map_begin(); _insert(src_map, scans["src"], scans["Cs"], scans["T"])
    inside = src_map.map_export()
    src_map.close()
    tc, ok = R.voxel_coords(scans["tgt"], 1.0)  # the bitmap's box holds at least the bounding box of the first scan's voxels
    box = np.all((inside["coords"] >= tc[ok].min(axis=0)) & (inside["coords"] <= tc[ok].max(axis=0)), axis=1)
    new = ~np.isin(S.packed_key(inside["coords"]), S.packed_key(tc[ok]))
    assert (box & new).sum() > 100  # voxels the import CREATES inside the box
    inside = dict(inside, coords=inside["coords"][box], sums=inside["sums"][box], ages=inside["ages"][box], num_voxels=int(box.sum()))
    far = dict(inside, coords=np.array([[3000, -2500, 40]], np.int32), sums=inside["sums"][:1].copy(), ages=np.zeros(1, np.uint32), num_points=int(inside["sums"][0, 9]))
    out = []
    for params in (dict(bitmap_min_points=1), dict()):
        c = _handle(**params)
        c.map_begin(); _insert(c, scans["tgt"], scans["Ct"])
        _prepared_source(c, scans)
        stages = []
        for snap in (inside, far):
            c.map_import(snap)
            r = c.align()
            c.update_correspondences(r["T"])
            stages.append((r, c.get_num_correspondences()))
        out.append((stages, c.map_export()))
        c.close()
    (with_bitmap, e1), (without, e0) = out
    # (two independent inserts of the first scan: the fp64 sums may differ in their last bits, the voxels, counts and ages may not)
    assert all(np.array_equal(e1[k], e0[k]) for k in ("coords", "ages")) and np.array_equal(e1["sums"][:, 9], e0["sums"][:, 9])
    assert all(e1[k] == e0[k] for k in ("num_voxels", "num_inserts", "num_points")) and e1["num_voxels"] > inside["num_voxels"] + 1
    for what, (r1, n1), (r0, n0) in zip(("voxels inside the box", "a voxel outside it"), with_bitmap, without):
        print("bitmap, %s: correspondences %d vs %d, rel_err %.3g" % (what, n1, n0, util.rel_err(r1["T"], r0["T"])))
        assert n1 == n0 > 0 and r1["nr_iterations"] == r0["nr_iterations"]
        assert util.rel_err(r1["T"], r0["T"]) <= POSE_TOL


def test_refusals_leave_the_map_as_it_was(scans):
    from fast_gicp_amd import capi
    c = _handle()

    def refused(code, word, fn, *args, **kw):
        with pytest.raises(capi.FvhError) as ei:
            fn(*args, **kw)
        assert "status %d" % code in str(ei.value) and word in str(ei.value), str(ei.value)

    good = _two(_handle(), scans)
    snap = good.map_export()
    # no live map
    refused(BAD_STATE, "map_begin", c.map_export)
    refused(BAD_STATE, "map_begin", c.map_import, snap)
    refused(BAD_STATE, "map_begin", c.map_merge_from, good)
    refused(BAD_STATE, "other handle", good.map_merge_from, c)
    assert S.same(good.map_export(), snap)
    # multi-GPU handles, CUDA_COMPAT, map sharding (none of them can hold a live map: the refusal comes first)
    other = _handle()
    exports = [h.peer_export(len(scans["tgt"])) for h in (c, other)]
    for rank, h in enumerate((c, other)):
        h.peer_attach(2, rank, 2, [x for x, _ in exports], [p for _, p in exports])
    for fn, args in ((c.map_export, ()), (c.map_import, (snap,)), (c.map_merge_from, (good,)), (good.map_merge_from, (c,))):
        refused(UNSUPPORTED, "multi-GPU", fn, *args)
    for h in (c, other):
        h.peer_detach()
    other.close()
    c.set_precision(capi.COMPUTE_CUDA_COMPAT)
    for fn, args in ((c.map_export, ()), (c.map_import, (snap,)), (c.map_merge_from, (good,)), (good.map_merge_from, (c,))):
        refused(UNSUPPORTED, "CUDA_COMPAT", fn, *args)
    c.set_precision(capi.COMPUTE_FP64)
    c.set_target_map_sharding(True)
    for fn, args in ((c.map_export, ()), (c.map_import, (snap,)), (c.map_merge_from, (good,)), (good.map_merge_from, (c,))):
        refused(UNSUPPORTED, "shard", fn, *args)
    c.set_target_map_sharding(False)
    assert S.same(good.map_export(), snap)

    # invalid input: each refusal leaves the live map byte-equal
    c.map_begin(); c.map_import(snap)
    before = c.map_export()
    assert S.same(before, snap)
    lim = (1 << 20) - 4096

    def row(**change):
        s = dict(snap, coords=snap["coords"][:3].copy(), sums=snap["sums"][:3].copy(), ages=snap["ages"][:3].copy(), num_points=5)
        for k, v in change.items():
            if k in ("coords", "sums", "ages"):
                s[k][1] = v if k == "ages" else np.where(np.isnan(np.asarray(v, np.float64)), s[k][1], v)  # (NaN in `v`: keep the entry)
            else:
                s[k] = v
        return s

    keep = np.nan
    cases = [("resolution", row(resolution=0.5)), ("resolution", row(resolution=np.nextafter(1.0, 2.0))), ("mode", row(mode=2)), ("mode", row(mode=1)),
             ("coordinate", row(coords=[lim, 0, 0])), ("coordinate", row(coords=[0, -lim, 0])), ("coordinate", row(coords=[0, 0, 1 << 30])),
             ("count", row(sums=[keep] * 9 + [0.0])), ("count", row(sums=[keep] * 9 + [2.5])), ("count", row(sums=[keep] * 9 + [-3.0])),
             ("age", row(ages=snap["num_inserts"])), ("age", row(ages=0, num_inserts=0)), ("negative", row(num_inserts=-1)), ("negative", row(num_points=-1))]
    for j, v in ((0, np.inf), (4, -np.inf), (9, np.inf)):
        s = row(); s["sums"][2, j] = v
        cases.append(("finite" if j != 9 else "", s))
    s = row(); s["sums"][0, 7] = np.nan
    cases.append(("finite", s))
    for word, s in cases:
        refused(BAD_ARG, word, c.map_import, s)
        assert S.same(c.map_export(), before), word
    ok = row(coords=[lim - 1, 1 - lim, 0])  # the largest coordinates an inserted point can have are accepted
    probe = _restored(ok, 0, 1.0)
    assert probe.map_info()["num_voxels"] == 3 and probe.map_info()["dropped"] == 0
    probe.close()
    # what the Python wrapper cannot form: n < 0, NULL arrays with n > 0, more than 2^28 rows (refused before a row is read)
    raw = c._lib.fvh_vgicp_voxelmap_import
    co, su, ag = snap["coords"], snap["sums"], snap["ages"]
    tail = (C.c_double(1.0), 0, snap["num_inserts"], C.c_longlong(0))
    assert raw(c.h, -1, capi._p(co), capi._p(su), capi._p(ag), *tail) == BAD_ARG
    assert raw(c.h, 3, None, capi._p(su), capi._p(ag), *tail) == BAD_ARG
    assert raw(c.h, 3, capi._p(co), None, capi._p(ag), *tail) == BAD_ARG
    assert raw(c.h, (1 << 28) + 1, capi._p(co), capi._p(su), capi._p(ag), *tail) == UNSUPPORTED
    assert raw(c.h, 0, None, None, None, *tail) == 0  # nothing to add is not an error
    assert c._lib.fvh_vgicp_voxelmap_merge_from(c.h, None) == BAD_ARG
    nv = C.c_int(0)
    assert c._lib.fvh_vgicp_voxelmap_export(c.h, C.byref(nv), None, None, None, None, capi._p(co.copy()), None, None) == BAD_ARG  # the three arrays go together
    assert S.same(c.map_export(), before)
    # merge_from: itself, another resolution, another mode
    refused(BAD_ARG, "itself", c.map_merge_from, c)
    half = _handle(0, 0.5); half.map_begin(); _insert(half, scans["tgt"], scans["Ct"])
    mult = _handle(2, 1.0); mult.map_begin(); _insert(mult, scans["tgt"], scans["Ct"])
    refused(BAD_ARG, "resolution", c.map_merge_from, half)
    refused(BAD_ARG, "mode", c.map_merge_from, mult)
    assert S.same(c.map_export(), before)
    # an align_async in flight on either handle
    _prepared_source(c, scans)
    c.align_async()
    refused(BAD_STATE, "align_async", c.map_export)
    refused(BAD_STATE, "align_async", c.map_import, snap)
    refused(BAD_STATE, "align_async", c.map_merge_from, good)
    refused(BAD_STATE, "align_async", good.map_merge_from, c)
    assert c.align_wait()["converged"]
    assert S.same(c.map_export(), before) and S.same(good.map_export(), snap)
    # the handle is usable: the refused merge now goes through
    c.map_merge_from(good)
    assert np.array_equal(c.map_export()["sums"], 2.0 * snap["sums"])
    for h in (c, good, half, mult):
        h.close()


def test_files_and_upper_layers(scans, tmp_path):
    import pygicp
    from fast_gicp_amd import capi
    A, B = capi.VGICPCore(0), capi.VGICPCore(0)  # (the engine's own defaults, as pygicp.FastVGICPCuda() runs on them)
    A.map_begin(); _insert(A, scans["tgt"], scans["Ct"])
    B.map_begin(); _insert(B, scans["src"], scans["Cs"], scans["T"])
    pa, pb = str(tmp_path / "a.fvhmap"), str(tmp_path / "b.fvhmap")
    A.map_save(pa); B.map_save(pb)
    ea, eb = A.map_export(), B.map_export()
    assert S.same(capi.read_map_file(pa), ea)
    # a fresh handle with no live map (and another resolution): map_load starts one from the file
    L = capi.VGICPCore(0)
    L.set_resolution(0.5)
    L.map_load(pa)
    assert S.same(L.map_export(), ea) and L.map_info()["capacity"] >= 2 * ea["num_voxels"]
    _prepared_source(L, scans)
    rc = L.align()
    # the same file through pygicp
    reg = pygicp.FastVGICPCuda()
    reg.load_target_map(pa)
    ep = reg.export_target_map()
    assert S.same({k: (np.asarray(v) if k in ("coords", "sums", "ages") else v) for k, v in ep.items()}, ea)
    reg.set_input_source(scans["src"].astype(np.float64))
    Tp = reg.align().astype(np.float64)
    Tc32 = rc["T"].astype(np.float32).astype(np.float64)  # (pygicp hands the pose back as float32: held against the float32 of capi's)
    print("pygicp on the loaded map vs capi: rel_err %.3g (bit-identical %s)" % (util.rel_err(Tp, Tc32), np.array_equal(Tp, Tc32)))
    assert reg.has_converged() and rc["converged"]
    assert util.rel_err(Tp, Tc32) <= POSE_TOL
    # save from pygicp: the same bytes
    pp = str(tmp_path / "p.fvhmap")
    reg.save_target_map(pp)
    assert open(pp, "rb").read() == open(pa, "rb").read()
    # merge_target_from equals capi's merge; import_target_map equals the host route
    other = pygicp.FastVGICPCuda()
    other.load_target_map(pb)
    reg.merge_target_from(other)
    A.map_merge_from(B)
    em = A.map_export()
    ep = reg.export_target_map()
    assert S.same({k: (np.asarray(v) if k in ("coords", "sums", "ages") else v) for k, v in ep.items()}, em)
    third = pygicp.FastVGICPCuda()
    third.begin_incremental_target()
    third.import_target_map(ea); third.import_target_map(eb)
    ep = third.export_target_map()
    assert S.same({k: (np.asarray(v) if k in ("coords", "sums", "ages") else v) for k, v in ep.items()}, em)
    for h in (A, B, L):
        h.close()
