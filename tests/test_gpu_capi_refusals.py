"""The entry points fvh_vgicp_* and fvh_ndt_* share, characterised on both handle types: a handle is put into a named state, one call is
made, and (status, full last_error text) -- for a call that succeeds: (0, what it returned) -- is compared with
tests/golden/capi_refusals.json. The fixture holds the answers of the build of the commit it names (the parent of the change that put the
two prefixes on one set of bodies): a refusal that moves, wins over another one or changes a word shows up here.

    python -m tests.test_gpu_capi_refusals --record OUT.json --commit HASH     (on a build of commit HASH, with a GPU)

64-point clouds at a resolution of 1.0; every row is a clean refusal or a clean success, and after every refused call the handle still
completes an align()."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from tests import util

GOLDEN = os.path.join(util.ROOT, "tests", "golden", "capi_refusals.json")
KINDS = ("vgicp", "ndt")
N = 64
_I16 = np.ascontiguousarray(np.eye(4))


def _clouds():
    rng = np.random.default_rng(20240)
    tgt = (rng.random((N, 3)) * [4.0, 4.0, 2.0]).astype(np.float32)
    src = (tgt + np.float32(0.05) + rng.normal(0.0, 0.01, (N, 3))).astype(np.float32)
    covs = np.ascontiguousarray(np.tile(np.diag([0.01, 0.01, 0.001]).reshape(1, 9), (N, 1)))
    return tgt, src, covs


class _Bench:
    """One handle type's table: the states, the rows run on each, what came back."""

    def __init__(self, kind):
        from fast_gicp_amd import capi
        self.capi, self.kind = capi, kind
        self.cls = capi.VGICPMapCore if kind == "vgicp" else capi.NDTMapCore
        self.own_mode = capi.VOXEL_ADDITIVE if kind == "vgicp" else capi.VOXEL_NDT_SUMS
        self.other_mode = capi.VOXEL_NDT_SUMS if kind == "vgicp" else capi.VOXEL_ADDITIVE
        self.tgt, self.src, self.covs = _clouds()
        self.rows = {}
        self.handles = []

    # ---- handles ----
    def make(self, precision=None, shard_map=False, clouds=True, target=True, resolution=1.0):
        capi = self.capi
        c = self.cls(0)
        self.handles.append(c)
        c.set_resolution(resolution); c.set_neighbor_search_method(capi.DIRECT7); c.set_engine_params(side_stream=0)
        if precision is not None:
            c.set_precision(precision)
        if shard_map:
            c.set_target_map_sharding(True, 2)
        if not clouds:
            return c
        if self.kind == "vgicp":
            if target:
                c.set_target_cloud(self.tgt); c.find_target_neighbors(10); c.calculate_target_covariances(); c.create_target_voxelmap()
            c.set_source_cloud(self.src); c.find_source_neighbors(10); c.calculate_source_covariances()
        else:
            if target:
                c.set_target_cloud(self.tgt)
            c.set_source_cloud(self.src)
        return c

    def live(self, resolution=1.0):
        c = self.make(target=False, resolution=resolution)
        c.map_begin(); c.map_insert_source()
        return c

    def close(self):
        for c in self.handles:
            c.close()

    # ---- one call ----
    def raw(self, c, name, *args):
        rc = getattr(c._lib, c._prefix + name)(c.h, *args)
        return rc, (getattr(c._lib, c._prefix + "last_error")(c.h).decode() if rc else None)

    def align_ok(self, c):
        r = self.capi.LmResult()
        rc, msg = self.raw(c, "align", self.capi._p(_I16), C.byref(self.capi._DEFAULT_LM), C.byref(r))
        assert rc == 0, (rc, msg)
        assert np.isfinite(np.frombuffer(r, dtype=np.float64, count=16)).all()

    def row(self, state, name, c, call_name, *args, out=None, then=None):
        """run one row; `out`: () -> dict of what a successful call returned; `then`: run right after the call"""
        rc, msg = self.raw(c, call_name, *args)
        if then:
            then()
        key = "%s/%s/%s" % (self.kind, state, name)
        assert key not in self.rows, key
        if rc == 0:
            self.rows[key] = {"status": 0, "out": out() if out else {}}
        else:
            self.rows[key] = {"status": rc, "error": msg}
            self.align_ok(c)  # a refusal leaves the handle usable

    # ---- the rows ----
    def map_calls(self, state, c, other, skip=()):
        """every incremental-map call once, on handle `c` in `state` (`other`: a handle of the same type with a live map)"""
        p = self.capi._p
        removed, n_out = C.c_int(-1), C.c_int(-1)
        inc, nv, cap, ni, dr, npts = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
        res, mode = C.c_double(-1.0), C.c_int(-1)
        info = lambda: dict(incremental=inc.value, num_voxels=nv.value, capacity=cap.value, num_inserts=ni.value, num_points=npts.value, num_dropped=dr.value)
        insert_cloud = (p(self.src), N, 3, p(self.covs), p(_I16), 0) if self.kind == "vgicp" else (p(self.src), N, 3, p(_I16), 0)
        calls = [
            ("map_begin", (0,), None),
            ("map_insert_source", (p(_I16),), None),
            ("map_insert_cloud", insert_cloud, None),
            ("map_prune", (None, C.c_double(0.0), 1, C.byref(removed)), lambda: dict(num_removed=removed.value)),
            ("map_get_info", (C.byref(inc), C.byref(nv), C.byref(cap), C.byref(ni), C.byref(npts), C.byref(dr)), info),
            ("voxelmap_export", (C.byref(nv), C.byref(res), C.byref(mode), C.byref(ni), C.byref(npts), None, None, None),
             lambda: dict(num_voxels=nv.value, resolution=res.value, mode=mode.value, num_inserts=ni.value, num_points=npts.value)),
            ("voxelmap_import", (0, None, None, None, C.c_double(1.0), self.own_mode, 0, C.c_longlong(0)), None),
            ("voxelmap_merge_from", (other.h,), None),
            ("target_from_map", (1, C.byref(n_out)), lambda: dict(num_points=n_out.value)),
        ]
        for name, args, out in calls:
            if name not in skip:
                self.row(state, name, c, name, *args, out=out)

    def run(self):
        capi, p = self.capi, self.capi._p
        live_other = self.live()

        # no map begun (map_begin itself succeeds: it is a row of the "live" state)
        c = self.make()
        self.map_calls("no_map", c, live_other, skip=("map_begin",))
        self.row("no_map", "set_precision_bad_value", c, "set_precision", 7)
        self.row("no_map", "set_engine_params_null", c, "set_engine_params", None)
        self.row("no_map", "get_engine_params_null", c, "get_engine_params", None)
        self.row("no_map", "get_lm_trace_null_count", c, "get_lm_trace", None, None)
        self.row("no_map", "set_resolution_zero", c, "set_resolution", C.c_double(0.0))
        self.row("no_map", "set_neighbor_search_method_unknown", c, "set_neighbor_search_method", 99, C.c_double(0.0))

        # no target cloud yet
        c = self.make(clouds=False)
        xyz, n_out = np.zeros((N, 3), np.float32), C.c_int(-1)
        self.row("empty", "get_num_target_points", c, "get_num_target_points", C.byref(n_out), out=lambda: dict(n=n_out.value))
        rc, msg = self.raw(c, "get_target_points", p(xyz))
        self.rows["%s/empty/get_target_points" % self.kind] = {"status": rc, "error": msg}
        if self.kind == "vgicp":
            c.set_target_cloud(self.tgt); c.find_target_neighbors(10); c.calculate_target_covariances(); c.create_target_voxelmap()
            c.set_source_cloud(self.src); c.find_source_neighbors(10); c.calculate_source_covariances()
        else:
            c.set_target_cloud(self.tgt); c.set_source_cloud(self.src)
        self.align_ok(c)

        # FVH_COMPUTE_CUDA_COMPAT handle
        self.map_calls("cuda_compat", self.make(precision=capi.COMPUTE_CUDA_COMPAT), live_other)
        # target-map sharding on (VGICP has it)
        if self.kind == "vgicp":
            self.map_calls("map_sharding", self.make(shard_map=True), live_other)

        # a live map: the success rows, then what is refused on it
        c = self.make(target=False)
        inc, nv, cap, ni, dr, npts = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
        self.row("live", "map_begin", c, "map_begin", 0)
        self.row("live", "map_insert_source", c, "map_insert_source", p(_I16))
        self.row("live", "map_get_info", c, "map_get_info", C.byref(inc), C.byref(nv), C.byref(cap), C.byref(ni), C.byref(npts), C.byref(dr),
                 out=lambda: dict(incremental=inc.value, num_voxels=nv.value, capacity=cap.value, num_inserts=ni.value, num_points=npts.value, num_dropped=dr.value))
        if self.kind == "vgicp":
            self.row("live", "map_insert_cloud_null_covariances", c, "map_insert_cloud", p(self.src), N, 3, None, p(_I16), 0)
        self.row("live", "voxelmap_import_other_types_mode", c, "voxelmap_import", 0, None, None, None, C.c_double(1.0), self.other_mode, 0, C.c_longlong(0))
        self.row("live", "merge_from_null", c, "voxelmap_merge_from", None)
        self.row("live", "merge_from_self", c, "voxelmap_merge_from", c.h)
        self.row("live", "merge_from_no_live_map", c, "voxelmap_merge_from", self.make().h)
        self.row("live", "merge_from_other_resolution", c, "voxelmap_merge_from", self.live(resolution=2.0).h)
        flying = self.make()
        flying.align_async()
        self.row("live", "merge_from_in_flight", c, "voxelmap_merge_from", flying.h, then=flying.align_wait)
        self.row("live", "set_resolution_other", c, "set_resolution", C.c_double(2.0))
        self.row("live", "set_precision_cuda_compat", c, "set_precision", capi.COMPUTE_CUDA_COMPAT)
        self.row("live", "map_get_info_after", c, "map_get_info", C.byref(inc), None, None, C.byref(ni), C.byref(npts), None,
                 out=lambda: dict(incremental=inc.value, num_inserts=ni.value, num_points=npts.value))
        return self.rows


def observe():
    rows = {}
    for kind in KINDS:
        b = _Bench(kind)
        try:
            rows.update(b.run())
        finally:
            b.close()
    return rows


@pytest.fixture(scope="module")
def observed():
    return observe()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_shared_entry_points_answer_as_the_recorded_build_did(kind, observed, golden):
    want = {k: v for k, v in golden["rows"].items() if k.startswith(kind + "/")}
    got = {k: v for k, v in observed.items() if k.startswith(kind + "/")}
    assert len(golden["commit"]) == 40
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


@pytest.mark.gpu
def test_the_table_holds_refusals_and_successes_of_both_types(observed):
    for kind in KINDS:
        rows = {k: v for k, v in observed.items() if k.startswith(kind + "/")}
        refused = [k for k, v in rows.items() if v["status"] != 0]
        assert len(refused) >= 25 and all(rows[k]["error"] for k in refused), (kind, len(refused))
        for state in ("no_map", "cuda_compat") + (("map_sharding",) if kind == "vgicp" else ()):
            for call in ("map_insert_source", "map_insert_cloud", "map_prune", "voxelmap_export", "voxelmap_import", "voxelmap_merge_from"):
                assert rows["%s/%s/%s" % (kind, state, call)]["status"] != 0, (kind, state, call)
        for name in ("map_begin", "map_insert_source", "map_get_info"):
            assert rows["%s/live/%s" % (kind, name)]["status"] == 0, (kind, name)


@pytest.mark.gpu
def test_the_same_sequence_gives_both_types_the_same_counts(observed):
    a, b = (observed["%s/live/map_get_info" % k]["out"] for k in KINDS)
    assert (a["incremental"], a["num_inserts"], a["num_points"]) == (b["incremental"], b["num_inserts"], b["num_points"]) == (1, 1, N)
    a, b = (observed["%s/live/map_get_info_after" % k]["out"] for k in KINDS)  # the refused calls in between changed nothing
    assert a == b == dict(incremental=1, num_inserts=1, num_points=N)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, help="file to write (copy it to tests/golden/capi_refusals.json)")
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    args = ap.parse_args()
    assert len(args.commit) == 40, "--commit takes the full hash"
    json.dump({"commit": args.commit, "source": "python -m tests.test_gpu_capi_refusals --record (the library built from `commit`)", "rows": observe()},
              open(args.record, "w"), indent=1, sort_keys=True)
    print("wrote", args.record, file=sys.stderr)
