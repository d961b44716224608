"""align_multi (fvh_vgicp_align_multi / fvh_ndt_align_multi): K initial guesses of one source / target pair in one launch of the gang
kernel. Every hypothesis must be, bit for bit, what a plain align(guess k) returns under the same grid plan (cost_max_blocks =
grid_blocks), on every route (persistent, one launch per transition, watchdog abort + redo), and the handle must be left where the
sequential loop leaves it."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

YAWS = [0.0, 15.0, -15.0, 30.0, -30.0, 60.0, -60.0, 180.0]
FIELDS = ("T", "H", "final_error", "converged", "nr_iterations", "num_linearize", "num_error_evals")
LM_CAPPED = dict(max_iterations=12)  # short enough that the far guesses end by max_iterations


def yaw(deg, base=None):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T if base is None else T @ base


def guesses(k):
    return np.stack([yaw(d) for d in YAWS[:k]])


def same(m, s, what=""):
    for f in FIELDS:
        assert np.array_equal(np.asarray(m[f]), np.asarray(s[f])), (what, f, m[f], s[f])


def vgicp(search, precision=None, **params):
    from fast_gicp_amd import capi
    tgt, src = util.bundled_pair()
    c = capi.VGICPCore(0)
    if params:
        c.set_engine_params(**params)
    if precision is not None:
        c.set_precision(precision)
    c.set_neighbor_search_method(search)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(); c.create_target_voxelmap()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
    return c


def sequential(c, G, nb, **lm):
    """align(guess k) for every k on handle c with cost_max_blocks = nb (restored afterwards)"""
    old = c.get_engine_params().cost_max_blocks
    c.set_engine_params(cost_max_blocks=nb)
    out = [c.align(g, **lm) for g in G]
    c.set_engine_params(cost_max_blocks=old)
    return out


@pytest.fixture(scope="module")
def direct_handles():
    from fast_gicp_amd import capi
    hs = {s: (vgicp(s), vgicp(s)) for s in (capi.DIRECT1, capi.DIRECT7, capi.DIRECT27)}
    yield hs
    for a, b in hs.values():
        a.close(); b.close()


@pytest.mark.parametrize("search", ["DIRECT1", "DIRECT7", "DIRECT27"])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_vgicp_multi_is_bit_identical_to_sequential_aligns(direct_handles, search, k):
    from fast_gicp_amd import capi
    a, b = direct_handles[getattr(capi, search)]
    G = guesses(k)
    for lm in (LM_CAPPED, {}):
        ms = a.align_multi(G, **lm)
        assert len(ms) == k
        nb = ms[0]["grid_blocks"]
        assert nb >= 1 and all(m["grid_blocks"] == nb for m in ms)
        for i, s in enumerate(sequential(b, G, nb, **lm)):
            same(ms[i], s, (search, k, i, lm))
        if k == 8 and lm is LM_CAPPED:
            # the hypotheses are not all alike: one ends by max_iterations unconverged, the converged ones took different numbers of trips
            assert any(not m["converged"] and m["nr_iterations"] == LM_CAPPED["max_iterations"] - 1 for m in ms), [(m["converged"], m["nr_iterations"]) for m in ms]
            assert len({m["num_error_evals"] for m in ms}) > 1
    if k == 1:  # K = 1 is a plain align with the default plan and parameters
        same(a.align_multi(G)[0], b.align(G[0]), "k=1 default")


@pytest.mark.parametrize("route", ["multi_launch", "watchdog_abort", "gauss_newton"])
def test_routes_agree_bit_for_bit(route):
    from fast_gicp_amd import capi
    params = {"multi_launch": dict(persistent=0), "watchdog_abort": dict(persist_watchdog_ticks=0), "gauss_newton": {}}[route]
    lm = dict(LM_CAPPED, optimizer=1) if route == "gauss_newton" else LM_CAPPED
    a, b = vgicp(capi.DIRECT7, **params), vgicp(capi.DIRECT7)
    G = guesses(8)
    ms = a.align_multi(G, **lm)
    nb = ms[0]["grid_blocks"]
    if route != "gauss_newton":
        assert all(m["num_launches"] > 1 for m in ms), [m["num_launches"] for m in ms]  # one launch per transition
    if route == "watchdog_abort":
        assert a.debug_persist_aborts() == 1
    for i, s in enumerate(sequential(b, G, nb, **lm)):
        same(ms[i], s, (route, i))
    a.close(); b.close()


def _ndt(mode, tgt, src, res=1.0, search=1):
    from fast_gicp_amd import capi
    c = capi.NDTCore(0)
    c.set_distance_mode(mode); c.set_neighbor_search_method(search); c.set_resolution(res)
    c.set_target_cloud(tgt); c.set_source_cloud(src)
    return c


def _check_same_handle(c, G, **lm):
    c.align(G[0], **lm)  # warm: the D2D grid is shaped by the source voxel count the last align saw
    ms = c.align_multi(G, **lm)
    for i, s in enumerate(sequential(c, G, ms[0]["grid_blocks"], **lm)):
        same(ms[i], s, i)
    return ms


@pytest.mark.parametrize("mode", ["P2D", "D2D"])
def test_ndt_multi_is_bit_identical(mode):
    from fast_gicp_amd import capi
    tgt, src = util.bundled_pair()
    c = _ndt(getattr(capi, "NDT_" + mode), tgt, src, search=capi.DIRECT7)
    _check_same_handle(c, guesses(8), **LM_CAPPED)
    _check_same_handle(c, guesses(3))
    c.close()


def test_ndt_lidar_stream_frame_from_the_voxel_grid_filter():
    import torch
    from fast_gicp_amd import capi
    raw = [util.lidar_frame(i) for i in range(2)]
    d = [torch.from_numpy(f).to("cuda:0").contiguous() for f in raw]
    vg = capi.VoxelGrid(0)
    c = capi.NDTCore(0)
    c.set_distance_mode(capi.NDT_D2D); c.set_neighbor_search_method(capi.DIRECT1); c.set_resolution(1.0)
    ptr, n = vg.filter_device(d[0].data_ptr(), len(raw[0]), 0.25)
    c.set_target_cloud_device(ptr, n, 3)
    ptr, n = vg.filter_device(d[1].data_ptr(), len(raw[1]), 0.25)
    c.set_source_cloud_device(ptr, n, 3)
    torch.cuda.synchronize()
    G = np.stack([yaw(y) for y in (0.0, 5.0, -5.0, 20.0)])
    ms = _check_same_handle(c, G)
    assert ms[0]["converged"]
    c.close(); vg.close()


@pytest.mark.parametrize("precision", ["COMPUTE_FP32", "COMPUTE_CUDA_COMPAT"])
def test_other_precisions(precision):
    from fast_gicp_amd import capi
    p = getattr(capi, precision)
    a, b = vgicp(capi.DIRECT7, precision=p), vgicp(capi.DIRECT7, precision=p)
    G = guesses(3)
    ms = a.align_multi(G)
    for i, s in enumerate(sequential(b, G, ms[0]["grid_blocks"])):
        same(ms[i], s, (precision, i))
    a.close(); b.close()


def test_large_map_gangs_shrink_to_be_coresident():
    from fast_gicp_amd import capi, workloads
    tgt, src, _ = workloads.synthetic_pair(1_000_000, 100_000, seed=44, extent=150.0)
    c = capi.VGICPCore(0)
    c.set_resolution(0.5); c.set_neighbor_search_method(capi.DIRECT7)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(); c.create_target_voxelmap()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
    plain = c.align()
    nb_plain, cap = c.debug_persist_grid()
    assert plain["num_launches"] == 1
    K = 4
    assert K * nb_plain > cap  # the single align's plan does not fit K times
    G = np.stack([yaw(y) for y in (0.0, 2.0, -2.0, 5.0)])
    ms = c.align_multi(G)
    nb = ms[0]["grid_blocks"]
    assert K * nb <= cap and nb >= 8 and nb < nb_plain
    assert all(m["num_launches"] == 1 for m in ms)  # the persistent route, with smaller gangs
    for i, s in enumerate(sequential(c, G, nb)):
        same(ms[i], s, i)
    c.close()


def test_later_calls_see_the_handle_the_sequential_loop_leaves():
    from fast_gicp_amd import capi
    c = vgicp(capi.DIRECT7)
    G = guesses(3)
    T_probe = yaw(3.0)
    ms = c.align_multi(G)
    e1 = c.compute_error(T_probe)
    r1 = c.align(G[1])
    seq = sequential(c, G, ms[0]["grid_blocks"])
    for i, s in enumerate(seq):
        same(ms[i], s, i)
    e2 = c.compute_error(T_probe)
    r2 = c.align(G[1])
    assert e1[0] == e2[0] and np.array_equal(e1[1], e2[1]) and np.array_equal(e1[2], e2[2])
    same(r1, r2, "next align")
    c.close()


def test_two_threads_share_the_slot_pool():
    from fast_gicp_amd import capi
    hs = [vgicp(capi.DIRECT27), vgicp(capi.DIRECT27)]
    G = [guesses(4), np.stack([yaw(y) for y in (5.0, -5.0, 45.0, -45.0)])]
    out = [None, None]
    barrier = threading.Barrier(2)

    def run(i):
        barrier.wait()
        out[i] = [hs[i].align_multi(G[i]) for _ in range(3)]

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert all(o is not None for o in out)
    time.sleep(0.1)  # the slot pool forgets the burst (SlotPool::QUIET_RESET_MS): the lone reference aligns get the whole chip again
    for i in range(2):
        for ms in out[i]:
            for k, s in enumerate(sequential(hs[i], G[i], ms[0]["grid_blocks"])):
                same(ms[k], s, (i, k))
    for h in hs:
        h.close()


def _raw(c, k, g, res=None, nb=None):
    from fast_gicp_amd import capi
    fn = getattr(c._lib, c._prefix + "align_multi")
    res = res if res is not None else (capi.LmResult * 64)()
    return fn(c.h, k, g, None, res, nb)


def test_refusals_leave_the_handle_usable():
    from fast_gicp_amd import capi
    c, ref = vgicp(capi.DIRECT7), vgicp(capi.DIRECT7)
    g = np.ascontiguousarray(np.tile(np.eye(4).ravel(), 65))
    gp = C.c_void_p(g.ctypes.data)
    assert _raw(c, 0, gp) == 1 and _raw(c, 65, gp) == 1          # k out of range
    assert _raw(c, 2, None) == 1                                  # null guesses
    assert c._lib.fvh_vgicp_align_multi(c.h, 2, gp, None, None, None) == 1  # null results
    bad = g.copy(); bad[16 + 5] = np.nan
    assert _raw(c, 2, C.c_void_p(bad.ctypes.data)) == 1           # non-finite guess
    c.align_async()
    assert _raw(c, 2, gp) == 2                                    # an align_async in flight
    c.align_wait()
    G = guesses(3)
    ms = c.align_multi(G)
    for i, s in enumerate(sequential(ref, G, ms[0]["grid_blocks"])):
        same(ms[i], s, i)
    # tiled NDT: not supported
    tgt, src = util.bundled_pair()
    n = _ndt(capi.NDT_D2D, tgt, src)
    n.set_source_tile(0, 2)
    assert _raw(n, 2, gp) == 4
    n.set_source_tile(0, 1)
    _check_same_handle(n, guesses(2))
    c.close(); ref.close(); n.close()


def test_two_hypotheses_match_the_cpu_oracle():
    from fast_gicp_amd import capi
    from oracle import oracle as O
    tgt, src = util.bundled_pair()
    c = vgicp(capi.DIRECT7)
    G = np.stack([yaw(0.0), yaw(4.0)])
    ms = c.align_multi(G)
    g = O.FastVGICP(search=O.DIRECT7)
    g.set_target(tgt); g.set_source(src)
    for i in range(2):
        ro = g.align(G[i])
        assert ms[i]["converged"] and ro["converged"]
        assert util.rel_err(ms[i]["T"], ro["T"]) < 1e-4, (i, ms[i]["T"], ro["T"])
    c.close()


def test_pygicp_align_multi_and_align_best():
    import pygicp
    t, s = util.bundled_pair(origin_filter=False, leaf=0.2, exact_voxelgrid=True)
    target, source, gt = t.astype(np.float64), s.astype(np.float64), util.relative_pose()
    R = yaw(100.0)
    turned = source @ R[:3, :3].T  # the source yawed by 100 degrees: the true pose becomes gt R^-1
    gt_turned = gt @ np.linalg.inv(R)
    for make in (pygicp.FastVGICPCuda, pygicp.NDTCuda):
        reg = make()
        reg.set_input_target(target); reg.set_input_source(source)
        G = np.stack([yaw(d) for d in (0.0, 10.0, -10.0)])
        T, err, conv, its = reg.align_multi(G)
        assert T.shape == (3, 4, 4) and T.dtype == np.float64 and err.shape == (3,) and conv.dtype == np.bool_ and its.shape == (3,)
        for k in range(3):  # each hypothesis is align(guess k)
            Tk = reg.align(G[k])
            assert np.array_equal(T[k].astype(np.float32), Tk) and conv[k] == reg.has_converged()
        reg.set_input_source(turned)
        te, re_ = util.pose_error(gt_turned, reg.align().astype(np.float64))
        assert te > 0.05 or re_ > np.radians(1.0), (te, re_)  # from identity, align() does not find the pose
        G12 = np.stack([yaw(30.0 * i) for i in range(12)])
        Tb, idx = reg.align_best(G12)
        te, re_ = util.pose_error(gt_turned, np.asarray(Tb, np.float64))
        assert te < 0.05 and re_ < np.radians(1.0), (make, idx, te, re_)
        assert np.array_equal(Tb, reg.get_final_transformation())


# ---- the branches the shared host-side LM driver merges (table-overflow rerun, degenerate launch, back-off, result transport) ----
def _small(res=None, hint=None, **params):
    """the small synthetic pair of test_gpu_robustness.py, prepared as there: several workgroups, several groups, a ragged last tile"""
    from fast_gicp_amd import capi
    tgt, src, _ = util.synthetic_pair(4000, 3500, seed=3, extent=12.0)
    c = capi.VGICPCore(0)
    if params:
        c.set_engine_params(**params)
    if res is not None:
        c.set_resolution(res)
    c.set_neighbor_search_method(1)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(3)
    if hint is not None:
        c.debug_set_voxel_hint(hint)
    c.create_target_voxelmap()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances(3)
    return c


def test_multi_table_overflow_reruns_on_the_rebuilt_map():
    c = _small(res=0.25, hint=1)  # 1,024 buckets for a few thousand voxels
    assert c.debug_table_capacity() == 1024
    G = guesses(3)
    ms = c.align_multi(G)
    assert c.debug_table_capacity() > 1024
    assert all(m["num_launches"] > 1 for m in ms), [m["num_launches"] for m in ms]  # the rerun: one launch per transition
    for i, s in enumerate(sequential(c, G, ms[0]["grid_blocks"])):  # (the same handle: the same rebuilt map)
        same(ms[i], s, i)
    c.close()


def test_multi_without_iterations_returns_the_guesses():
    a, b, fresh = _small(), _small(), _small()
    G = guesses(3)
    ms = a.align_multi(G, max_iterations=0)
    for k, m in enumerate(ms):
        assert np.array_equal(m["T"], G[k]), (k, m["T"], G[k])
        assert m["num_linearize"] == 0 and m["num_error_evals"] == 0 and m["nr_iterations"] == 0, m
        same(m, b.align(G[k], max_iterations=0), k)
    after, ref = a.align_multi(G), fresh.align_multi(G)
    for k in range(3):
        same(after[k], ref[k], ("after", k))
        assert after[k]["grid_blocks"] == ref[k]["grid_blocks"]
    a.close(); b.close(); fresh.close()


def test_multi_abort_backs_off_the_next_plain_align():
    from fast_gicp_amd import capi
    a, fresh = _small(persist_watchdog_ticks=0), _small()
    a.align_multi(guesses(3))
    assert a.debug_persist_aborts() == 1
    a.set_engine_params(persist_watchdog_ticks=capi.default_engine_params().persist_watchdog_ticks)
    r1, r2, r0 = a.align(), a.align(), fresh.align()
    assert r1["num_launches"] > 1, r1["num_launches"]   # skipped the persistent route once ...
    assert r2["num_launches"] == 1, r2["num_launches"]  # ... and took it again
    assert a.debug_persist_aborts() == 1
    assert np.array_equal(r1["T"], r0["T"]) and np.array_equal(r2["T"], r0["T"])
    a.close(); fresh.close()


def test_multi_result_transports_agree():
    c = _small()
    G = guesses(3)
    ref = c.align_multi(G)
    assert all(m["num_launches"] == 1 for m in ref)
    for params in (dict(zerocopy_result=0), dict(zerocopy_result=1, host_wait_block=1)):
        c.set_engine_params(**params)
        ms = c.align_multi(G)
        for k in range(3):
            same(ms[k], ref[k], (params, k))
            assert ms[k]["num_launches"] == 1, (params, ms[k]["num_launches"])
    c.close()
