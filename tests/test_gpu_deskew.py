"""Motion compensation on the voxel-grid handle (fvh_voxelgrid_deskew) against the fp64 numpy twin of its definition (tests/deskew_ref.py).

Tolerance per coordinate: |dev - twin64| <= 0.5 * spacing(float32(|twin64|)) + 1e-12 * M, M = 1 + max |p| + 2 max |knot translation|. The
first term is the final cast, the second fp64 evaluation-order noise: two fp64 formulations of the twin differ by under 1e-14 M
(tests/test_deskew_cpu.py), and the term stays five orders under a float32 ulp -- an fp32 intermediate on the device fails it. On the
bundled cloud at most 1 coordinate in 1,000 may differ in bits from float32(twin64). No cloud is larger than 4,099 points."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import deskew_ref as R
from tests import util

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def cloud(name="A"):
    from fast_gicp_amd import preprocess
    if name == "A":
        return np.ascontiguousarray(preprocess.bundled_pair(util.DATA)[1][:4099])
    assert name == "lattice"
    return R.cloud_lattice()


@functools.lru_cache(maxsize=None)
def times(name="A"):
    return R.azimuth_times(cloud(name))


@functools.lru_cache(maxsize=None)
def trajectory(K, seed=0):
    """knot times that float32 holds exactly (so that a point's time can sit exactly on a knot)"""
    tau, T = R.random_trajectory(K, seed)
    tau = tau.astype(np.float32).astype(np.float64)
    assert np.all(np.diff(tau) > 0)
    return tau, T


@pytest.fixture(scope="module")
def vg():
    from fast_gicp_amd import capi
    v = capi.VoxelGrid(0)
    yield v
    v.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(out, p, t, tau, T, t_ref, cap=False, what=""):
    ref64, ref32 = R.deskew(p, t, tau, T, t_ref)
    assert out.shape == ref32.shape and out.dtype == np.float32
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(out), nan)
    err = np.abs(np.where(nan, 0.0, out.astype(np.float64) - ref64))
    tol = np.where(nan, 1.0, R.tolerance(np.where(nan, 0.0, ref64), p, T))
    differ = int((out.view(np.uint32) != ref32.view(np.uint32))[~nan].sum())
    print("%s n=%d K=%d t_ref=%s: max err / tol %.3f, %d of %d coordinates differ in bits" % (what, len(p), len(tau), t_ref, float((err / tol).max(initial=0.0)), differ, out.size))
    assert np.all(err <= tol), (what, float((err / tol).max()))
    if cap:
        assert differ * 1000 <= out.size, (what, differ)


# ---- against the twin ----
@pytest.mark.parametrize("K", [2, 3, 64])
def test_bundled_cloud_equals_the_twin_at_every_reference_time(vg, K):
    p, t = cloud(), times()
    tau, T = trajectory(K, 20 + K)
    for t_ref in (None, tau[0], 0.5 * (tau[0] + tau[-1]), tau[-1], -0.02, 0.13):  # start, middle, end, outside the knots on either side
        out = vg.deskew(p, t, tau, T, t_ref)
        check(out, p, t, tau, T, t_ref, cap=True)
        ptr, m = vg.device_points()
        assert m == len(p) and ptr


@pytest.mark.parametrize("n", SIZES)
def test_ragged_sizes(vg, n):
    p, t = cloud()[:n], times()[:n]
    for K in (2, 64):
        tau, T = trajectory(K, 30 + K)
        check(vg.deskew(p, t, tau, T), p, t, tau, T, None)


def test_lattice_cloud(vg):
    p, t = cloud("lattice"), times("lattice")
    assert len(p) == 729 and not p[364].any()  # the origin is one of its points
    for K in (2, 3, 64):
        tau, T = trajectory(K, 40 + K)
        check(vg.deskew(p, t, tau, T, tau[1]), p, t, tau, T, tau[1])


@pytest.mark.parametrize("K", [2, 3, 64])
def test_times_on_before_after_equal_and_descending(vg, K):
    p = cloud()[:1000]
    tau, T = trajectory(K, 50 + K)
    n = len(p)
    on_knots = tau[np.arange(n) % K].astype(np.float32)
    assert np.array_equal(on_knots.astype(np.float64), tau[np.arange(n) % K])
    span = tau[-1] - tau[0]
    cases = {"on knots": on_knots,
             "before the first knot": np.linspace(tau[0] - 0.3 * span, tau[0], n).astype(np.float32),
             "after the last knot": np.linspace(tau[-1], tau[-1] + 0.3 * span, n).astype(np.float32),
             "all equal": np.full(n, np.float32(0.37 * span), np.float32),
             "descending": np.sort(times()[:n])[::-1].copy()}
    for what, t in cases.items():
        check(vg.deskew(p, t, tau, T), p, t, tau, T, None, what=what)
    # before / after really extrapolate: the end segments' twists, not the end poses
    t = cases["after the last knot"]
    frozen = R.deskew(p, np.minimum(t, np.float32(tau[-1])), tau, T)[0]
    assert np.abs(R.deskew(p, t, tau, T)[0] - frozen).max() > 0.1


def _chain(twists_, start=None):
    T = [R.se3_exp([0.2, -0.1, 0.4], [1.0, -2.0, 0.5]) if start is None else start]
    for w, v in twists_:
        T.append(T[-1] @ R.se3_exp(w, v))
    return np.linspace(0.0, 0.1, len(T)).astype(np.float32).astype(np.float64), np.array(T)


SEGMENTS = {"pure translation": [([0.0, 0.0, 0.0], [1.2, 0.3, -0.1]), ([0.01, 0.02, -0.03], [0.5, 0.0, 0.0])],
            "1e-12 rad": [([6e-13, -8e-13, 0.0], [0.8, 0.1, 0.0]), ([0.0, 0.0, 0.02], [0.7, 0.0, 0.1])],
            "below the series threshold after scaling": [([4e-10, 0.0, 3e-10], [0.8, 0.1, 0.0])],
            "3.0 rad": [([0.0, 0.0, 0.02], [0.7, 0.0, 0.1]), ([1.8, 0.0, 2.4], [0.3, -0.2, 0.1])]}


@pytest.mark.parametrize("what", sorted(SEGMENTS))
def test_segment_kinds(vg, what):
    p, t = cloud()[:2049], times()[:2049]
    tau, T = _chain(SEGMENTS[what])
    w, _ = R.twists(T)
    print(what, "segment angles:", np.linalg.norm(w, axis=1))
    for t_ref in (None, tau[0]):
        check(vg.deskew(p, t, tau, T, t_ref), p, t, tau, T, t_ref, what=what)


def test_identity_motion_returns_the_input_bits(vg):
    from fast_gicp_amd import capi
    other = capi.VoxelGrid(0)
    for name in ("A", "lattice"):
        p, t = cloud(name), times(name)
        for K in (2, 64):
            tau, T = R.identity_trajectory(K)
            for t_ref in (None, 0.03, -5.0):
                assert same_bits(vg.deskew(p, t, tau, T, t_ref), p)
                ptr, m = vg.device_points()
                assert m == len(p)
                other.crop_range_device(ptr, m, 0.0, float("inf"))  # a bit copy of what the pointer holds
                assert same_bits(other.get_points(m), p)
    other.close()


# ---- non-finite points pass through as NaNs ----
def test_non_finite_rows_become_nans_and_the_crop_drops_exactly_them(vg):
    n = 300
    p, t = cloud()[:n].copy(), times()[:n].copy()
    tau, T = trajectory(3, 60)
    clean = vg.deskew(p, t, tau, T).copy()
    check(clean, p, t, tau, T, None)
    p[0, 1], p[63, 0], t[64], p[n - 1, 2], t[n - 1] = np.nan, np.inf, -np.inf, -np.inf, np.nan
    p[63, 2] = np.nan
    bad = np.zeros(n, bool)
    bad[[0, 63, 64, n - 1]] = True
    out = vg.deskew(p, t, tau, T)
    assert np.isnan(out[bad]).all() and same_bits(out[~bad], clean[~bad])
    check(out, p, t, tau, T, None)
    ptr, m = vg.device_points()
    assert m == n
    ptr2, m2 = vg.crop_range_device(ptr, m, 0.0, float("inf"))  # the handle's own output as its input
    assert m2 == n - 4 and np.array_equal(vg.kept_indices(), np.flatnonzero(~bad)) and same_bits(vg.get_points(m2), clean[~bad])
    for col, val in ((0, np.inf), (1, -np.inf), (2, np.nan)):  # every coordinate, every kind, one at a time
        q = cloud()[:n].copy()
        q[64, col] = val
        out = vg.deskew(q, times()[:n], tau, T)
        assert np.isnan(out[64]).all() and same_bits(np.delete(out, 64, 0), np.delete(clean, 64, 0))
    tt = times()[:n].copy()
    tt[63] = np.inf
    out = vg.deskew(cloud()[:n], tt, tau, T)
    assert np.isnan(out[63]).all() and same_bits(np.delete(out, 63, 0), np.delete(clean, 63, 0))


# ---- plumbing ----
def test_every_input_form_gives_the_same_bits(vg):
    import torch
    p, t = cloud()[:1031], times()[:1031]
    n = len(p)
    tau, T = trajectory(40, 70)
    t_ref = 0.04
    ref = vg.deskew(p, t, tau, T, t_ref).copy()
    check(ref, p, t, tau, T, t_ref)
    p4 = np.ascontiguousarray(np.hstack([p, t[:, None]]))
    assert same_bits(vg.deskew(p4, None, tau, T, t_ref, stride=4, time_stride=4), ref)        # xyzt rows, the time in the 4th float
    assert same_bits(vg.deskew(p4, t, tau, T, t_ref, stride=4, time_stride=1), ref)           # xyzt rows, the times given apart
    t2 = np.ascontiguousarray(np.stack([t, np.full(n, 9.0, np.float32)], 1)).reshape(-1)
    assert same_bits(vg.deskew(p, t2, tau, T, t_ref, time_stride=2), ref)                     # times two floats apart
    dev = torch.device("cuda", 0)
    d3, d4, dt = torch.from_numpy(p).to(dev).contiguous(), torch.from_numpy(p4).to(dev).contiguous(), torch.from_numpy(t).to(dev).contiguous()
    ptr, m = vg.deskew_device(d3.data_ptr(), n, dt.data_ptr(), tau, T, t_ref)
    assert m == n and ptr and same_bits(vg.get_points(m), ref)
    ptr, m = vg.deskew_device(d4.data_ptr(), n, d4.data_ptr() + 12, tau, T, t_ref, stride=4, time_stride=4)
    assert m == n and same_bits(vg.get_points(m), ref)
    # the input aliased to the handle's own output: load the cloud into it first (a crop that keeps everything is a bit copy)
    own, m = vg.crop_range_device(d3.data_ptr(), n, 0.0, float("inf"))
    assert m == n and same_bits(vg.get_points(m), p)
    ptr, m = vg.deskew_device(own, n, dt.data_ptr(), tau, T, t_ref)
    assert m == n and ptr == own and same_bits(vg.get_points(m), ref)
    # deskewing twice from the own output: the second pass sees the first one's output
    ptr, m = vg.deskew_device(ptr, n, dt.data_ptr(), tau, T, t_ref)
    assert same_bits(vg.get_points(m), vg.deskew(ref, t, tau, T, t_ref))
    # two consecutive runs: identical bytes
    assert same_bits(vg.deskew(p, t, tau, T, t_ref), ref)
    empty = vg.deskew(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), tau, T)
    assert empty.shape == (0, 3) and vg.device_points() == (0, 0)


def test_deskew_crop_filter_chain_on_one_handle_equals_fresh_handles():
    import torch
    from fast_gicp_amd import capi
    p, t = cloud().copy(), times()
    p[[5, 700, 4098], [0, 1, 2]] = np.nan, np.inf, np.nan
    n = len(p)
    tau, T = trajectory(40, 80)
    dev = torch.device("cuda", 0)
    d3, dt = torch.from_numpy(p).to(dev).contiguous(), torch.from_numpy(t).to(dev).contiguous()
    a = capi.VoxelGrid(0)
    ptr, m = a.deskew_device(d3.data_ptr(), n, dt.data_ptr(), tau, T)
    moved = a.get_points(m).copy()
    assert m == n and np.isnan(moved).any(axis=1).sum() == 3
    ptr, m1 = a.crop_range_device(ptr, m, 1e-3, 30.0 ** 2)
    cropped = a.get_points(m1).copy()
    ptr, m2 = a.filter_device(ptr, m1, 0.25)
    chained = a.get_points(m2).copy()
    assert 0 < m2 < m1 < n - 3 + 1
    b = capi.VoxelGrid(0)  # crop + filter on a fresh handle, from the downloaded deskew output
    dm = torch.from_numpy(moved).to(dev).contiguous()
    ptr_b, mb1 = b.crop_range_device(dm.data_ptr(), n, 1e-3, 30.0 ** 2)
    assert mb1 == m1 and same_bits(b.get_points(mb1), cropped)
    c = capi.VoxelGrid(0)
    dc = torch.from_numpy(cropped).to(dev).contiguous()
    ptr_c, mc = c.filter_device(dc.data_ptr(), m1, 0.25)
    assert mc == m2 and same_bits(c.get_points(mc), chained)
    # the deskew output taken by an NDT handle as its target, without a copy
    d3 = torch.from_numpy(cloud()).to(dev).contiguous()
    ptr, m = a.deskew_device(d3.data_ptr(), n, dt.data_ptr(), tau, T)
    want = a.get_points(m).copy()
    check(want, cloud(), t, tau, T, None)
    ndt = capi.NDTMapCore(0)
    ndt.set_target_cloud_from_voxelgrid(a)
    assert same_bits(ndt.get_target_points(), want)
    with pytest.raises(capi.FvhError):
        ndt.set_target_cloud_from_voxelgrid(a)  # an output can be taken once
    assert same_bits(a.get_points(m), want)  # the packed output is still there
    for h in (a, b, c, ndt):
        h.close()


def test_side_outputs_are_gone_after_a_deskew_and_the_profile_class_counts(vg):
    from fast_gicp_amd import capi
    p, t = cloud()[:500], times()[:500]
    tau, T = trajectory(3, 90)
    vg.crop_range(p, 1e-3, 400.0)
    assert len(vg.kept_indices()) > 0
    vg.deskew(p, t, tau, T)
    for getter in (vg.kept_indices, vg.scores):
        with pytest.raises(capi.FvhError, match="code 2"):  # FVH_ERR_BAD_STATE
            getter()
    vg.crop_range(p, 1e-3, 400.0)
    assert len(vg.kept_indices()) > 0 and len(vg.scores()[0]) == len(p)
    vg.profile_enable(True); vg.profile_reset()
    for _ in range(3):
        vg.deskew(p, t, tau, T)
    got = {c: vg.profile_get(c) for c in ("deskew", "compact", "downsample")}
    vg.profile_enable(False); vg.profile_reset()
    assert got["deskew"][1] == 3 and got["deskew"][0] > 0 and got["compact"] == (0.0, 0) and got["downsample"] == (0.0, 0), got


def test_refusals_leave_no_output_and_say_why(vg):
    from fast_gicp_amd import capi
    p, t = cloud()[:100], times()[:100]
    tau, T = trajectory(3, 100)
    lib = capi.load()

    def knots(K):
        return np.linspace(0.0, 0.1, K), np.tile(np.eye(4), (K, 1, 1))

    def with_pose(j, M):
        Tb = T.copy()
        Tb[j] = M
        return Tb

    scaled, sheared, row, nan_pose, mirror = (T[1].copy() for _ in range(5))
    scaled[:3, :3] *= 1.001
    sheared[0, 1] += 1e-3
    row[3, 0] = 1e-3
    nan_pose[1, 3] = np.nan
    mirror[:3, 0] *= -1.0
    half_turn = T[0] @ R.se3_exp([0.0, 0.0, np.pi], [0.1, 0.0, 0.0])
    almost = T[0] @ R.se3_exp([0.0, 0.0, np.pi - 1e-7], [0.1, 0.0, 0.0])
    p5 = np.zeros((20, 5), np.float32)
    errors = {"K = 1": lambda: vg.deskew(p, t, *knots(1)), "K = 65": lambda: vg.deskew(p, t, *knots(65)), "K = 0": lambda: vg.deskew(p, t, np.zeros(0), np.zeros((0, 4, 4)), 0.0),
              "NaN knot time": lambda: vg.deskew(p, t, [0.0, np.nan, 0.1], T), "infinite knot time": lambda: vg.deskew(p, t, [0.0, 0.05, np.inf], T),
              "equal knot times": lambda: vg.deskew(p, t, [0.0, 0.05, 0.05], T), "descending knot times": lambda: vg.deskew(p, t, tau[::-1].copy(), T),
              "scaled pose": lambda: vg.deskew(p, t, tau, with_pose(1, scaled)), "sheared pose": lambda: vg.deskew(p, t, tau, with_pose(1, sheared)),
              "last row": lambda: vg.deskew(p, t, tau, with_pose(1, row)), "NaN pose": lambda: vg.deskew(p, t, tau, with_pose(1, nan_pose)),
              "mirrored pose": lambda: vg.deskew(p, t, tau, with_pose(1, mirror)),
              "half turn": lambda: vg.deskew(p, t, tau, with_pose(1, half_turn)), "pi - 1e-7": lambda: vg.deskew(p, t, tau, with_pose(1, almost)),
              "NaN t_ref": lambda: vg.deskew(p, t, tau, T, np.nan), "infinite t_ref": lambda: vg.deskew(p, t, tau, T, -np.inf),
              "stride 5": lambda: vg.deskew(p5, np.zeros(20, np.float32), tau, T, stride=5), "time_stride 0": lambda: vg.deskew(p, t, tau, T, time_stride=0),
              "time_stride -1": lambda: vg.deskew(p, t, tau, T, time_stride=-1)}
    for what, call in errors.items():
        vg.deskew(p, t, tau, T)  # an output to lose
        assert vg.device_points()[1] == len(p)
        with pytest.raises(capi.FvhError, match="code 1"):  # FVH_ERR_INVALID_ARGUMENT
            call()
        assert vg.device_points() == (0, 0), what
        assert len(lib.fvh_voxelgrid_last_error(vg._h) or b"") > 0, what
        with pytest.raises(capi.FvhError, match="code 2"):
            vg.kept_indices()
    # null pointers, through the ABI itself
    a, tt = np.ascontiguousarray(p), np.ascontiguousarray(t)
    kt, kp = np.ascontiguousarray(tau), np.ascontiguousarray(T.transpose(0, 2, 1))
    P = capi._p
    n = C.c_int(5)
    nulls = {"xyz": (None, P(tt), P(kt), P(kp)), "times": (P(a), None, P(kt), P(kp)), "knot times": (P(a), P(tt), None, P(kp)), "knot poses": (P(a), P(tt), P(kt), None)}
    for what, (xa, ta, kta, kpa) in nulls.items():
        n.value = 5
        assert lib.fvh_voxelgrid_deskew(vg._h, xa, len(a), ta, 1, kta, kpa, 3, 0.1, C.byref(n)) == 1 and n.value == 0, what
        assert len(lib.fvh_voxelgrid_last_error(vg._h)) > 0
        n.value = 5
        assert lib.fvh_voxelgrid_deskew_device(vg._h, xa, len(a), 3, ta, 1, kta, kpa, 3, 0.1, C.byref(n)) == 1 and n.value == 0, what
    assert lib.fvh_voxelgrid_deskew(vg._h, P(a), len(a), P(tt), 1, P(kt), P(kp), 3, 0.1, None) == 1  # null out_n
    assert lib.fvh_voxelgrid_deskew(vg._h, P(a), -1, P(tt), 1, P(kt), P(kp), 3, 0.1, C.byref(n)) == 1 and n.value == 0
    # n == 0 is an empty result, not an error -- but its knots are still checked
    n.value = 5
    assert lib.fvh_voxelgrid_deskew(vg._h, None, 0, None, 1, P(kt), P(kp), 3, 0.1, C.byref(n)) == 0 and n.value == 0
    assert lib.fvh_voxelgrid_deskew(vg._h, None, 0, None, 1, P(kt), P(kp), 1, 0.1, C.byref(n)) == 1
    # just inside the angle limit, and the handle still works
    inside = T[0] @ R.se3_exp([0.0, 0.0, np.pi - 1e-5], [0.1, 0.0, 0.0])
    Tb = np.array([T[0], inside])
    check(vg.deskew(p, t, tau[:2], Tb), p, t, tau[:2], Tb, None, what="pi - 1e-5")
    check(vg.deskew(p, t, tau, T), p, t, tau, T, None)


# ---- end to end ----
def test_a_sweep_bent_by_the_twin_is_straightened_on_the_device(vg):
    p, t = cloud(), times()
    tau, T = trajectory(40, 110)
    for t_ref in (None, tau[0]):
        bent = R.skew(p, t, tau, T, t_ref).astype(np.float32)
        assert 0.3 < np.abs(bent - p).max() < 10.0
        out = vg.deskew(bent, t, tau, T, t_ref)
        M = R.scale(p, T)
        err = np.abs(out.astype(np.float64) - p)
        print("t_ref=%s: bent by up to %.2f m, recovered to %.2e = %.2f spacing(float32(M)), M = %.1f" % (t_ref, np.abs(bent - p).max(), err.max(), err.max() / np.spacing(np.float32(M)), M))
        # the skew's cast carried through a rotation (<= sqrt(3) / 2 ulp) plus the output cast (1 / 2 ulp)
        assert err.max() <= 2.0 * np.spacing(np.float32(M))


def test_pygicp_binding_equals_the_capi_route(vg):
    import torch  # noqa: F401  (its HIP runtime first, see tests/conftest.py)
    import pygicp
    p, t = cloud()[:1000], times()[:1000]
    tau, T = trajectory(40, 120)
    got = pygicp.deskew_device(p, t, tau, T)
    assert got.dtype == np.float64 and got.shape == (1000, 3) and same_bits(got.astype(np.float32), vg.deskew(p, t, tau, T))
    got = pygicp.deskew_device(p, t, tau, T, t_ref=0.02)
    assert same_bits(got.astype(np.float32), vg.deskew(p, t, tau, T, 0.02))
    with pytest.raises(Exception):
        pygicp.deskew_device(p, t[:10], tau, T)
    with pytest.raises(Exception):
        pygicp.deskew_device(p, t, tau[::-1].copy(), T)
