"""The cooperative small sort's histogram exchange (kernels_sort.hpp, sort_coop_kernel; sort_granule.hpp): its 32 workgroups hand each other
their digit counts as 8-byte granules of four 11-bit counts under one launch-and-pass tag, and every wave derives its own scatter cursors
from them. The order it produces is a pure permutation, so it is compared exactly: against the one-workgroup fallback (no exchange at all)
at every size where the chunking changes and on clouds that put a workgroup's whole 1,024 keys into one bin -- the largest count a slot has
to carry -- and against numpy's stable sort over many launches of one handle with shrinking and growing clouds (a granule left over from an
earlier, larger launch must never pass for a current one)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 511, 513, 1000, 4097, 17334, 32767, 32768]


def _spread(v, bits):
    out = np.zeros_like(v)
    for b in range(bits):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def _keys18(pts):
    """kernels_sort.hpp: the small sorts' 18-bit Morton key, 6 bits per axis on the cloud's bounding cube"""
    lo = pts.min(0)
    extent = np.float32(max((pts.max(0) - lo).max(), np.float32(1e-6)))
    qmax = np.float32(63)
    scale = np.float32((qmax + np.float32(0.999)) / extent)
    q = np.minimum(qmax, np.maximum(np.float32(0), (pts - lo) * scale)).astype(np.int64)
    return _spread(q[:, 0], 6) | (_spread(q[:, 1], 6) << 1) | (_spread(q[:, 2], 6) << 2)


def _tied_cloud(n):
    rng = np.random.default_rng(n)
    pts = (rng.normal(size=(n, 3)) * np.array([20.0, 20.0, 2.0])).astype(np.float32)
    pts[: n // 8] = np.round(pts[: n // 8])  # many equal keys and equal points
    return pts


def _one_bin_cloud(n):
    return np.full((n, 3), 1.5, np.float32)  # every key equal: one bin holds everything, 1,024 per workgroup at n = 32,768


@pytest.mark.parametrize("make", [_tied_cloud, _one_bin_cloud], ids=["ties", "one_bin"])
@pytest.mark.parametrize("n", SIZES)
def test_cooperative_route_equals_the_one_workgroup_fallback(n, make, monkeypatch):
    from fast_gicp_amd import capi
    pts = make(n)
    monkeypatch.delenv("FVH_SORT_COOP_WATCHDOG_TICKS", raising=False)
    c = capi.VGICPCore(0)
    c.synchronize()
    r0 = np.array(capi.debug_sort_routes())
    c.set_source_cloud(pts)
    order, boxes = c.debug_spatial_order("source")
    order, boxes = order.copy(), boxes.copy()
    c.synchronize()
    assert tuple(np.array(capi.debug_sort_routes()) - r0) == (1, 0, 0, 0), "the first run did not take the cooperative route"
    c.close()
    monkeypatch.setenv("FVH_SORT_COOP_WATCHDOG_TICKS", "0")  # route choice: the cooperative kernel steps aside at once, one workgroup sorts
    f = capi.VGICPCore(0)
    f.set_source_cloud(pts)
    order_fb, boxes_fb = f.debug_spatial_order("source")
    f.synchronize()
    monkeypatch.delenv("FVH_SORT_COOP_WATCHDOG_TICKS")
    f.close()
    assert np.array_equal(np.sort(order_fb), np.arange(n))
    assert np.array_equal(order, order_fb)
    assert np.array_equal(boxes, boxes_fb)


def test_forty_launches_of_alternating_size_on_one_handle_match_numpy(monkeypatch):
    from fast_gicp_amd import capi
    monkeypatch.delenv("FVH_SORT_COOP_WATCHDOG_TICKS", raising=False)
    sizes = [17334, 1000, 32768, 63]
    clouds = [_tied_cloud(n) for n in sizes]
    want = [np.argsort(_keys18(p), kind="stable") for p in clouds]
    c = capi.VGICPCore(0)
    c.synchronize()
    r0 = np.array(capi.debug_sort_routes())
    for it in range(40):
        j = it % len(sizes)
        c.set_source_cloud(clouds[j])
        order, _ = c.debug_spatial_order("source")
        assert np.array_equal(order, want[j]), "launch %d (n = %d): %d positions differ" % (it, sizes[j], int((order != want[j]).sum()))
    assert tuple(np.array(capi.debug_sort_routes()) - r0) == (40, 0, 0, 0)
    c.close()
