#!/usr/bin/env python
"""Times the device RANSAC plane segmentation (fvh_voxelgrid_segment_plane) on an MI355X and writes profiles/plane_timing.json.
   python tools/plane_timing.py [--reps 10] [--out profiles/plane_timing.json]

Legs: the bundled 17k source, a simulated LiDAR frame after ApproximateVoxelGrid 0.25, a 100k synthetic scene; distance threshold 0.1,
256 hypotheses, seed 7, no axis, FVH_PLANE_KEEP_OUTLIERS (ground removal). Per leg, medians over the repetitions:
  - wall time of the call (device pointer in, coefficients and counts out), plain and with FVH_PLANE_REFINE;
  - device time per profile class: plane (hypotheses, sweep, winner, refit), compact (flags, scan, compaction);
  - wall time of the host route it replaces: get_points, the same 256 hypotheses scored with vectorised numpy on one core (the
    division-free test of the contract, in chunks of 32 hypotheses), upload of the kept points;
  - the GATE: the device call is faster than that host route, with the same winner and the same counts;
  - reported, not gated: the "plane" class against one outlier_radius_count_kernel sweep of the same cloud (min_neighbors = 2^30: no
    early exit, radius 0.5) -- a dense N x H sweep against a culled N x neighbours one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, H, SEED = 0.1, 256, 7


def med(v):
    return float(np.median(v))


def mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7FEB352D); x ^= x >> np.uint32(15); x *= np.uint32(0x846CA68B); x ^= x >> np.uint32(16)
    return x


def host_scores(p, t, nh, seed):
    """(counts int32[H], winner, inlier mask): the contract of include/fast_vgicp_hip.h in vectorised numpy"""
    n = len(p)
    with np.errstate(over="ignore"):
        s0 = mix32(np.array([seed & 0xFFFFFFFF], np.uint32) ^ mix32(np.array([(seed >> 32) ^ 0x9E3779B9], np.uint32)))
        k = np.arange(1, 3 * nh + 1, dtype=np.uint32)
        idx = ((mix32(s0 + np.uint32(0x9E3779B9) * k).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64).reshape(nh, 3)
    p64 = p.astype(np.float64)
    q = p64[idx[:, 0]]
    e1, e2 = p64[idx[:, 1]] - q, p64[idx[:, 2]] - q
    a = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    b = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    c = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    nn = (a * a + b * b) + c * c
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & (nn != 0.0)
    counts = np.full(nh, -1, np.int32)
    t2 = t * t
    x, y, z = p64[:, 0][None, :], p64[:, 1][None, :], p64[:, 2][None, :]
    for lo in range(0, nh, 32):
        hs = lo + np.flatnonzero(valid[lo:lo + 32])
        s = (a[hs, None] * (x - q[hs, 0, None]) + b[hs, None] * (y - q[hs, 1, None])) + c[hs, None] * (z - q[hs, 2, None])
        counts[hs] = (s * s <= (t2 * nn[hs])[:, None]).sum(axis=1)
    w = int(np.argmax(counts))
    s = (a[w] * (p64[:, 0] - q[w, 0]) + b[w] * (p64[:, 1] - q[w, 1])) + c[w] * (p64[:, 2] - q[w, 2])
    return counts, w, s * s <= t2 * nn[w]


def host_route(vg, m, reps):
    """what a caller does today: the cloud back to the host, the hypotheses scored there, upload of the remainder"""
    import torch
    total, parts = [], {"get_points_ms": [], "score_ms": [], "upload_ms": []}
    for _ in range(reps):
        t0 = time.perf_counter()
        p = vg.get_points(m)
        t1 = time.perf_counter()
        counts, w, inl = host_scores(p, T, H, SEED)
        kept = np.ascontiguousarray(p[~inl])
        t2 = time.perf_counter()
        torch.from_numpy(kept).to(torch.device("cuda", 0)); torch.cuda.synchronize()
        t3 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[k].append(v * 1e3)
        total.append((t3 - t0) * 1e3)
    out = {k: med(v) for k, v in parts.items()}
    out.update(host_method="numpy, one core, 32 hypotheses per chunk", total_ms=med(total), winner=w, count_winner=int(counts[w]), kept=int(len(kept)))
    return out, counts


def leg(name, pts, reps):
    import torch
    from fast_gicp_amd import capi
    torch.set_num_threads(1)
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    d = torch.from_numpy(pts).to(torch.device("cuda", 0)).contiguous()
    vg = capi.VoxelGrid(0)
    lib = vg._lib
    co, ni, m = np.zeros(4), C.c_int(0), C.c_int(0)

    def call(flags):
        rc = lib.fvh_voxelgrid_segment_plane_device(vg._h, C.c_void_p(d.data_ptr()), n, 3, T, H, SEED, None, 0.0, flags, capi._p(co), C.byref(ni), C.byref(m))
        assert rc == 0, rc

    res = {"leg": name, "points": n, "distance_threshold": T, "max_iterations": H, "seed": SEED}
    for label, flags in (("plain", capi.PLANE_KEEP_OUTLIERS), ("refine", capi.PLANE_KEEP_OUTLIERS | capi.PLANE_REFINE)):
        for _ in range(3):
            call(flags)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call(flags)
            wall.append((time.perf_counter() - t0) * 1e6)
        per = {"plane": [], "compact": []}
        vg.profile_enable(True)
        for _ in range(reps):
            vg.profile_reset()
            call(flags)
            for c in per:
                per[c].append(vg.profile_get(c)[0] * 1e3)
        vg.profile_enable(False); vg.profile_reset()
        res[label] = {"wall_us": med(wall), "device_us": {c: med(v) for c, v in per.items()}, "num_inliers": ni.value, "kept": m.value, "coefficients": [float(v) for v in co]}
    vg.segment_plane((d.data_ptr(), n), T, H, SEED, keep_outliers=True, device=True)  # through the wrapper: plane_model() sizes its counts array by this call's H
    model = vg.plane_model()
    # one culled radius sweep of the same cloud, without its early exit
    sweep = []
    vg.profile_enable(True)
    for _ in range(3):
        vg.remove_radius_outliers_device(d.data_ptr(), n, 0.5, 2 ** 30)
    for _ in range(reps):
        vg.profile_reset()
        vg.remove_radius_outliers_device(d.data_ptr(), n, 0.5, 2 ** 30)
        sweep.append(vg.profile_get("outlier_count")[0] * 1e3)
    vg.profile_enable(False); vg.profile_reset()
    res["radius_count_sweep_us"] = med(sweep)
    res["plane_over_radius_sweep"] = res["plain"]["device_us"]["plane"] / res["radius_count_sweep_us"]
    _, mm = vg.crop_range_device(d.data_ptr(), n, 0.0, float("inf"))  # the whole cloud as the handle's output: what the host route starts from
    hr, counts = host_route(vg, mm, max(3, reps // 3))
    vg.close()
    res["host_route"] = hr
    same = bool(np.array_equal(counts, model["counts"]) and hr["winner"] == model["winner"] and hr["kept"] == res["plain"]["kept"])
    res["winner"], res["count_winner"], res["valid"] = model["winner"], model["count_winner"], model["valid"]
    res["gate"] = {"device_call_ms": res["plain"]["wall_us"] * 1e-3, "host_route_ms": hr["total_ms"], "speedup": hr["total_ms"] / (res["plain"]["wall_us"] * 1e-3),
                   "same_result": same, "passed": bool(res["plain"]["wall_us"] * 1e-3 < hr["total_ms"] and same)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first: INTEGRATION.md, "Sharing a process with PyTorch")
    from fast_gicp_amd import capi, preprocess, workloads
    assert capi.device_count() >= 1, "no GPU visible"
    vg = capi.VoxelGrid(0)
    frame = vg.filter(workloads.lidar_frame(3), 0.25)
    vg.close()
    legs = [("bundled_source_17k", preprocess.bundled_pair(os.path.join(ROOT, "data"))[1]), ("lidar_frame_avg025", frame), ("synthetic_100k", workloads.synthetic_scene(100000, 42))]
    out = {"device": capi.device_name(0) if hasattr(capi, "device_name") else "gfx950", "reps": a.reps, "legs": [leg(nm, p, a.reps) for nm, p in legs]}
    out["gate_passed"] = all(l["gate"]["passed"] is True for l in out["legs"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for l in out["legs"]:
        print("%-20s n=%6d winner %3d count %6d | call %7.1f us wall (plane %.1f compact %.1f), refine %7.1f us (plane %.1f) | plane / radius sweep %.1f / %.1f = %.2f | host route %.1f ms: same %s gate %s" % (
            l["leg"], l["points"], l["winner"], l["count_winner"], l["plain"]["wall_us"], l["plain"]["device_us"]["plane"], l["plain"]["device_us"]["compact"], l["refine"]["wall_us"],
            l["refine"]["device_us"]["plane"], l["plain"]["device_us"]["plane"], l["radius_count_sweep_us"], l["plane_over_radius_sweep"], l["host_route"]["total_ms"],
            l["gate"]["same_result"], l["gate"]["passed"]))
    print(json.dumps({"gate_passed": out["gate_passed"], "out": a.out}))
    return 0 if out["gate_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
