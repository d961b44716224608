#!/usr/bin/env python
"""Times the device crop / outlier filters (fvh_voxelgrid_crop_range, _remove_radius_outliers, _remove_statistical_outliers) on an
MI355X and writes profiles/outlier_timing.json.   python tools/outlier_timing.py [--reps 20] [--out profiles/outlier_timing.json]

Legs: the bundled 17k source, a simulated LiDAR frame after ApproximateVoxelGrid 0.25, a 100k synthetic scene. Per leg:
  - device time per profile class (sort, knn, outlier_count, outlier_score, compact) of the radius filter (r = 0.5, min = 2) and the
    statistical filter (k = 20, mul = 1.0), medians over the repetitions;
  - wall time of the call (device pointer in, count out);
  - wall time of the host route it replaces: get_points, scipy's cKDTree (when scipy is importable; otherwise the brute-force numpy twin of
    the tests, on clouds of at most 5,000 points only), upload;
  - the gate: outlier_radius_count_kernel against the RBF covariance sweep with kernel_max_dist = radius ("rbf" class of a VGICP handle) on
    the same cloud in the same process. The count kernel visits the same tiles, does less per candidate and may stop early: it must not
    take longer;
  - statistical: the whole chain over its own sort + knn share (reported, not gated);
  - crop: time against the bytes it moves (16 B read + 4 B flag + 4 B score written per point, then the scan and 28 B per kept point)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return float(np.median(v))


def host_route(vg, m, radius, min_nb, mean_k, mul):
    """what a caller does today: filtered cloud back to the host, neighbour queries there, upload of the result (timed without the upload's consumer)"""
    out = {}
    try:
        from scipy.spatial import cKDTree
    except Exception:
        cKDTree = None
    t0 = time.perf_counter()
    p = vg.get_points(m)
    out["get_points_ms"] = (time.perf_counter() - t0) * 1e3
    if cKDTree is not None:
        t0 = time.perf_counter()
        tree = cKDTree(p)
        cnt = tree.query_ball_point(p, radius, return_length=True) - 1
        keep = cnt >= min_nb
        out["radius_host_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        d, _ = tree.query(p, mean_k + 1)
        md = d[:, 1:].mean(axis=1)
        keep2 = md <= md.mean() + mul * md.std(ddof=1)
        out["statistical_host_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_method"] = "scipy.cKDTree"
        out["host_kept"] = [int(keep.sum()), int(keep2.sum())]
    elif m <= 5000:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import outlier_ref as R
        t0 = time.perf_counter()
        R.radius(p, radius, min_nb)
        out["radius_host_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        R.statistical(p, mean_k, mul)
        out["statistical_host_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_method"] = "numpy brute force"
    else:
        out["host_method"] = None  # no scipy, and the brute-force twin is O(n^2): not timed at this size
    return out


def leg(name, pts, reps, radius=0.5, min_nb=2, mean_k=20, mul=1.0):
    import torch
    from fast_gicp_amd import capi
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    d = torch.from_numpy(pts).to(torch.device("cuda", 0)).contiguous()
    vg = capi.VoxelGrid(0)
    res = {"leg": name, "points": n}
    calls = {"radius": lambda: vg.remove_radius_outliers_device(d.data_ptr(), n, radius, min_nb),
             "statistical": lambda: vg.remove_statistical_outliers_device(d.data_ptr(), n, mean_k, mul),
             "crop": lambda: vg.crop_range_device(d.data_ptr(), n, 1e-3, 60.0 ** 2)}
    classes = ("sort", "knn", "outlier_count", "outlier_score", "compact")
    for what, call in calls.items():
        for _ in range(3):
            _, m = call()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e6)
        per = {c: [] for c in classes}
        vg.profile_enable(True)
        for _ in range(reps):
            vg.profile_reset()
            call()
            for c in classes:
                ms, k = vg.profile_get(c)
                if k:
                    per[c].append(ms * 1e3)
        vg.profile_enable(False); vg.profile_reset()
        res[what] = {"kept": m, "wall_us": med(wall), "device_us": {c: med(v) for c, v in per.items() if v}}
    st = res["statistical"]["device_us"]
    res["statistical"]["chain_over_sort_knn"] = sum(st.values()) / (st["sort"] + st["knn"])
    cr = res["crop"]
    moved = n * (16 + 4 + 4) + n * 8 + cr["kept"] * (16 + 12 + 16 + 4)  # flags + score pass, scan in/out, compaction (read point, write xyz, float4, index)
    cr["bytes_moved"] = moved
    cr["gb_per_s"] = moved / (cr["device_us"]["compact"] * 1e-6) / 1e9
    # the gate: the RBF sweep at kernel_max_dist = radius, same cloud, same process
    c = capi.VGICPCore(0)
    c.set_kernel_params(0.25, radius)
    c.set_source_cloud_device(d.data_ptr(), n, 3)
    for _ in range(3):
        c.calculate_source_covariances_rbf()
    rbf = []
    c.profile_enable(True)
    for _ in range(reps):
        c.profile_reset()
        c.calculate_source_covariances_rbf()
        rbf.append(c.profile_get("rbf")[0] * 1e3)
    c.profile_enable(False)
    c.close()
    count_us = res["radius"]["device_us"]["outlier_count"]
    res["gate"] = {"outlier_count_us": count_us, "rbf_sweep_us": med(rbf), "ratio": count_us / med(rbf), "passed": bool(count_us <= med(rbf))}
    _, m = vg.crop_range_device(d.data_ptr(), n, 0.0, float("inf"))  # the whole cloud as the handle's output: what the host route starts from
    res["host_route"] = host_route(vg, m, radius, min_nb, mean_k, mul)
    t0 = time.perf_counter()
    torch.from_numpy(pts).to(torch.device("cuda", 0)); torch.cuda.synchronize()
    res["host_route"]["upload_ms"] = (time.perf_counter() - t0) * 1e3
    vg.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first: INTEGRATION.md, "Sharing a process with PyTorch")
    from fast_gicp_amd import capi, preprocess, workloads
    assert capi.device_count() >= 1, "no GPU visible"
    vg = capi.VoxelGrid(0)
    frame = vg.filter(workloads.lidar_frame(3), 0.25)
    vg.close()
    legs = [("bundled_source_17k", preprocess.bundled_pair(os.path.join(ROOT, "data"))[1]), ("lidar_frame_avg025", frame), ("synthetic_100k", workloads.synthetic_scene(100000, 42))]
    out = {"device": capi.device_name(0) if hasattr(capi, "device_name") else "gfx950", "reps": a.reps, "legs": [leg(nm, p, a.reps) for nm, p in legs]}
    out["gate_passed"] = all(l["gate"]["passed"] for l in out["legs"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for l in out["legs"]:
        print("%-20s n=%6d radius %7.1f us wall (%s) | statistical %7.1f us wall (%s) x%.2f of sort+knn | crop %6.1f us wall, %.0f GB/s | gate count %.1f <= rbf %.1f: %s" % (
            l["leg"], l["points"], l["radius"]["wall_us"], " ".join("%s %.1f" % kv for kv in l["radius"]["device_us"].items()), l["statistical"]["wall_us"],
            " ".join("%s %.1f" % kv for kv in l["statistical"]["device_us"].items()), l["statistical"]["chain_over_sort_knn"], l["crop"]["wall_us"], l["crop"]["gb_per_s"],
            l["gate"]["outlier_count_us"], l["gate"]["rbf_sweep_us"], l["gate"]["passed"]))
    print(json.dumps({"gate_passed": out["gate_passed"], "out": a.out}))
    return 0 if out["gate_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
