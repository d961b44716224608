#!/usr/bin/env python
"""Times the device Euclidean cluster extraction (fvh_voxelgrid_cluster_euclidean) on an MI355X and writes profiles/cluster_timing.json.
   python tools/cluster_timing.py [--reps 10] [--out profiles/cluster_timing.json]

Legs: the bundled 17k source, a simulated LiDAR frame after ApproximateVoxelGrid 0.25, a 100k synthetic scene; tolerance 0.5, min 10.
Per leg, medians over the repetitions:
  - wall time of the call (device pointer in, counts out);
  - device time per profile class: sort, cluster (the union-find sweep), compact (everything after it);
  - wall time of the host route it replaces, when scipy is importable: get_points, scipy.spatial.cKDTree.query_pairs,
    scipy.sparse.csgraph.connected_components and the size window, upload of the kept points;
  - the GATE: the device call is faster than that host route;
  - reported, not gated: the link kernel's time over outlier_radius_count_kernel run with min_neighbors = 2^30 (a full sweep, no early exit)
    at the same radius on the same cloud -- what the unions cost on top of the traversal (the link kernel visits the tiles up to the
    query's own only, the count kernel all of them)."""
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


def host_route(vg, m, tolerance, min_size, reps):
    """what a caller does today: the cloud back to the host, a kd-tree and a graph search there, upload of the kept points"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except Exception:
        return {"host_method": None}
    import torch
    total, parts = [], {"get_points_ms": [], "query_pairs_ms": [], "components_ms": [], "upload_ms": []}
    for _ in range(reps):
        t0 = time.perf_counter()
        p = vg.get_points(m)
        t1 = time.perf_counter()
        pairs = cKDTree(p).query_pairs(tolerance, output_type="ndarray")
        t2 = time.perf_counter()
        g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(m, m))
        ncomp, comp = connected_components(g, directed=False)
        keep = np.bincount(comp, minlength=ncomp)[comp] >= min_size
        kept = np.ascontiguousarray(p[keep])
        t3 = time.perf_counter()
        torch.from_numpy(kept).to(torch.device("cuda", 0)); torch.cuda.synchronize()
        t4 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[k].append(v * 1e3)
        total.append((t4 - t0) * 1e3)
    out = {k: med(v) for k, v in parts.items()}
    out.update(host_method="scipy.cKDTree.query_pairs + csgraph.connected_components", total_ms=med(total), pairs=int(len(pairs)), kept=int(keep.sum()),
               clusters=int((np.bincount(comp, minlength=ncomp) >= min_size).sum()))
    return out


def leg(name, pts, reps, tolerance=0.5, min_size=10):
    import torch
    from fast_gicp_amd import capi
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    d = torch.from_numpy(pts).to(torch.device("cuda", 0)).contiguous()
    vg = capi.VoxelGrid(0)
    lib = vg._lib
    import ctypes as C
    nc, m = C.c_int(0), C.c_int(0)

    def call():
        rc = lib.fvh_voxelgrid_cluster_euclidean_device(vg._h, C.c_void_p(d.data_ptr()), n, 3, float(tolerance), int(min_size), 0, C.byref(nc), C.byref(m))
        assert rc == 0, rc

    for _ in range(3):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    classes = ("sort", "cluster", "compact")
    per = {c: [] for c in classes}
    vg.profile_enable(True)
    for _ in range(reps):
        vg.profile_reset()
        call()
        for c in classes:
            per[c].append(vg.profile_get(c)[0] * 1e3)
    # the traversal alone: the radius filter's count kernel with a neighbour count it can never reach
    sweep = []
    for _ in range(3):
        vg.remove_radius_outliers_device(d.data_ptr(), n, tolerance, 2 ** 30)
    for _ in range(reps):
        vg.profile_reset()
        vg.remove_radius_outliers_device(d.data_ptr(), n, tolerance, 2 ** 30)
        sweep.append(vg.profile_get("outlier_count")[0] * 1e3)
    vg.profile_enable(False); vg.profile_reset()
    res = {"leg": name, "points": n, "tolerance": tolerance, "min_cluster_size": min_size, "clusters": nc.value, "kept": m.value, "wall_us": med(wall),
           "device_us": {c: med(v) for c, v in per.items()}, "full_sweep_us": med(sweep)}
    res["link_over_full_sweep"] = res["device_us"]["cluster"] / res["full_sweep_us"]
    _, mm = vg.crop_range_device(d.data_ptr(), n, 0.0, float("inf"))  # the whole cloud as the handle's output: what the host route starts from
    res["host_route"] = host_route(vg, mm, tolerance, min_size, max(3, reps // 3))
    vg.close()
    hr = res["host_route"]
    if hr["host_method"] is None:
        res["gate"] = {"passed": None, "reason": "scipy is not importable: the host route was not timed"}
    else:
        res["gate"] = {"device_call_ms": res["wall_us"] * 1e-3, "host_route_ms": hr["total_ms"], "speedup": hr["total_ms"] / (res["wall_us"] * 1e-3),
                       "passed": bool(res["wall_us"] * 1e-3 < hr["total_ms"]), "same_result": bool(hr["kept"] == m.value and hr["clusters"] == nc.value)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_timing.json"))
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
        print("%-20s n=%6d clusters %5d kept %6d | call %7.1f us wall (%s) | link / full sweep %.1f / %.1f = %.2f | host route %s ms: gate %s" % (
            l["leg"], l["points"], l["clusters"], l["kept"], l["wall_us"], " ".join("%s %.1f" % kv for kv in l["device_us"].items()), l["device_us"]["cluster"], l["full_sweep_us"],
            l["link_over_full_sweep"], ("%.1f" % l["host_route"]["total_ms"]) if l["host_route"]["host_method"] else "n/a", l["gate"]["passed"]))
    print(json.dumps({"gate_passed": out["gate_passed"], "out": a.out}))
    return 0 if out["gate_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
