#!/usr/bin/env python
"""What an insert into the incremental NDT target map costs, beside the VGICP additive map on the same box in the same process.

The bundled 17k-point scan is inserted into (a) an empty map, (b) the map of the 100k-point synthetic scene, (c) the map of the 1M-point
scene of bench.py's synth1m (resolution 0.5), as tools/map_insert_timing.py does it -- once into an NDT handle's map (voxel sums of points:
vm_insert_kernel<1> + vm_refresh_kernel<1>, the refresh carrying one MIN_EIG eigen-decomposition per touched voxel) and once into a VGICP
handle's additive map (vm_insert_kernel<0> + vm_refresh_kernel<0>: points + covariances, no decomposition). Then a full rehash of each map
(a prune that removes nothing moves every bucket and recomputes every record: vm_rehash_kernel<1> against <0>).

Device times are HIP events on the handle's stream (the engine's profiler: classes map_insert = both kernels of an insert, map_rehash = the
clears of the other side + the kernel); `wall` is the host clock around the device-synchronised call. After a warm-up, medians of --repeats
runs. Every repeat inserts the scan at another height (50 m apart), so every insert CREATES its voxels. The two handles alternate repeat by
repeat, so a drift of the box hits both. The ratios NDT / VGICP are reported, not gated: the refresh and the rehash do strictly more work per
voxel on the NDT side, the insert kernel strictly less per point.

    python tools/ndt_map_timing.py OUT_DIR [--repeats 20] [--legs empty,100k,1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--legs", default="empty,100k,1m")
    args = ap.parse_args()
    import torch
    from fast_gicp_amd import capi, preprocess, workloads
    sync = torch.cuda.synchronize
    _, scan = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "scan_points": int(len(scan)), "legs": {}}
    for leg in args.legs.split(","):
        res = 0.5 if leg == "1m" else 1.0
        ndt, vg = capi.NDTMapCore(0), capi.VGICPCore(0)
        for c in (ndt, vg):
            c.set_resolution(res); c.set_neighbor_search_method(capi.DIRECT7)
        vg.set_source_cloud(scan); vg.find_source_neighbors(20); vg.calculate_source_covariances()
        scan_cov = vg.get_covariances("source").astype(np.float64)
        base = base_cov = None
        if leg != "empty":
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            base = workloads.synthetic_scene(n, seed, extent)
            vg.set_source_cloud(base); vg.find_source_neighbors(20); vg.calculate_source_covariances()
            base_cov = vg.get_covariances("source").copy()
        for c in (ndt, vg):
            c.profile_enable(True)
            c.map_begin()
        if base is not None:
            ndt.map_insert_cloud(base)
            vg.map_insert_cloud(base, base_cov)

        def insert_scan(c, i):
            T = np.eye(4); T[2, 3] = 50.0 * (i + 1)
            c.set_source_cloud(scan)
            if c is vg:
                c.set_source_covariances(scan_cov)
            c.synchronize(); c.profile_reset(); sync()
            t0 = time.perf_counter()
            c.map_insert_source(T)
            c.synchronize()
            wall = time.perf_counter() - t0
            return c.profile_get("map_insert")[0], 1e3 * wall

        def rehash(c):
            c.synchronize(); c.profile_reset()
            assert c.map_prune([0.0, 0.0, 0.0], 1e9, 0) == 0
            c.synchronize()
            return c.profile_get("map_rehash")[0]

        for i in range(3):  # warm-up
            for c in (ndt, vg):
                insert_scan(c, i)
        info = {"ndt": ndt.map_info(), "vgicp": vg.map_info()}
        t = {k: [] for k in ("ndt_dev", "ndt_wall", "vgicp_dev", "vgicp_wall", "ndt_rehash", "vgicp_rehash")}
        for i in range(args.repeats):
            for name, c in (("ndt", ndt), ("vgicp", vg)):
                d, w = insert_scan(c, 3 + i)
                t[name + "_dev"].append(d); t[name + "_wall"].append(w)
        for _ in range(args.repeats):
            for name, c in (("ndt", ndt), ("vgicp", vg)):
                t[name + "_rehash"].append(rehash(c))
        row = dict(map_points=0 if base is None else int(len(base)), resolution=res)
        for name, c in (("ndt", ndt), ("vgicp", vg)):
            end = c.map_info()
            row[name] = dict(num_voxels_before=info[name]["num_voxels"], capacity_before=info[name]["capacity"], num_voxels_at_rehash=end["num_voxels"], capacity_at_rehash=end["capacity"],
                             insert_refresh_device_ms=med(t[name + "_dev"]), insert_wall_ms=med(t[name + "_wall"]), rehash_device_ms=med(t[name + "_rehash"]), dropped=end["dropped"])
        row["insert_refresh_ndt_over_vgicp"] = row["ndt"]["insert_refresh_device_ms"] / row["vgicp"]["insert_refresh_device_ms"]
        row["rehash_ndt_over_vgicp"] = row["ndt"]["rehash_device_ms"] / row["vgicp"]["rehash_device_ms"]
        print("%-6s insert + refresh of %d points, map of %d voxels: NDT %.4f ms device (%.3f wall) | VGICP additive %.4f ms (%.3f wall) | ratio %.2f" % (
            leg, len(scan), row["ndt"]["num_voxels_before"], row["ndt"]["insert_refresh_device_ms"], row["ndt"]["insert_wall_ms"], row["vgicp"]["insert_refresh_device_ms"],
            row["vgicp"]["insert_wall_ms"], row["insert_refresh_ndt_over_vgicp"]), flush=True)
        print("       full rehash, %d voxels in %d buckets: NDT %.4f ms device | VGICP additive %.4f ms | ratio %.2f" % (
            row["ndt"]["num_voxels_at_rehash"], row["ndt"]["capacity_at_rehash"], row["ndt"]["rehash_device_ms"], row["vgicp"]["rehash_device_ms"], row["rehash_ndt_over_vgicp"]), flush=True)
        out["legs"][leg] = row
        ndt.close(); vg.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "ndt_map_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
