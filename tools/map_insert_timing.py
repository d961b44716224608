#!/usr/bin/env python
"""What an insert into the incremental target map costs, against the batch route to the same map.

The bundled 17k-point source (with its k-NN covariances) is inserted into (a) an empty map, (b) the map of the 100k-point synthetic
scene, (c) the map of the 1M-point scene of bench.py's synth1m (resolution 0.5) -- "cost follows the scan, not the map" is (c) ~ (a).
For (c) the batch route to the same map is timed too: set_target_cloud_device(concatenation) + set_target_covariances +
create_target_voxelmap (the k-NN of the concatenation is not even counted, in the batch route's favour), and a full rehash of the 1M map.

Device times are HIP events on the handle's stream (the engine's profiler: classes map_insert, map_rehash, voxelmap); `wall` is the host
clock around the device-synchronised calls. After a warm-up, medians of --repeats runs, one process. Every repeat inserts the scan at
another height (50 m apart), so every insert CREATES its voxels -- the dearer case; a table growth that this triggers is its own profiler
class (map_rehash) and shows in the wall time only. The device time brackets the two kernels of an insert (vm_insert, vm_refresh); the wall
time adds what the host does around them: the 4-byte clear of the dirty count and, when the host's bound says the table could pass load
0.5, a counter readback. Exits non-zero if the insert into the 1M-point map is not faster than the batch build kernels.

    python tools/map_insert_timing.py OUT_DIR [--repeats 20] [--legs empty,100k,1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def covariances(c, pts):
    c.set_source_cloud(pts); c.find_source_neighbors(20); c.calculate_source_covariances()
    return c.get_covariances("source").copy()


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
        c = capi.VGICPCore(0)
        c.set_resolution(res); c.set_neighbor_search_method(capi.DIRECT7)
        scan_cov = covariances(c, scan)
        base = base_cov = None
        if leg != "empty":
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            base = workloads.synthetic_scene(n, seed, extent)
            base_cov = covariances(c, base)
        c.profile_enable(True)

        def restart():
            c.map_begin()
            if base is not None:
                c.map_insert_cloud(base, base_cov)

        def insert_scan(i):
            T = np.eye(4); T[2, 3] = 50.0 * (i + 1)
            c.set_source_cloud(scan); c.set_source_covariances(scan_cov.astype(np.float64))
            c.synchronize(); c.profile_reset(); sync()
            t0 = time.perf_counter()
            c.map_insert_source(T)
            c.synchronize()
            wall = time.perf_counter() - t0
            return c.profile_get("map_insert")[0], 1e3 * wall

        restart()
        for i in range(3):  # warm-up
            insert_scan(i)
        info = c.map_info()
        dev, wall = [], []
        for i in range(args.repeats):
            d, w = insert_scan(3 + i)
            dev.append(d); wall.append(w)
        row = dict(map_points=0 if base is None else int(len(base)), resolution=res, num_voxels=info["num_voxels"], capacity=info["capacity"],
                   insert_device_ms=med(dev), insert_wall_ms=med(wall), dropped=c.map_info()["dropped"])
        print("%-6s insert of %d points into a map of %d voxels: %.3f ms device, %.3f ms wall" % (leg, len(scan), row["num_voxels"], row["insert_device_ms"], row["insert_wall_ms"]), flush=True)
        if leg == "1m":
            # the rehash at 1M points: a prune that removes nothing moves every bucket
            dev = []
            for _ in range(args.repeats):
                c.synchronize(); c.profile_reset()
                assert c.map_prune([0.0, 0.0, 0.0], 1e9, 0) == 0
                c.synchronize()
                dev.append(c.profile_get("map_rehash")[0])
            row["rehash_device_ms"] = med(dev)
            print("       rehash of that map: %.3f ms device" % row["rehash_device_ms"], flush=True)
            # the batch route to the map insert (c) leaves behind: the concatenation, uploaded from a device buffer + its covariances + a build
            b = capi.VGICPCore(0)
            b.set_resolution(res); b.set_neighbor_search_method(capi.DIRECT7); b.profile_enable(True)
            P = np.concatenate([base, scan]); Cov = np.concatenate([base_cov, scan_cov]).astype(np.float64)
            d_P = torch.from_numpy(P).cuda()
            dev, wall = [], []
            for i in range(3 + args.repeats):
                b.synchronize(); b.profile_reset(); sync()
                t0 = time.perf_counter()
                b.set_target_cloud_device(d_P.data_ptr(), len(P), 3); b.set_target_covariances(Cov); b.create_target_voxelmap()
                b.synchronize()
                w = time.perf_counter() - t0
                if i >= 3:
                    dev.append(b.profile_get("voxelmap")[0]); wall.append(1e3 * w)
            row["batch_build_kernels_device_ms"] = med(dev)
            row["batch_route_wall_ms"] = med(wall)
            row["insert_faster_than_batch_kernels_alone"] = row["insert_device_ms"] < row["batch_build_kernels_device_ms"]
            print("       batch route to the same map: %.3f ms device for the build kernels alone, %.3f ms wall with upload + covariances" % (row["batch_build_kernels_device_ms"], row["batch_route_wall_ms"]), flush=True)
            b.close()
        out["legs"][leg] = row
        c.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "map_insert_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    # the one gate: an insert into the 1M-point map is faster than the batch route to the same map (here: than its build kernels ALONE)
    gate = out["legs"].get("1m")
    if gate is not None and not gate["insert_faster_than_batch_kernels_alone"]:
        print("GATE FAILED: insert %.3f ms is not below the batch build's %.3f ms" % (gate["insert_device_ms"], gate["batch_build_kernels_device_ms"]))
        sys.exit(1)


if __name__ == "__main__":
    main()
