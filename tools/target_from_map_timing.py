#!/usr/bin/env python
"""What it costs to make the live incremental map the handle's target cloud: fvh_vgicp_target_from_map against the host route it replaces.

Maps: the bundled 17k-point scan alone, and the scan on top of the 100k-point and the 1M-point synthetic scene (resolution 0.5 for the
latter, as tools/map_insert_timing.py builds them). Per map, medians over --repeats after a warm-up, one process:

  device route   target_from_map(1): `device` = HIP events on the handle's stream around its kernels (the engine's profiler, class
                 map_target: select + keys + radix passes + gather; the pack kernel of the upload is class-less and not in it), `wall` =
                 the host clock around the call, its 32-byte readback and stream synchronisation included, + a synchronize.
  host route     get_voxelmap() + numpy key sort + set_target_cloud + set_target_covariances: `device` = the events around the table's
                 trip over PCIe (class map_fetch: 64 B per BUCKET, not per voxel; the uploads back are not bracketed), `wall` = the host
                 clock around all of it.

Before every repeat a one-point cloud is inserted far away, as a frame's insert would: the getters' host copy of the table is stale again
(the host route pays its PCIe trip every time, as it does in a scan-to-map loop) and the map grows by one voxel per repeat.

    python tools/target_from_map_timing.py OUT_DIR [--repeats 15] [--legs scan,100k,1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COORD_BIAS = 1 << 20


def covariances(c, pts):
    c.set_source_cloud(pts); c.find_source_neighbors(20); c.calculate_source_covariances()
    return c.get_covariances("source").copy()


def key_order(coords):
    k = np.asarray(coords, np.int64) + COORD_BIAS
    return np.argsort((k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)).astype(np.uint64), kind="stable")


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--legs", default="scan,100k,1m")
    args = ap.parse_args()
    import torch
    from fast_gicp_amd import capi, preprocess, workloads
    _, scan = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "scan_points": int(len(scan)), "legs": {}}
    one, one_cov = np.zeros((1, 3), np.float32), np.eye(3)[None]
    for leg in args.legs.split(","):
        res = 0.5 if leg == "1m" else 1.0
        c = capi.VGICPMapCore(0)
        c.set_resolution(res); c.set_neighbor_search_method(capi.DIRECT7)
        c.map_begin()
        if leg != "scan":
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            base = workloads.synthetic_scene(n, seed, extent)
            c.map_insert_cloud(base, covariances(c, base))
        c.map_insert_cloud(scan, covariances(c, scan))
        c.profile_enable(True)
        step = [0]

        def touch():  # a frame's insert: the host copy of the table is stale again
            step[0] += 1
            T = np.eye(4); T[2, 3] = 500.0 + 3.0 * step[0]
            c.map_insert_cloud(one, one_cov, T)
            c.synchronize(); c.profile_reset()

        def device_route():
            touch()
            t0 = time.perf_counter()
            n = c.target_from_map(1)
            c.synchronize()
            wall = time.perf_counter() - t0
            return n, c.profile_get("map_target")[0], 1e3 * wall

        def host_route():
            touch()
            t0 = time.perf_counter()
            coords, _, means, covs = c.get_voxelmap()
            o = key_order(coords)
            c.set_target_cloud(means[o]); c.set_target_covariances(covs[o].astype(np.float64))
            c.synchronize()
            wall = time.perf_counter() - t0
            return len(o), c.profile_get("map_fetch")[0], 1e3 * wall

        row = dict(resolution=res)
        for name, fn in (("device_route", device_route), ("host_route", host_route)):
            for _ in range(3):
                fn()
            dev, wall, n = [], [], 0
            for _ in range(args.repeats):
                n, d, w = fn()
                dev.append(d); wall.append(w)
            row[name] = dict(points=int(n), device_ms=med(dev), wall_ms=med(wall))
        # the two routes leave the same cloud (the last host-route cloud against a device-route one made of the same map)
        hp, hc = c.get_target_points(), c.get_covariances("target")
        assert c.target_from_map(1) == len(hp)
        row["routes_agree_to_the_bit"] = bool(hp.tobytes() == c.get_target_points().tobytes() and hc.tobytes() == c.get_covariances("target").tobytes())
        info = c.map_info()
        row.update(num_voxels=info["num_voxels"], capacity=info["capacity"], table_bytes=64 * info["capacity"])
        row["device_route_faster_wall"] = row["device_route"]["wall_ms"] < row["host_route"]["wall_ms"]
        print("%-5s %8d voxels (table %5.1f MB): device route %.3f ms device / %.3f ms wall; host route %.3f ms fetch / %.3f ms wall; same cloud: %s"
              % (leg, row["num_voxels"], row["table_bytes"] / 1e6, row["device_route"]["device_ms"], row["device_route"]["wall_ms"], row["host_route"]["device_ms"],
                 row["host_route"]["wall_ms"], row["routes_agree_to_the_bit"]), flush=True)
        out["legs"][leg] = row
        c.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "target_from_map_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
