#!/usr/bin/env python
"""What adding a map under a rigid pose, and re-anchoring a live map, cost -- against the same-frame merge, a full rehash and the host route they replace.

Three maps, as tools/map_snapshot_timing.py builds them: the bundled 17k-point scan, the 100k-point synthetic scene (resolution 1.0) and the
1M-point scene of bench.py's synth1m (resolution 0.5). Per map, HIP-event device times (the engine's profiler) and host wall times of
  merge_from_posed : another handle's equal map added under a general pose (class map_merge_posed: kernel + refresh)
  map_transform    : a restored copy of the map re-anchored by that pose (class transform_map: kernel + refresh; wall: + the clears and the bitmap)
  merge_from       : the same map added in the same frame (class map_merge), existing code measured in the same process
  rehash           : a prune that removes nothing (class map_rehash), existing code
  host route       : what the device call replaces -- export, numpy transform_rows (tests/posedmerge_ref.py), import -- wall time
After a warm-up, medians of --repeats runs, one process. The gate: the device route's wall time is below the host route's on every map.
The ratios to merge_from and to the rehash are reported, not gated. Exits non-zero when the gate is missed.

    python tools/map_posed_merge_timing.py OUT_DIR [--repeats 10] [--legs 17k,100k,1m]"""
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--legs", default="17k,100k,1m")
    args = ap.parse_args()
    import torch
    from fast_gicp_amd import capi, preprocess, workloads
    from tests import posedmerge_ref as P
    sync = torch.cuda.synchronize
    _, scan = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    T = P.GENERAL
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "pose": T.tolist(), "legs": {}}
    failed = []
    for leg in args.legs.split(","):
        res = 0.5 if leg == "1m" else 1.0
        if leg == "17k":
            cloud = scan
        else:
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            cloud = workloads.synthetic_scene(n, seed, extent)

        def handle():
            h = capi.VGICPMapCore(0)
            h.set_resolution(res); h.set_neighbor_search_method(capi.DIRECT7); h.profile_enable(True)
            return h

        c, o, host, t = handle(), handle(), handle(), handle()
        c.set_source_cloud(cloud); c.find_source_neighbors(20); c.calculate_source_covariances()
        cov = c.get_covariances("source").copy()
        for h in (c, o, host):
            h.map_begin(); h.map_insert_cloud(cloud, cov)
        snap = o.map_export()

        def timed(h, classes, fn):
            h.synchronize(); h.profile_reset(); sync()
            t0 = time.perf_counter()
            ret = fn()
            h.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            return [h.profile_get(k)[0] for k in classes], wall, ret

        def host_route():
            e = o.map_export()
            coords, sums, ages, skipped, _, _ = P.transform_rows(e, T)
            keep = ~skipped
            host.map_import(dict(e, coords=coords[keep], sums=sums[keep], ages=ages[keep], num_voxels=int(keep.sum())))

        W = 2
        mp, mp_w, tr, tr_w, mg, mg_w, rh, hr_w = ([] for _ in range(8))
        for i in range(W + args.repeats):
            (d_p,), w_p, skipped = timed(c, ("map_merge_posed",), lambda: c.map_merge_from_posed(o, T))
            assert skipped == 0
            t.map_begin(snap["num_voxels"]); t.map_import(snap)
            (d_t,), w_t, skipped = timed(t, ("transform_map",), lambda: t.map_transform(T))
            assert skipped == 0
            (d_m,), w_m, _ = timed(c, ("map_merge",), lambda: c.map_merge_from(o))
            (d_r,), _, removed = timed(c, ("map_rehash",), lambda: c.map_prune([0.0, 0.0, 0.0], 1e9, 0))
            assert removed == 0
            _, w_h, _ = timed(host, (), host_route)
            if i >= W:
                mp.append(d_p); mp_w.append(w_p); tr.append(d_t); tr_w.append(w_t); mg.append(d_m); mg_w.append(w_m); rh.append(d_r); hr_w.append(w_h)
        end, hend = c.map_info(), host.map_info()
        assert end["dropped"] == 0 and hend["dropped"] == 0 and end["num_voxels"] == hend["num_voxels"], (end, hend)
        row = dict(map_points=int(len(cloud)), resolution=res, other_voxels=snap["num_voxels"], merged_voxels=end["num_voxels"], capacity=end["capacity"],
                   merge_from_posed_device_ms=med(mp), merge_from_posed_wall_ms=med(mp_w), map_transform_device_ms=med(tr), map_transform_wall_ms=med(tr_w),
                   merge_from_device_ms=med(mg), merge_from_wall_ms=med(mg_w), rehash_device_ms=med(rh), host_route_wall_ms=med(hr_w))
        row["posed_over_merge_from"] = row["merge_from_posed_device_ms"] / row["merge_from_device_ms"]
        row["posed_over_rehash"] = row["merge_from_posed_device_ms"] / row["rehash_device_ms"]
        row["transform_over_rehash"] = row["map_transform_device_ms"] / row["rehash_device_ms"]
        row["host_route_over_device_route_wall"] = row["host_route_wall_ms"] / row["merge_from_posed_wall_ms"]
        row["gate_device_wall_below_host_wall"] = row["merge_from_posed_wall_ms"] < row["host_route_wall_ms"]
        print("%-5s %d voxels: merge_from_posed %.3f ms device (%.3f wall) | map_transform %.3f (%.3f) | merge_from %.3f (%.3f) | rehash %.3f | host route %.3f wall | "
              "posed / merge_from %.2f, posed / rehash %.2f, host / device wall %.1f" % (leg, row["other_voxels"], row["merge_from_posed_device_ms"], row["merge_from_posed_wall_ms"],
                                                                                         row["map_transform_device_ms"], row["map_transform_wall_ms"], row["merge_from_device_ms"],
                                                                                         row["merge_from_wall_ms"], row["rehash_device_ms"], row["host_route_wall_ms"], row["posed_over_merge_from"],
                                                                                         row["posed_over_rehash"], row["host_route_over_device_route_wall"]), flush=True)
        if not row["gate_device_wall_below_host_wall"]:
            failed.append(leg)
        out["legs"][leg] = row
        for h in (c, o, host, t):
            h.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "map_posed_merge_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    if failed:
        print("GATE FAILED: the posed merge's wall time is not below the host route's on: %s" % ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    main()
