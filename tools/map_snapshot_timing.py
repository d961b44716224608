#!/usr/bin/env python
"""What saving, restoring and merging an incremental target map costs, against a full rehash of the same map.

Three maps, as tools/map_insert_timing.py builds them: the bundled 17k-point scan, the 100k-point synthetic scene (resolution 1.0) and the
1M-point scene of bench.py's synth1m (resolution 0.5). Per map, HIP-event device times (the engine's profiler) and host wall times of
  export      : the gather kernel alone (class map_export), with the device-to-host copy (+ map_export_copy), and the whole call (wall: + host sort)
  import      : a snapshot added into an EMPTY map sized for it (restore) and into an EQUAL map (class map_import: kernel + refresh; wall: + validation, upload)
  merge_from  : another handle's equal map added device to device (class map_merge: kernel + refresh)
  rehash      : the yardstick, existing code measured in the same run -- a prune that removes nothing moves every bucket at unchanged capacity (class map_rehash)
After a warm-up, medians of --repeats runs, one process. The gate: merge_from takes at most 2 x the rehash on every map measured (a rehash
does one claim, ten stores and a record write per voxel; a merge the same plus a read-modify-write of the sums and the refresh launch).
Exits non-zero when the gate is missed.

    python tools/map_snapshot_timing.py OUT_DIR [--repeats 20] [--legs 17k,100k,1m]"""
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
    ap.add_argument("--legs", default="17k,100k,1m")
    args = ap.parse_args()
    import torch
    from fast_gicp_amd import capi, preprocess, workloads
    sync = torch.cuda.synchronize
    _, scan = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "legs": {}}
    failed = []
    for leg in args.legs.split(","):
        res = 0.5 if leg == "1m" else 1.0
        if leg == "17k":
            cloud = scan
        else:
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            cloud = workloads.synthetic_scene(n, seed, extent)

        def handle():
            h = capi.VGICPCore(0)
            h.set_resolution(res); h.set_neighbor_search_method(capi.DIRECT7); h.profile_enable(True)
            return h

        c, o, r = handle(), handle(), handle()
        cov = covariances(c, cloud)
        for h in (c, o):
            h.map_begin(); h.map_insert_cloud(cloud, cov)
        info = c.map_info()
        assert o.map_info()["num_voxels"] == info["num_voxels"]

        def timed(h, classes, fn):
            h.synchronize(); h.profile_reset(); sync()
            t0 = time.perf_counter()
            ret = fn()
            h.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            return [h.profile_get(k)[0] for k in classes], wall, ret

        W = 3
        ex_k, ex_c, ex_w, im_e, im_ew, im_q, im_qw, mg, mg_w, rh = ([] for _ in range(10))
        snap = None
        for i in range(W + args.repeats):
            (k, cp), w, snap = timed(c, ("map_export", "map_export_copy"), c.map_export)
            r.map_begin(snap["num_voxels"])
            (d_e,), w_e, _ = timed(r, ("map_import",), lambda: r.map_import(snap))
            (d_q,), w_q, _ = timed(c, ("map_import",), lambda: c.map_import(snap))
            (d_m,), w_m, _ = timed(c, ("map_merge",), lambda: c.map_merge_from(o))
            (d_r,), _, removed = timed(c, ("map_rehash",), lambda: c.map_prune([0.0, 0.0, 0.0], 1e9, 0))
            assert removed == 0
            if i >= W:
                ex_k.append(k); ex_c.append(k + cp); ex_w.append(w); im_e.append(d_e); im_ew.append(w_e); im_q.append(d_q); im_qw.append(w_q); mg.append(d_m); mg_w.append(w_m); rh.append(d_r)
        end = c.map_info()
        assert end["num_voxels"] == info["num_voxels"] and end["capacity"] == info["capacity"] and end["dropped"] == 0, (info, end)
        assert r.map_info()["num_voxels"] == info["num_voxels"] and r.map_info()["dropped"] == 0
        row = dict(map_points=int(len(cloud)), resolution=res, num_voxels=info["num_voxels"], capacity=info["capacity"], snapshot_bytes=96 * info["num_voxels"],
                   export_kernel_device_ms=med(ex_k), export_with_copy_device_ms=med(ex_c), export_wall_ms=med(ex_w),
                   import_into_empty_device_ms=med(im_e), import_into_empty_wall_ms=med(im_ew), import_into_equal_device_ms=med(im_q), import_into_equal_wall_ms=med(im_qw),
                   merge_from_device_ms=med(mg), merge_from_wall_ms=med(mg_w), rehash_device_ms=med(rh))
        row["merge_over_rehash"] = row["merge_from_device_ms"] / row["rehash_device_ms"]
        row["gate_merge_at_most_2x_rehash"] = row["merge_over_rehash"] <= 2.0
        print("%-5s %d voxels: export %.3f ms kernel, %.3f with copy, %.3f wall | import %.3f ms device (%.3f wall) into an empty map, %.3f (%.3f) into an equal one | "
              "merge_from %.3f ms device | rehash %.3f ms | merge / rehash %.2f" % (leg, row["num_voxels"], row["export_kernel_device_ms"], row["export_with_copy_device_ms"], row["export_wall_ms"],
                                                                                  row["import_into_empty_device_ms"], row["import_into_empty_wall_ms"], row["import_into_equal_device_ms"],
                                                                                  row["import_into_equal_wall_ms"], row["merge_from_device_ms"], row["rehash_device_ms"], row["merge_over_rehash"]), flush=True)
        if not row["gate_merge_at_most_2x_rehash"]:
            failed.append(leg)
        out["legs"][leg] = row
        for h in (c, o, r):
            h.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "map_snapshot_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    if failed:
        print("GATE FAILED: merge_from took more than 2 x the rehash of the same map on: %s" % ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    main()
