#!/usr/bin/env python
"""align_multi against K sequential align() calls on the same handle, K in {1, 2, 4, 8, 16, 32}: the bundled pair (VGICP DIRECT27, and NDT D2D
at the lidar_stream settings: resolution 1.0, DIRECT1) and the 1M-point map <-> 100k scan (VGICP DIRECT7, resolution 0.5, seed 44 as bench.py's
synth1m). Warm-up, then the median of --repeats runs, host clocks around device-synchronised calls. Records the route align_multi took
(persistent: one launch; else one launch per transition) and the workgroups per hypothesis (nb_h).

    python tools/multi_guess_timing.py OUT_DIR [--repeats 5] [--ks 1,2,4,8,16,32] [--workloads vgicp17k,ndt17k,map1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def yaw_guesses(k):
    out = []
    for i in range(k):
        a = np.deg2rad(0.0 if i == 0 else (360.0 * i / k if k > 12 else [15, -15, 30, -30, 60, -60, 90, -90, 120, -120, 180][(i - 1) % 11]))
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        out.append(T)
    return np.stack(out)


def make(name):
    from fast_gicp_amd import capi, preprocess, workloads
    if name in ("vgicp17k", "ndt17k"):
        tgt, src = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    else:
        tgt, src, _ = workloads.synthetic_pair(1_000_000, 100_000, seed=44, extent=150.0)
    if name == "ndt17k":
        c = capi.NDTCore(0)
        c.set_distance_mode(capi.NDT_D2D); c.set_neighbor_search_method(capi.DIRECT1); c.set_resolution(1.0)
        c.set_target_cloud(tgt); c.set_source_cloud(src)
        return c
    c = capi.VGICPCore(0)
    if name == "map1m":
        c.set_resolution(0.5); c.set_neighbor_search_method(capi.DIRECT7)
    else:
        c.set_neighbor_search_method(capi.DIRECT27)
    c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances(); c.create_target_voxelmap()
    c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
    return c


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    r = fn()
    sync()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--workloads", default="vgicp17k,ndt17k,map1m")
    args = ap.parse_args()
    import torch
    sync = torch.cuda.synchronize
    ks = [int(k) for k in args.ks.split(",")]
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in args.workloads.split(","):
        c = make(name)
        for _ in range(3):
            c.align()
        rows = []
        for k in ks:
            G = yaw_guesses(k)
            c.align_multi(G)  # warm-up (grows the per-hypothesis buffers once)
            [c.align(g) for g in G]
            tm, ts, info = [], [], None
            for _ in range(args.repeats):
                dt, ms = timed(lambda: c.align_multi(G), sync)
                tm.append(dt)
                info = ms
                dt, _ = timed(lambda: [c.align(g) for g in G], sync)
                ts.append(dt)
            row = dict(k=k, multi_ms=1e3 * float(np.median(tm)), sequential_ms=1e3 * float(np.median(ts)),
                       route="persistent" if all(m["num_launches"] == 1 for m in info) else "multi_launch",
                       nb_h=info[0]["grid_blocks"], trips=[1 + m["num_error_evals"] for m in info], converged=[m["converged"] for m in info])
            row["speedup"] = row["sequential_ms"] / row["multi_ms"]
            rows.append(row)
            print("%-9s K=%2d multi %8.3f ms  sequential %8.3f ms  x%.2f  %s nb_h=%d" % (name, k, row["multi_ms"], row["sequential_ms"], row["speedup"], row["route"], row["nb_h"]), flush=True)
        out["workloads"][name] = rows
        c.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "multi_guess_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
