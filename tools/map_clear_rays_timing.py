#!/usr/bin/env python
"""What free-space carving (fvh_vgicp_clear_rays_source) costs -- against the host route it replaces, a full rehash and a DIRECT27 lookup pass.

The rays are the bundled 17k-point scan at the pose a registration of the bundled pair finds, origin = the sensor, max_range 100 m, against
three maps at resolution 0.5: the map of the scan pair itself, the 100k-point synthetic scene and the 1M-point scene of bench.py's synth1m.
Per map, after a warm-up, medians of --repeats runs in one process (the map is restored from its snapshot in front of every run):
  call          : mark kernel, sweep kernel and rehash apart (HIP events: classes map_raymark, map_raysweep, map_rehash) and the host wall time
  idle call     : the same call with min_misses above the ray count -- nothing is removed, no rehash runs
  cells / us    : the cells the rays cross (counted by the host walk below) over the mark kernel's device time
  host route    : what the parent offers for the same result -- voxelmap_export, a lock-step vectorised numpy walk of all rays (this file),
                  map_begin + voxelmap_import of the surviving rows -- wall time
  reported only : a prune that removes nothing (class map_rehash) and one DIRECT27 update_correspondences of the same scan (class cost)
The gate: the call's wall time is below the host route's on every map. Exits non-zero when it is missed.

    python tools/map_clear_rays_timing.py [OUT_DIR = profiles] [--repeats 10] [--legs pair,100k,1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIAS = 1 << 20


def med(x):
    return float(np.median(x))


def pack(c):
    c = c.astype(np.int64) + BIAS
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def host_walk(snapshot, pts, T, origin, max_range, end_margin, min_misses):
    """the contract of fvh_*_clear_rays_* on all rays in lock step (numpy, fp64): -> (keep mask over the snapshot's rows, cells crossed, rays used)"""
    res = float(snapshot["resolution"])
    R, t = np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3]
    P = np.asarray(pts, np.float32).astype(np.float64)
    o = np.asarray(origin, np.float64)
    o32 = (((R[:, 0] * o[0] + R[:, 1] * o[1]) + R[:, 2] * o[2]) + t).astype(np.float32).astype(np.float64)
    p32 = (((P[:, :1] * R[:, 0] + P[:, 1:2] * R[:, 1]) + P[:, 2:] * R[:, 2]) + t).astype(np.float32).astype(np.float64)
    a, b = o32 / res - 0.5, p32 / res - 0.5
    dm = p32 - o32
    r = np.sqrt((dm[:, 0] * dm[:, 0] + dm[:, 1] * dm[:, 1]) + dm[:, 2] * dm[:, 2])
    lim = BIAS - 4096
    ok = np.isfinite(P).all(axis=1) & (r != 0.0) & ~(r > max_range) & (np.abs(np.floor(b)) < lim).all(axis=1) & bool((np.abs(np.floor(a)) < lim).all())
    b, r = b[ok], r[ok]
    keys = pack(np.asarray(snapshot["coords"]))
    order = np.argsort(keys)
    skeys = keys[order]
    misses = np.zeros(len(keys), np.int64)
    hit = np.zeros(len(keys), bool)

    def rows_of(cells):
        k = pack(cells)
        i = np.minimum(np.searchsorted(skeys, k), len(skeys) - 1)
        found = skeys[i] == k
        return order[i[found]]

    e = np.floor(b).astype(np.int64)
    hit[rows_of(e)] = True
    c = np.tile(np.floor(a).astype(np.int64), (len(b), 1))
    d = b - a
    s = np.sign(d).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_delta = 1.0 / np.abs(d)
        t_max = np.where(d > 0.0, ((c + 1).astype(np.float64) - a) / d, np.where(d < 0.0, (a - c.astype(np.float64)) / (-d), np.inf))
    t_end = 1.0 - end_margin / r
    n_steps = np.abs(e - c).sum(axis=1)
    t_in = np.zeros(len(b))
    steps = np.zeros(len(b), np.int64)
    live = np.arange(len(b))
    cells = 0
    while True:
        live = live[t_in[live] < t_end[live]]
        if not len(live):
            break
        cells += len(live)
        np.add.at(misses, rows_of(c[live]), 1)
        live = live[steps[live] < n_steps[live]]
        tm = t_max[live]
        k = np.where((tm[:, 0] <= tm[:, 1]) & (tm[:, 0] <= tm[:, 2]), 0, np.where(tm[:, 1] <= tm[:, 2], 1, 2))
        t_in[live] = tm[np.arange(len(live)), k]
        c[live, k] += s[live, k]
        t_max[live, k] += t_delta[live, k]
        steps[live] += 1
    return ~((misses >= min_misses) & ~hit), cells, int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--legs", default="pair,100k,1m")
    args = ap.parse_args()
    import torch
    from fast_gicp_amd import capi, preprocess, workloads
    sync = torch.cuda.synchronize
    tgt, scan = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    res, max_range, end_margin = 0.5, 100.0, 0.5
    origin = [0.0, 0.0, 0.0]

    def handle(search=None):
        h = capi.VGICPMapCore(0)
        h.set_resolution(res); h.set_neighbor_search_method(capi.DIRECT7 if search is None else search); h.profile_enable(True)
        return h

    reg = handle()
    reg.set_target_cloud(tgt); reg.find_target_neighbors(20); reg.calculate_target_covariances(); reg.create_target_voxelmap()
    reg.set_source_cloud(scan); reg.find_source_neighbors(20); reg.calculate_source_covariances()
    cov_t, cov_s = reg.get_covariances("target").astype(np.float64), reg.get_covariances("source").astype(np.float64)
    T = reg.align()["T"].copy()
    reg.close()
    flat = np.array([[0.01, 0.0, 0.0], [0.0, 0.01, 0.0], [0.0, 0.0, 0.01]])  # (the scenes' covariances: carving never reads the sums)
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "pose": T.tolist(), "resolution": res, "max_range": max_range, "end_margin": end_margin,
           "rays": int(len(scan)), "legs": {}}
    failed = []
    for leg in args.legs.split(","):
        c, host = handle(), handle()
        c.map_begin()
        if leg == "pair":
            c.map_insert_cloud(tgt, cov_t); c.map_insert_cloud(scan, cov_s, T)
            n_points = len(tgt) + len(scan)
        else:
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            cloud = workloads.synthetic_scene(n, seed, extent)
            c.map_insert_cloud(cloud, np.broadcast_to(flat, (len(cloud), 3, 3)))
            n_points = len(cloud)
        snap = c.map_export()
        c.set_source_cloud(scan); c.set_source_covariances(cov_s)
        keep, cells, rays_used = host_walk(snap, scan, T, origin, max_range, end_margin, 1)

        def restore(h):
            h.map_begin(snap["num_voxels"]); h.map_import(snap)

        def timed(h, classes, fn):
            h.synchronize(); h.profile_reset(); sync()
            t0 = time.perf_counter()
            ret = fn()
            h.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            return [h.profile_get(k)[0] for k in classes], wall, ret

        def host_route():
            e = host.map_export()
            k, _, _ = host_walk(e, scan, T, origin, max_range, end_margin, 1)
            host.map_begin(e["num_voxels"])
            host.map_import(dict(e, coords=e["coords"][k], sums=e["sums"][k], ages=e["ages"][k], num_voxels=int(k.sum())))
            return int((~k).sum())

        d27 = handle(capi.DIRECT27)
        restore(d27)
        d27.set_source_cloud(scan); d27.set_source_covariances(cov_s)
        W = 2
        mk, sw, rh, wl, idle_w, idle_mk, full_rh, hr_w, uc, uc_w = ([] for _ in range(10))
        removed = used = host_removed = None
        for i in range(W + args.repeats):
            restore(c)
            (d_m, d_s, d_r), w, (removed, used) = timed(c, ("map_raymark", "map_raysweep", "map_rehash"), lambda: c.map_clear_rays(T, origin=origin, max_range=max_range, end_margin=end_margin))
            restore(c)
            (d_i,), w_i, (none, _) = timed(c, ("map_raymark",), lambda: c.map_clear_rays(T, origin=origin, max_range=max_range, end_margin=end_margin, min_misses=len(scan) + 1))
            assert none == 0
            (d_f,), _, pruned = timed(c, ("map_rehash",), lambda: c.map_prune([0.0, 0.0, 0.0], 1e9, 0))
            assert pruned == 0
            restore(host)
            _, w_h, host_removed = timed(host, (), host_route)
            (d_u,), w_u, _ = timed(d27, ("cost",), lambda: d27.update_correspondences(T))
            if i >= W:
                mk.append(d_m); sw.append(d_s); rh.append(d_r); wl.append(w); idle_w.append(w_i); idle_mk.append(d_i); full_rh.append(d_f); hr_w.append(w_h); uc.append(d_u); uc_w.append(w_u)
        row = dict(map_points=int(n_points), voxels=snap["num_voxels"], capacity=c.map_info()["capacity"], rays_used=used, removed=removed, cells_crossed=int(cells),
                   host_walk_removed=host_removed, host_walk_rays_used=rays_used, host_route_matches_device=bool(host_removed == removed and rays_used == used),
                   mark_device_ms=med(mk), sweep_device_ms=med(sw), rehash_device_ms=med(rh), call_wall_ms=med(wl), idle_call_wall_ms=med(idle_w), idle_mark_device_ms=med(idle_mk),
                   full_rehash_device_ms=med(full_rh), host_route_wall_ms=med(hr_w), direct27_update_correspondences_device_ms=med(uc), direct27_update_correspondences_wall_ms=med(uc_w))
        row["cells_per_us"] = row["cells_crossed"] / (1e3 * row["mark_device_ms"]) if row["mark_device_ms"] > 0 else None
        row["host_route_over_call_wall"] = row["host_route_wall_ms"] / row["call_wall_ms"]
        row["gate_call_wall_below_host_route_wall"] = row["call_wall_ms"] < row["host_route_wall_ms"]
        print("%-5s %d voxels, %d rays, %d cells, %d removed: mark %.3f ms, sweep %.3f, rehash %.3f, call %.3f wall (idle %.3f) | %.1f cells/us | host route %.1f wall (x%.1f) | "
              "full rehash %.3f, DIRECT27 update_correspondences %.3f device" % (leg, row["voxels"], used, cells, removed, row["mark_device_ms"], row["sweep_device_ms"], row["rehash_device_ms"],
                                                                               row["call_wall_ms"], row["idle_call_wall_ms"], row["cells_per_us"] or 0.0, row["host_route_wall_ms"],
                                                                               row["host_route_over_call_wall"], row["full_rehash_device_ms"], row["direct27_update_correspondences_device_ms"]), flush=True)
        if not row["gate_call_wall_below_host_route_wall"]:
            failed.append(leg)
        out["legs"][leg] = row
        for h in (c, host, d27):
            h.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "map_clear_rays_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    if failed:
        print("GATE FAILED: the call's wall time is not below the host route's on: %s" % ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    main()
