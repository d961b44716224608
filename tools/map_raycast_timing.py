#!/usr/bin/env python
"""What casting rays into the target voxel map (fvh_vgicp_cast_rays_source) costs -- against the host route it replaces.

The rays run from the sensor (the scan frame's origin) to the points of the bundled 17k-point scan, at the pose a registration of the bundled
pair finds, max_range 100 m, max_m2 9, against three maps at resolution 0.5: the map of the scan pair itself, the 100k-point synthetic
scene and the 1M-point scene of bench.py's synth1m. Per map, after a warm-up, medians of --repeats runs in one process:
  call          : the cast kernel (HIP events: class map_raycast) and the host wall time, without and with the per-ray rows
  host route    : what the parent offers for the same answer -- get_voxel_coords / num_points / means / covs over PCIe (the host copy is
                  invalidated in front of every run, as an insert between two scans does) and a vectorised numpy walk (this file: all rays
                  step in lockstep, sorted packed keys + searchsorted per step, the closed-form closest approach on the cells that exist) --
                  wall time, median of --host-runs runs; it must give the same n_hit
  reported only : vm_raymark_kernel (class map_raymark) on the same rays and map through clear_rays_source with a min_misses nothing reaches
                  (it removes nothing), and cells visited per microsecond of the cast kernel
The gate: the call's wall time (both forms) is below the host route's on every map, and the host route's n_hit equals the device's. Exits
non-zero when it is missed.

    python tools/map_raycast_timing.py [OUT_DIR = profiles] [--repeats 10] [--host-runs 3] [--legs pair,100k,1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIAS = 1 << 20
LIM = BIAS - 4096


def med(x):
    return float(np.median(x))


def pack(c):
    c = c.astype(np.int64) + BIAS
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def _bilinear(u, v, A):
    return (((u[:, 0] * v[:, 0]) * A[0] + (u[:, 1] * v[:, 1]) * A[3]) + (u[:, 2] * v[:, 2]) * A[5]) + ((((u[:, 0] * v[:, 1] + u[:, 1] * v[:, 0]) * A[1]) + ((u[:, 0] * v[:, 2] + u[:, 2] * v[:, 0]) * A[2])) +
                                                                                                 ((u[:, 1] * v[:, 2] + u[:, 2] * v[:, 1]) * A[4]))


def host_cast(coords, num, means, covs, res, pts, T, origin, min_range, max_range, min_points, max_m2):
    """the contract of fvh_*_cast_rays_* on all rays at once (numpy, fp64; the rays step in lockstep) -> the struct's fields and the ranges"""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    P = np.asarray(pts, np.float32).astype(np.float64)
    n = len(P)
    with np.errstate(all="ignore"):
        q = (((P[:, :1] * R[:, 0] + P[:, 1:2] * R[:, 1]) + P[:, 2:] * R[:, 2]) + t).astype(np.float32).astype(np.float64)
        og = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
        o = (((og[0] * R[:, 0] + og[1] * R[:, 1]) + og[2] * R[:, 2]) + t).astype(np.float32).astype(np.float64)
        a0, b = o / res - 0.5, q / res - 0.5
        fa, fb = np.floor(a0), np.floor(b)
        dm = q - o
        r = np.sqrt((dm[:, 0] * dm[:, 0] + dm[:, 1] * dm[:, 1]) + dm[:, 2] * dm[:, 2])
        used = np.isfinite(P).all(axis=1) & ~(r == 0.0) & ~(r > max_range) & (np.abs(fa) < LIM).all() & (np.abs(fb) < LIM).all(axis=1)
    rows_used = np.flatnonzero(used)
    b, fb, dm, r = b[used], fb[used], dm[used], r[used]
    m = len(r)
    a = np.broadcast_to(a0, (m, 3))
    c = np.broadcast_to(fa, (m, 3)).astype(np.int64).copy()
    e = fb.astype(np.int64)
    d = b - a
    s = np.sign(d).astype(np.int64)
    with np.errstate(all="ignore"):
        t_delta = 1.0 / np.abs(d)
        t_max = np.where(d > 0.0, ((c + 1).astype(np.float64) - a) / d, np.where(d < 0.0, (a - c.astype(np.float64)) / (-d), np.inf))
    t_lo = min_range / r
    n_steps = np.abs(e - c).sum(axis=1)
    keys = pack(np.asarray(coords))
    order = np.argsort(keys)
    skeys = keys[order]
    C = np.asarray(covs, np.float64).reshape(-1, 3, 3)
    cxx, cxy, cxz, cyy, cyz, czz = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    with np.errstate(all="ignore"):
        adj = np.stack([cyy * czz - cyz * cyz, cxz * cyz - cxy * czz, cxy * cyz - cxz * cyy, cxx * czz - cxz * cxz, cxy * cxz - cxx * cyz, cxx * cyy - cxy * cxy])
        det = (cxx * adj[0] + cxy * adj[1]) + cxz * adj[2]
    mu = np.asarray(means, np.float32).astype(np.float64)
    eligible = np.asarray(num) >= min_points if min_points > 1 else np.ones(len(keys), bool)
    t_in = np.zeros(m)
    step = np.zeros(m, np.int64)
    active = np.ones(m, bool)
    hit = np.zeros(m, bool)
    rng = np.full(m, np.inf)
    hit_first = np.zeros(m, bool)
    n_cells = 0
    ar = np.arange(m)
    while active.any() and len(skeys):
        idx = np.flatnonzero(active)
        n_cells += len(idx)
        tm = t_max[idx]
        axis = np.where((tm[:, 0] <= tm[:, 1]) & (tm[:, 0] <= tm[:, 2]), 0, np.where(tm[:, 1] <= tm[:, 2], 1, 2))
        t_next = tm[ar[:len(idx)], axis]
        last = step[idx] == n_steps[idx]
        t_out = np.where(last | ~(t_next < 1.0), 1.0, t_next)
        k = pack(c[idx])
        i = np.minimum(np.searchsorted(skeys, k), len(skeys) - 1)
        rows = order[i]
        found = (t_out > t_lo[idx]) & (skeys[i] == k) & eligible[rows]
        j, rw, hi = idx[found], rows[found], t_out[found]
        lo = np.maximum(t_in[j], t_lo[j])
        ev, dv, A, dt = o - mu[rw], dm[j], adj[:, rw], det[rw]
        with np.errstate(all="ignore"):
            den, num_ = _bilinear(dv, dv, A), _bilinear(dv, ev, A)
            sing = ~(dt > 0.0) | ~np.isfinite(dt) | ~(den > 0.0) | ~np.isfinite(den) | ~np.isfinite(num_)
            sstar = (-num_) / den
            sv = np.where(sing, lo, np.where(sstar < lo, lo, np.where(sstar > hi, hi, sstar)))
            x = ev + sv[:, None] * dv
            qq = (((x[:, 0] * x[:, 0]) * A[0] + (x[:, 1] * x[:, 1]) * A[3]) + (x[:, 2] * x[:, 2]) * A[5]) + 2.0 * ((((x[:, 0] * x[:, 1]) * A[1]) + ((x[:, 0] * x[:, 2]) * A[2])) + ((x[:, 1] * x[:, 2]) * A[4]))
            m2 = np.where(sing | ~np.isfinite(qq), np.inf, np.maximum(qq / dt, 0.0))
        h = m2 <= max_m2
        hit[j[h]] = True
        rng[j[h]] = sv[h] * r[j[h]]
        hit_first[j[h]] = step[j[h]] == 0
        active[j[h]] = False
        go = active[idx] & ~last
        active[idx[last]] = False
        gi, ga = idx[go], axis[go]
        t_in[gi] = t_next[go]
        c[gi, ga] += s[gi, ga]
        t_max[gi, ga] += t_delta[gi, ga]
        step[gi] += 1
        active[gi] = t_in[gi] < 1.0
    if not len(skeys):
        n_cells = int((n_steps + 1).sum())  # (an empty map: every ray walks to its end; not timed anywhere)
    ranges = np.full(n, np.nan)
    ranges[rows_used] = rng
    return dict(n_rays=int(n), n_used=int(m), n_hit=int(hit.sum()), n_hit_at_origin=int(hit_first.sum()), n_cells=int(n_cells), range=ranges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--legs", default="pair,100k,1m")
    args = ap.parse_args()
    import torch
    from fast_gicp_amd import capi, preprocess, workloads
    sync = torch.cuda.synchronize
    tgt, scan = preprocess.bundled_pair(os.path.join(ROOT, "data"))
    res, max_m2, min_points, max_range = 0.5, 9.0, 1, 100.0

    def handle(search=capi.DIRECT7):
        h = capi.VGICPMapCore(0)
        h.set_resolution(res); h.set_neighbor_search_method(search); h.profile_enable(True)
        return h

    reg = handle()
    reg.set_target_cloud(tgt); reg.find_target_neighbors(20); reg.calculate_target_covariances(); reg.create_target_voxelmap()
    reg.set_source_cloud(scan); reg.find_source_neighbors(20); reg.calculate_source_covariances()
    cov_t, cov_s = reg.get_covariances("target").astype(np.float64), reg.get_covariances("source").astype(np.float64)
    T = reg.align()["T"].copy()
    reg.close()
    flat = np.array([[0.01, 0.0, 0.0], [0.0, 0.01, 0.0], [0.0, 0.0, 0.01]])
    none3, none33 = np.zeros((0, 3), np.float32), np.zeros((0, 3, 3))
    out = {"repeats": args.repeats, "host_runs": args.host_runs, "device": torch.cuda.get_device_name(0), "pose": T.tolist(), "resolution": res, "max_m2": max_m2, "max_range": max_range,
           "min_points": min_points, "rays": int(len(scan)), "legs": {}}
    failed = []
    for leg in args.legs.split(","):
        c = handle()
        c.map_begin()
        if leg == "pair":
            c.map_insert_cloud(tgt, cov_t); c.map_insert_cloud(scan, cov_s, T)
            n_points = len(tgt) + len(scan)
        else:
            n, extent, seed = (1_000_000, 150.0, 44) if leg == "1m" else (100_000, 60.0, 42)
            cloud = workloads.synthetic_scene(n, seed, extent)
            c.map_insert_cloud(cloud, np.broadcast_to(flat, (len(cloud), 3, 3)))
            n_points = len(cloud)
        c.set_source_cloud(scan)

        def timed(classes, fn):
            c.synchronize(); c.profile_reset(); sync()
            t0 = time.perf_counter()
            ret = fn()
            c.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            return [c.profile_get(k)[0] for k in classes], wall, ret

        def host_route():
            coords, num, means, covs = c.get_voxelmap()
            return host_cast(coords, num, means, covs, res, scan, T, None, 0.0, max_range, min_points, max_m2)

        kw = dict(max_range=max_range, min_points=min_points, max_m2=max_m2)
        W = 2
        dev, wall, dev_pr, wall_pr, hr, mark = ([] for _ in range(6))
        got = rows = host = None
        for i in range(W + args.repeats):
            (d,), w, got = timed(("map_raycast",), lambda: c.map_cast_rays(T, per_ray=False, **kw))
            (d2,), w2, rows = timed(("map_raycast",), lambda: c.map_cast_rays(T, per_ray=True, **kw))
            (d_m,), _, (removed, used) = timed(("map_raymark",), lambda: c.map_clear_rays(T, max_range=max_range, min_misses=len(scan) + 1))
            assert removed == 0
            if i >= W:
                dev.append(d); wall.append(w); dev_pr.append(d2); wall_pr.append(w2); mark.append(d_m)
        for i in range(args.host_runs):
            c.map_insert_cloud(none3, none33)  # (an insert -- here of nothing -- is what invalidates the host copy of the map between two scans)
            _, w_h, host = timed((), host_route)
            hr.append(w_h)
        counts = ("n_rays", "n_used", "n_hit", "n_hit_at_origin", "n_cells")
        hits = rows["hit"] == 1
        row = dict(map_points=int(n_points), voxels=c.map_info()["num_voxels"], capacity=c.map_info()["capacity"], **{k: int(got[k]) for k in counts},
                   rays_used_by_raymark=int(used), host_route=dict((k, host[k]) for k in counts), host_route_n_hit_matches_device=bool(host["n_hit"] == got["n_hit"]),
                   host_route_counts_match_device=bool(all(host[k] == got[k] for k in counts)),
                   host_route_max_abs_range_diff_m=float(np.abs(host["range"][hits] - rows["range"][hits]).max()) if hits.any() and host["n_hit"] == got["n_hit"] else None,
                   median_hit_range_m=float(np.median(rows["range"][hits])) if hits.any() else None,
                   raycast_device_ms=med(dev), call_wall_ms=med(wall), per_ray_raycast_device_ms=med(dev_pr), per_ray_call_wall_ms=med(wall_pr), host_route_wall_ms=med(hr),
                   raymark_device_ms=med(mark))
        row["raycast_device_over_raymark_device"] = row["raycast_device_ms"] / row["raymark_device_ms"]
        row["cells_per_microsecond"] = row["n_cells"] / (1e3 * row["raycast_device_ms"])
        row["cells_per_used_ray"] = row["n_cells"] / max(row["n_used"], 1)
        row["host_route_over_call_wall"] = row["host_route_wall_ms"] / row["call_wall_ms"]
        row["gate_call_wall_below_host_route_wall"] = bool(row["call_wall_ms"] < row["host_route_wall_ms"] and row["per_ray_call_wall_ms"] < row["host_route_wall_ms"] and row["host_route_n_hit_matches_device"])
        print("%-5s %d voxels, %d rays (%d used, %d hit, %d cells): cast %.3f ms device, call %.3f ms wall (per ray: %.3f) | host route %.1f ms wall (x%.1f), same n_hit: %s | raymark %.3f ms "
              "device (cast / raymark %.2f) | %.1f cells/us" % (leg, row["voxels"], got["n_rays"], got["n_used"], got["n_hit"], got["n_cells"], row["raycast_device_ms"], row["call_wall_ms"],
                                                              row["per_ray_call_wall_ms"], row["host_route_wall_ms"], row["host_route_over_call_wall"], row["host_route_n_hit_matches_device"],
                                                              row["raymark_device_ms"], row["raycast_device_over_raymark_device"], row["cells_per_microsecond"]), flush=True)
        if not row["gate_call_wall_below_host_route_wall"]:
            failed.append(leg)
        out["legs"][leg] = row
        c.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "map_raycast_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    if failed:
        print("GATE FAILED: the call's wall time is not below the host route's, or the host route's n_hit differs, on: %s" % ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    main()
