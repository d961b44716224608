#!/usr/bin/env python
"""What scoring a posed scan against the target voxel map (fvh_vgicp_score_source) costs -- against the host route it replaces.

The scan is the bundled 17k-point scan at the pose a registration of the bundled pair finds, DIRECT27, max_m2 9, against three maps at
resolution 0.5: the map of the scan pair itself, the 100k-point synthetic scene and the 1M-point scene of bench.py's synth1m.
Per map, after a warm-up, medians of --repeats runs in one process:
  call          : score kernel + fixed-order sums (HIP events: class map_score) and the host wall time, without and with the per-point arrays
  host route    : what the parent offers for the same numbers -- get_voxel_coords / num_points / means / covs over PCIe (the host copy is
                  invalidated in front of every run, as an insert between two scans does) and a vectorised numpy scorer (this file: sorted
                  packed keys + searchsorted per offset, batched closed-form inverse) -- wall time
  reported only : update_correspondences + compute_error (error only) of the same scan, pose and DIRECT27 on the same map (class cost): the
                  project's tuned kernels doing the same lookups with more arithmetic per hit
The gate: the call's wall time (both forms) is below the host route's on every map. Exits non-zero when it is missed.

    python tools/map_score_timing.py [OUT_DIR = profiles] [--repeats 10] [--legs pair,100k,1m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIAS = 1 << 20
OFFSETS27 = np.array([(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)], np.int64)


def med(x):
    return float(np.median(x))


def pack(c):
    c = c.astype(np.int64) + BIAS
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def host_score(coords, num, means, covs, res, pts, T, min_points, max_m2, score_scale):
    """the contract of fvh_*_score_* on all points at once (numpy, fp64) -> the struct's fields"""
    R, t = np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3]
    P = np.asarray(pts, np.float32).astype(np.float64)
    q = (((P[:, :1] * R[:, 0] + P[:, 1:2] * R[:, 1]) + P[:, 2:] * R[:, 2]) + t).astype(np.float32).astype(np.float64)
    c = np.floor(q / res - 0.5)
    used = np.isfinite(P).all(axis=1) & (np.abs(c) < BIAS - 4096).all(axis=1)
    q, c = q[used], c[used].astype(np.int64)
    keys = pack(np.asarray(coords))
    order = np.argsort(keys)
    skeys = keys[order]
    C = np.asarray(covs, np.float64).reshape(-1, 3, 3)
    cxx, cxy, cxz, cyy, cyz, czz = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    a00, a01, a02 = cyy * czz - cyz * cyz, cxz * cyz - cxy * czz, cxy * cyz - cxz * cyy
    a11, a12, a22 = cxx * czz - cxz * cxz, cxy * cxz - cxx * cyz, cxx * cyy - cxy * cxy
    det = (cxx * a00 + cxy * a01) + cxz * a02
    mu = np.asarray(means, np.float64)
    eligible = np.asarray(num) >= min_points if min_points > 1 else np.ones(len(keys), bool)
    best = np.full(len(q), np.inf)
    found = np.zeros(len(q), np.int64)
    own = np.zeros(len(q), bool)
    all_sum = np.zeros(len(q))
    for o, off in enumerate(OFFSETS27):
        k = pack(c + off)
        i = np.minimum(np.searchsorted(skeys, k), max(len(skeys) - 1, 0))
        rows = order[i] if len(skeys) else np.zeros(len(q), np.int64)
        hit = (skeys[i] == k) & eligible[rows] if len(skeys) else np.zeros(len(q), bool)
        r = rows[hit]
        d = q[hit] - mu[r]
        with np.errstate(all="ignore"):
            qq = (((d[:, 0] * d[:, 0]) * a00[r] + (d[:, 1] * d[:, 1]) * a11[r]) + (d[:, 2] * d[:, 2]) * a22[r]) + 2.0 * ((((d[:, 0] * d[:, 1]) * a01[r]) + ((d[:, 0] * d[:, 2]) * a02[r])) + ((d[:, 1] * d[:, 2]) * a12[r]))
            m2 = np.where((det[r] > 0.0) & np.isfinite(det[r]) & np.isfinite(qq), np.maximum(qq / det[r], 0.0), np.inf)
        found[hit] += 1
        if tuple(off) == (0, 0, 0):
            own[hit] = True
        idx = np.flatnonzero(hit)
        better = m2 < best[idx]
        best[idx[better]] = m2[better]
        all_sum[idx] += np.where(np.isfinite(m2), np.exp((-0.5 * score_scale) * m2), 0.0)
    near = found > 0
    explained = near & np.isfinite(best) & (best <= max_m2)
    return dict(n_points=int(len(P)), n_used=int(used.sum()), n_in_voxel=int(own.sum()), n_near=int(near.sum()), n_explained=int(explained.sum()), sum_best_m2=float(best[explained].sum()),
                sum_score_max=float(np.where(np.isfinite(best[near]), np.exp((-0.5 * score_scale) * best[near]), 0.0).sum()), sum_score_all=float(all_sum.sum()))


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
    res, max_m2, scale, min_points = 0.5, 9.0, 1.0, 1

    def handle(search=capi.DIRECT27):
        h = capi.VGICPMapCore(0)
        h.set_resolution(res); h.set_neighbor_search_method(search); h.profile_enable(True)
        return h

    reg = handle(capi.DIRECT7)
    reg.set_target_cloud(tgt); reg.find_target_neighbors(20); reg.calculate_target_covariances(); reg.create_target_voxelmap()
    reg.set_source_cloud(scan); reg.find_source_neighbors(20); reg.calculate_source_covariances()
    cov_t, cov_s = reg.get_covariances("target").astype(np.float64), reg.get_covariances("source").astype(np.float64)
    T = reg.align()["T"].copy()
    reg.close()
    flat = np.array([[0.01, 0.0, 0.0], [0.0, 0.01, 0.0], [0.0, 0.0, 0.01]])
    none3, none33 = np.zeros((0, 3), np.float32), np.zeros((0, 3, 3))
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "pose": T.tolist(), "resolution": res, "neighbors": "DIRECT27", "max_m2": max_m2, "score_scale": scale,
           "scan_points": int(len(scan)), "legs": {}}
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
        c.set_source_cloud(scan); c.set_source_covariances(cov_s)

        def timed(classes, fn):
            c.synchronize(); c.profile_reset(); sync()
            t0 = time.perf_counter()
            ret = fn()
            c.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            return [c.profile_get(k)[0] for k in classes], wall, ret

        def host_route():
            coords, num, means, covs = c.get_voxelmap()
            return host_score(coords, num, means, covs, res, scan, T, min_points, max_m2, scale)

        kw = dict(neighbors=capi.DIRECT27, min_points=min_points, max_m2=max_m2, score_scale=scale)
        W = 2
        dev, wall, dev_pp, wall_pp, hr, uc, ce = ([] for _ in range(7))
        got = host = None
        for i in range(W + args.repeats):
            (d,), w, got = timed(("map_score",), lambda: c.map_score(T, **kw))
            (d2,), w2, _ = timed(("map_score",), lambda: c.map_score(T, per_point=True, **kw))
            c.map_insert_cloud(none3, none33)  # (an insert -- here of nothing -- is what invalidates the host copy of the map between two scans)
            _, w_h, host = timed((), host_route)
            (d_u,), _, _ = timed(("cost",), lambda: c.update_correspondences(T))
            (d_e,), _, _ = timed(("cost",), lambda: c.compute_error(T, derivatives=False))
            if i >= W:
                dev.append(d); wall.append(w); dev_pp.append(d2); wall_pp.append(w2); hr.append(w_h); uc.append(d_u); ce.append(d_e)
        counts = ("n_points", "n_used", "n_in_voxel", "n_near", "n_explained")
        row = dict(map_points=int(n_points), voxels=c.map_info()["num_voxels"], capacity=c.map_info()["capacity"], **{k: got[k] for k in counts},
                   overlap=got["overlap"], nvtl=got["nvtl"], tp=got["tp"], host_route_matches_device=bool(all(got[k] == host[k] for k in counts)),
                   host_route_max_rel_sum_diff=max(abs(got[k] - host[k]) / max(abs(host[k]), 1e-300) for k in ("sum_best_m2", "sum_score_max", "sum_score_all")),
                   score_device_ms=med(dev), call_wall_ms=med(wall), per_point_call_wall_ms=med(wall_pp), host_route_wall_ms=med(hr),
                   update_correspondences_device_ms=med(uc), compute_error_device_ms=med(ce))
        row["per_point_score_device_ms"] = med(dev_pp)
        row["score_device_over_find_plus_error_device"] = row["score_device_ms"] / (row["update_correspondences_device_ms"] + row["compute_error_device_ms"])
        row["host_route_over_call_wall"] = row["host_route_wall_ms"] / row["call_wall_ms"]
        row["gate_call_wall_below_host_route_wall"] = bool(row["call_wall_ms"] < row["host_route_wall_ms"] and row["per_point_call_wall_ms"] < row["host_route_wall_ms"])
        print("%-5s %d voxels, %d points: score %.3f ms device, call %.3f ms wall (per point: %.3f) | host route %.1f ms wall (x%.1f) | update_correspondences %.3f + compute_error %.3f "
              "device (ratio %.2f) | overlap %.3f nvtl %.3f tp %.3f, host scorer agrees: %s" % (leg, row["voxels"], got["n_points"], row["score_device_ms"], row["call_wall_ms"], row["per_point_call_wall_ms"],
                                                                                                 row["host_route_wall_ms"], row["host_route_over_call_wall"], row["update_correspondences_device_ms"],
                                                                                                 row["compute_error_device_ms"], row["score_device_over_find_plus_error_device"], got["overlap"], got["nvtl"],
                                                                                                 got["tp"], row["host_route_matches_device"]), flush=True)
        if not row["gate_call_wall_below_host_route_wall"]:
            failed.append(leg)
        out["legs"][leg] = row
        c.close()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "map_score_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    if failed:
        print("GATE FAILED: the call's wall time is not below the host route's on: %s" % ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    main()
