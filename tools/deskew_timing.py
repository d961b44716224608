#!/usr/bin/env python
"""Times the device motion compensation (fvh_voxelgrid_deskew_device) on an MI355X and writes profiles/deskew_timing.json.
    python tools/deskew_timing.py [--reps 20] [--out profiles/deskew_timing.json]

Legs: the bundled 17k source, a simulated LiDAR frame (workloads.lidar_frame, ~118k points) and a 100k synthetic scene, each with
azimuth times, for K = 2 and K = 40 knots. Per leg and K:
  - device time of profile class "deskew" and wall time of deskew_device (device pointers in, count out), medians over the repetitions;
  - beside them, in the same process on the same cloud: the "compact" class (three passes) and the wall time of crop_range_device;
  - for scale only, not gated: the numpy twin of the tests on one core.
Gate: the deskew kernel's device time is at most the crop's "compact" device time on the same cloud -- one pass over the points against
three. A loss would point at a spill, uncoalesced time loads or a slow sincos path."""
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


def leg(name, pts, reps):
    import torch
    from fast_gicp_amd import capi
    from tests import deskew_ref as R
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    t = R.azimuth_times(pts)
    dev = torch.device("cuda", 0)
    d, dt = torch.from_numpy(pts).to(dev).contiguous(), torch.from_numpy(t).to(dev).contiguous()
    vg = capi.VoxelGrid(0)
    res = {"leg": name, "points": n, "knots": {}}

    def timed(call, cls):
        for _ in range(3):
            call()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e6)
        devt = []
        vg.profile_enable(True)
        for _ in range(reps):
            vg.profile_reset()
            call()
            devt.append(vg.profile_get(cls)[0] * 1e3)
        vg.profile_enable(False); vg.profile_reset()
        return med(wall), med(devt)

    crop_wall, crop_dev = timed(lambda: vg.crop_range_device(d.data_ptr(), n, 1e-3, 60.0 ** 2), "compact")
    res["crop"] = {"wall_us": crop_wall, "compact_device_us": crop_dev}
    for K in (2, 40):
        tau, T = R.random_trajectory(K, 7)
        wall, devt = timed(lambda: vg.deskew_device(d.data_ptr(), n, dt.data_ptr(), tau, T), "deskew")
        t0 = time.perf_counter()
        R.deskew(pts, t, tau, T)
        twin_ms = (time.perf_counter() - t0) * 1e3
        res["knots"][str(K)] = {"wall_us": wall, "deskew_device_us": devt, "bytes_moved": n * (16 + 4 + 12 + 16), "gb_per_s": n * 48 / (devt * 1e-6) / 1e9,
                                "numpy_twin_one_core_ms": twin_ms, "ratio_to_compact": devt / crop_dev, "passed": bool(devt <= crop_dev)}
    vg.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first: INTEGRATION.md, "Sharing a process with PyTorch")
    from fast_gicp_amd import capi, preprocess, workloads
    assert capi.device_count() >= 1, "no GPU visible"
    legs = [("bundled_source_17k", preprocess.bundled_pair(os.path.join(ROOT, "data"))[1]), ("lidar_frame", workloads.lidar_frame(3)), ("synthetic_100k", workloads.synthetic_scene(100000, 42))]
    out = {"device": capi.device_name(0) if hasattr(capi, "device_name") else "gfx950", "reps": a.reps, "legs": [leg(nm, p, a.reps) for nm, p in legs]}
    out["gate_passed"] = all(k["passed"] for l in out["legs"] for k in l["knots"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for l in out["legs"]:
        for K, k in l["knots"].items():
            print("%-20s n=%6d K=%2s deskew %6.1f us device, %7.1f us wall | crop: compact %6.1f us device, %7.1f us wall | twin %7.1f ms | gate %.2f: %s" % (
                l["leg"], l["points"], K, k["deskew_device_us"], k["wall_us"], l["crop"]["compact_device_us"], l["crop"]["wall_us"], k["numpy_twin_one_core_ms"], k["ratio_to_compact"], k["passed"]))
    print(json.dumps({"gate_passed": out["gate_passed"], "out": a.out}))
    return 0 if out["gate_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
