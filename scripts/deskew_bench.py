"""Timing of the motion deskew (include/ngicp.h "motion deskew") inside the scan preprocessing.

  python scripts/deskew_bench.py [--out PATH]   one JSON line on stdout, the same object in profiles/deskew_bench.json (or PATH)
Kernel times: run it once under  rocprofv3 --kernel-trace --stats -- python scripts/deskew_bench.py --once  (a run of its own).

One 100 000-point VLP-16 shaped sweep (32-byte records, a float32 time per point in the record's padding), DLO's filter settings
(removeNaN, crop 1.0 m, voxel 0.25 m), a constant-twist trajectory of M = 2 and M = 40 poses.  Host-to-host times of whole calls (each
ends in the download of the filtered cloud, so in a device synchronise), all routes inside every repetition (the device routes in
rotating order after one untimed call, the host routes after them), median and p10-p90 over REPS repetitions after WARMUP:
  plain              preprocessScan of the raw sweep: what the engine did before, no deskew at all
  deskewed           preprocessScanDeskewed, time inside the record (nothing more is uploaded than for `plain`)
  deskewed_times     preprocessScanDeskewed, times in a float32 array of their own (400 KB more to upload)
  host_then_plain    the deskew in numpy on the host (float64, vectorised, ONE thread: clouds.trajectory_poses + two einsum), then
                     preprocessScan of the result; `host_deskew` is its numpy part alone.  A C++ loop would be faster than numpy;
                     it was not measured.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 100_000
CROP, LEAF = 1.0, 0.25  # cfg/params.yaml:28-33 of the reference
POSES = (2, 40)
REPS, WARMUP = 30, 5
SWEEP_S = 0.1
TWIST_V, TWIST_W = (5.0, 0.0, 0.0), (0.0, 0.0, 1.0)  # m/s, rad/s


def twist_trajectory(clouds, M):
    """M poses of a constant yaw rate and forward speed, equal steps over the sweep."""
    tau = np.linspace(0.0, SWEEP_S, M)
    poses = np.tile(np.eye(4), (M, 1, 1))
    for k, t in enumerate(tau):
        yaw = TWIST_W[2] * t
        poses[k] = clouds.make_pose((TWIST_V[0] * np.sin(yaw) / TWIST_W[2], TWIST_V[0] * (1 - np.cos(yaw)) / TWIST_W[2], 0.0), (0.0, 0.0, np.degrees(yaw)))
    return tau, poses


def host_deskew(clouds, xyzi, s, tau, poses, T_ref):
    R, t = clouds.trajectory_poses(s, tau, poses)
    world = np.einsum("nij,nj->ni", R, xyzi[:, :3].astype(np.float64)) + t
    out = xyzi.copy()
    out[:, :3] = (world - T_ref[:3, 3]) @ T_ref[:3, :3]
    return out


def summary(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90))}


def case(ng, clouds, M, reps, warmup):
    scan = clouds.scan_to_scan(N).source
    tau, poses = twist_trajectory(clouds, M)
    T_ref = poses[-1]
    s = clouds.sweep_times(len(scan), sweep_s=SWEEP_S)
    raw = clouds.to_xyzi(clouds.skew_scan(scan, s, tau, poses, T_ref))
    s32 = s.astype(np.float32)
    raw[:, 5] = s32
    g = ng.NanoGICP()
    device_routes = {
        "plain": lambda: g.preprocessScan(raw, True, CROP, LEAF, intensity_col=4),
        "deskewed": lambda: g.preprocessScanDeskewed(raw, 5, tau, poses, T_ref, remove_nan=True, crop_size=CROP, voxel_res=LEAF, intensity_col=4),
        "deskewed_times": lambda: g.preprocessScanDeskewed(raw, s32, tau, poses, T_ref, remove_nan=True, crop_size=CROP, voxel_res=LEAF, intensity_col=4),
    }
    host_routes = {"host_deskew": lambda: host_deskew(clouds, raw, s32.astype(np.float64), tau, poses, T_ref)}
    host_routes["host_then_plain"] = lambda: g.preprocessScan(host_routes["host_deskew"](), True, CROP, LEAF, intensity_col=4)
    ms = {k: [] for k in (*device_routes, *host_routes)}
    rows = {}

    def timed(name, fn, keep):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        rows[name] = len(out)
        if keep:
            ms[name].append(dt)

    names = list(device_routes)
    for rep in range(warmup + reps):
        # The host routes leave the device idle for ~20 ms; the call after such a gap is slower whichever route it is.  So an untimed
        # call comes first, and the three device routes follow in an order that rotates with the repetition.
        device_routes["plain"]()
        for j in range(len(names)):
            name = names[(rep + j) % len(names)]
            timed(name, device_routes[name], rep >= warmup)
        for name, fn in host_routes.items():
            timed(name, fn, rep >= warmup)
    # the device route and the host route see the same scan: the restored cloud is the undistorted one to float32 rounding
    restored = g.deskewCloud(raw, 5, tau, poses, T_ref)
    g.close()
    res = {name: summary(v) for name, v in ms.items()}
    res.update({"poses": M, "points": N, "repetitions": reps, "warmup": warmup, "rows_out": rows,
                "max_abs_restored_minus_undistorted_m": float(np.abs(restored - scan).max()),
                "max_abs_distortion_m": float(np.abs(raw[:, :3] - scan).max())})
    res["deskewed_minus_plain_median_ms"] = res["deskewed"]["median_ms"] - res["plain"]["median_ms"]
    res["deskewed_times_minus_plain_median_ms"] = res["deskewed_times"]["median_ms"] - res["plain"]["median_ms"]
    return res


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("deskew_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    once = "--once" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "deskew_bench.json")
    out = {"metric": "deskew_preprocess", "device": torch.cuda.get_device_name(0), "crop": CROP, "leaf": LEAF, "sweep_s": SWEEP_S,
           "twist": {"v_mps": TWIST_V, "w_radps": TWIST_W}, "host_label": "numpy float64, vectorised, one thread; not a C++ loop"}
    for M in POSES:
        out[f"M{M}"] = case(ng, clouds, M, 2 if once else REPS, 1 if once else WARMUP)
    line = json.dumps(out)
    if not once:
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
