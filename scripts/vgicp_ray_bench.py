"""Clearing the rolling voxel map along a scan's rays (clearVoxelMapAlongRays) timed against the insert of the same scan -
the per-frame cost a clear is added to - in the same process, the two alternating.

  python scripts/vgicp_ray_bench.py [--cases filtered:0.5,unfiltered:0.5,unfiltered:0.2] [--map-frames 20] [--reps 30] [--warmup 5] [--points 100000]
                                    [--out profiles/vgicp_ray_bench.json]
one JSON line on stdout (and in --out).

Workload: the synthetic drive of scripts/vgicp_rolling_bench.py through clouds.make_scene(): one VLP-16 scan of --points rays per frame,
0.32 m and 1 degree of yaw apart.  `filtered` passes every scan through the engine's scan filter first (preprocessScan, VoxelGrid leaf
0.5 m), `unfiltered` keeps all --points rays; behind the colon the map's resolution in metres (the room is 40 x 30 x 6 m, so a finer
resolution is what makes the map large).  --map-frames scans are inserted at their ground-truth poses; the next scan of the drive is
the one that is cleared with and inserted, at its ground-truth pose, with the source covariances already computed (in a frame loop the
alignment has made them).  Before every timed call the map is restored to the same state (setRollingVoxelMap, untimed), so every
repetition does the same work.

Per case, host to host (time.perf_counter around calls that end in a device synchronisation), medians and p10..p90 over --reps:
  clear_ms       one clearVoxelMapAlongRays with the defaults (counts, flags, scan, compaction; the copies back and the table rebuild
                 are left in the stream, where the next call on the handle waits for them: clear_synced_ms adds that wait)
  clear_dry_ms   the same with dry_run (counts only)
  insert_ms      insertIntoVoxelMap of the same scan into the same map
  kernel_ms      the device event time of the counting kernel; insert_device_ms the insert's
and once: the numpy model (tests/_vgicp_ray_model.py) on the same input, checked equal; the share of counted steps that land in occupied
cells; counted steps per ray (mean, percentiles, the longest) and what a wave of 64 consecutive rays spends waiting for its longest ray,
estimated in the scan's own order and in ascending end cell (the engine walks the rays in its cell-sorted order, which neither is).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEAF = 0.5


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _wave_efficiency(steps, order):
    """useful lane-steps over issued lane-steps when 64 consecutive rays of `order` share a wave that runs as long as its longest ray"""
    s = steps[order]
    pad = (-len(s)) % 64
    w = np.r_[s, np.zeros(pad, s.dtype)].reshape(-1, 64)
    issued = float((w.max(axis=1) * 64).sum())
    return float(s.sum()) / issued if issued else 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="filtered:0.5,unfiltered:0.5,unfiltered:0.2")
    ap.add_argument("--map-frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgicp_ray_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_ray_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    import _vgicp_ray_model as ray
    from _vgicp_rolling_model import transform_pcl_f32
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    sc = clouds.make_scene()
    cols = a.points // 16
    n_frames = a.map_frames + 1
    gts = [clouds.make_pose((-0.16 * (n_frames - 1) + 0.32 * i, 0.0, 0.0), (0.0, 0.0, 1.0 * i - 0.5 * n_frames)).astype(np.float32) for i in range(n_frames)]
    raw = [clouds.vlp16(sc, p.astype(np.float64), 400 + i, cols=cols) for i, p in enumerate(gts)]
    out = {"metric": "ray_clear_vs_insert", "device": torch.cuda.get_device_name(0), "map_frames": a.map_frames, "reps": a.reps, "warmup": a.warmup,
           "rays_per_raw_scan": int(len(raw[0])), "filter_leaf": LEAF, "options": dict(ng.RayClearOptions.DEFAULTS), "cases": {}}
    for spec in a.cases.split(","):
        case, res = spec.split(":")[0], float(spec.split(":")[1])
        if case == "filtered":
            pre = ng.NanoGICP()
            scans = [np.ascontiguousarray(pre.preprocessScan(s, voxel_res=LEAF)[:, :3], np.float32) for s in raw]
            pre.close()
        else:
            scans = raw
        g = ng.NanoGICP()
        g.setCorrespondenceRandomness(20)
        g.setVoxelResolution(res)
        g.setVoxelRolling(True)
        for s, T in zip(scans[:-1], gts[:-1]):
            g.setInputSource(s)
            g.insertIntoVoxelMap(g, T)
        state = (*g.rollingVoxelMap(), g.voxelRollingStats()["inserts"])
        scan, T = scans[-1], gts[-1]
        g.setInputSource(scan)
        g.calculateSourceCovariances()
        rec = {k: [] for k in ("clear_ms", "clear_synced_ms", "clear_dry_ms", "insert_ms", "kernel_ms", "kernel_dry_ms", "insert_device_ms")}
        removed = None
        for i in range(a.warmup + a.reps):
            timed = i >= a.warmup
            for what in (("clear", "insert", "dry") if i % 2 == 0 else ("insert", "dry", "clear")):
                g.setRollingVoxelMap(*state)
                g.getVoxelMapSize()
                torch.cuda.synchronize()
                if what == "insert":
                    t, _ = _timed(lambda: g.insertIntoVoxelMap(g, T))
                    dev = g.voxelRollingStats()["last_insert_ms"]
                    if timed:
                        rec["insert_ms"].append(t); rec["insert_device_ms"].append(dev)
                else:
                    t0 = time.perf_counter()
                    r = g.clearVoxelMapAlongRays(g, T, dry_run=int(what == "dry"))
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if what == "clear":
                        removed = r
                    if timed and what == "clear":
                        rec["clear_ms"].append((t1 - t0) * 1e3); rec["clear_synced_ms"].append((t2 - t0) * 1e3); rec["kernel_ms"].append(r["kernel_ms"])
                    elif timed:
                        rec["clear_dry_ms"].append((t1 - t0) * 1e3); rec["kernel_dry_ms"].append(r["kernel_ms"])
        cell = {k: _summ(v) for k, v in rec.items()}
        # the numpy model on the same input, once, and checked
        ijk, S, _, cnt, st = state[:5]
        mean = S / cnt.astype(np.float64)[:, None]
        t_model, want = _timed(lambda: ray.ray_clear(ijk, mean, st, res, scan, T))
        g.setRollingVoxelMap(*state)
        got = g.clearVoxelMapAlongRays(g, T)
        miss, hit = g.voxelMapRayCounts()
        equal = bool(np.array_equal(miss, want["miss"]) and np.array_equal(hit, want["hit"]) and all(got[k] == want[k] for k in ("steps", "occupied", "misses", "n_removed")))
        rays = ray.Rays(T[:3, 3], transform_pcl_f32(T, scan), res)
        o = ng.RayClearOptions.DEFAULTS
        per_ray = np.maximum(0, np.minimum(rays.N - 1 - o["back_cells"], o["max_steps"]) - o["near_cells"] + 1)
        cell.update(resolution=res, points=int(len(scan)), map_voxels=int(len(ijk)), removed=int(removed["n_removed"]), counted_steps=int(got["steps"]), occupied_steps=int(got["occupied"]),
                    misses=int(got["misses"]), occupied_share=got["occupied"] / max(1, got["steps"]), numpy_model_ms=t_model, engine_equals_model=equal,
                    clear_over_insert=cell["clear_ms"]["median_ms"] / cell["insert_ms"]["median_ms"],
                    steps_per_ray={"mean": float(per_ray.mean()), "p10": float(np.percentile(per_ray, 10)), "median": float(np.median(per_ray)),
                                   "p90": float(np.percentile(per_ray, 90)), "max": int(per_ray.max())},
                    wave_efficiency_estimate={"scan_order": _wave_efficiency(per_ray, np.arange(len(per_ray))),
                                              "ascending_end_cell": _wave_efficiency(per_ray, np.argsort(ray.pack(rays.c1), kind="stable"))},
                    counted_steps_per_kernel_us=got["steps"] / max(1e-9, cell["kernel_ms"]["median_ms"] * 1e3))
        out["cases"][spec] = cell
        print(spec, json.dumps(cell), file=sys.stderr, flush=True)
        g.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
