"""The gated insert of the rolling voxel map (insertIntoVoxelMapGated) timed against the plain insert of the same scan - the
difference is the price of the gate - and against the host route it replaces, the three alternating in one process.

  python scripts/vgicp_gate_bench.py [--neighbors 1,7,27] [--resolution 0.5] [--gate 0.5] [--map-frames 20] [--reps 30] [--warmup 5] [--points 100000]
                                     [--out profiles/vgicp_gate_bench.json]
one JSON line on stdout (and in --out).

Workload: the synthetic drive of scripts/vgicp_ray_bench.py through clouds.make_scene(): one VLP-16 scan of --points rays per frame, 0.32 m
and 1 degree of yaw apart.  --map-frames scans, each passed through the engine's scan filter (preprocessScan, VoxelGrid leaf 0.5 m), are
inserted at their ground-truth poses; the next scan of the drive is the one that is inserted, at its ground-truth pose, with the source
covariances already computed (in a frame loop the alignment has made them): `filtered` after the same filter, `unfiltered` with all its
rays, both into the same map.  Before every timed call the map is restored to the same state (setRollingVoxelMap, untimed) and the device
is idle, so every repetition does the same work.

Per case and neighbourhood, host to host (time.perf_counter around calls that end in a device synchronisation), medians and p10..p90 over
--reps, the routes in rotating order:
  gated_ms       (a) one insertIntoVoxelMapGated with the defaults and --gate
  plain_ms       (b) insertIntoVoxelMap of the same scan
  host_route_ms  (c) the route the documents used to describe: voxel_fitness_points, the covariances read back, a host mask, the subset
                 uploaded as a source of its own on a second handle (setInputSource, setSourceCovariances) and inserted from there
  gated_device_ms / plain_device_ms   the device event times the two calls report
and once: the maps of (a) and (c) compared (they must be equal), the classes' counts.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEAF = 0.5


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--neighbors", default="1,7,27")
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--gate", type=float, default=0.5)
    ap.add_argument("--map-frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgicp_gate_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_gate_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    sc = clouds.make_scene()
    cols = a.points // 16
    n_frames = a.map_frames + 1
    gts = [clouds.make_pose((-0.16 * (n_frames - 1) + 0.32 * i, 0.0, 0.0), (0.0, 0.0, 1.0 * i - 0.5 * n_frames)).astype(np.float32) for i in range(n_frames)]
    raw = [clouds.vlp16(sc, p.astype(np.float64), 400 + i, cols=cols) for i, p in enumerate(gts)]
    pre = ng.NanoGICP()
    filtered = [np.ascontiguousarray(pre.preprocessScan(s, voxel_res=LEAF)[:, :3], np.float32) for s in raw]
    pre.close()
    T = gts[-1]
    out = {"metric": "gated_insert_vs_plain_insert_vs_host_route", "device": torch.cuda.get_device_name(0), "map_frames": a.map_frames, "reps": a.reps, "warmup": a.warmup,
           "resolution": a.resolution, "max_mahalanobis": a.gate, "filter_leaf": LEAF, "options": dict(ng.GateOptions.DEFAULTS), "cases": {}}
    for K in [int(k) for k in a.neighbors.split(",")]:
        g, sub = ng.NanoGICP(), ng.NanoGICP()
        g.setCorrespondenceRandomness(20)
        g.setVoxelResolution(a.resolution)
        g.setNeighborSearchMethod(K)
        g.setVoxelRolling(True)
        for s, P in zip(filtered[:-1], gts[:-1]):
            g.setInputSource(s)
            g.insertIntoVoxelMap(g, P)
        state = (*g.rollingVoxelMap(), g.voxelRollingStats()["inserts"])
        for case, scan in (("filtered", filtered[-1]), ("unfiltered", np.ascontiguousarray(raw[-1][:, :3], np.float32))):
            g.setInputSource(scan)
            g.calculateSourceCovariances()

            def gated():
                return g.insertIntoVoxelMapGated(g, T, a.gate)

            def plain():
                return g.insertIntoVoxelMap(g, T)

            def host_route():
                m, _, v = g.voxel_fitness_points(T)
                keep = (v < 0) | (m <= a.gate)  # NEW (-1 / -1), UNJUDGED (+inf / -1), EXPLAINED
                covs = g.getSourceCovariances()
                sub.setInputSource(np.ascontiguousarray(scan[keep]), identity=0)
                sub.setSourceCovariances(covs[keep])
                return g.insertIntoVoxelMap(sub, T)

            routes = {"gated": gated, "plain": plain, "host_route": host_route}
            rec = {k: [] for k in ("gated_ms", "plain_ms", "host_route_ms", "gated_device_ms", "plain_device_ms")}
            names = list(routes)
            last = {}
            for i in range(a.warmup + a.reps):
                for what in names[i % 3:] + names[:i % 3]:
                    g.setRollingVoxelMap(*state)
                    g.getVoxelMapSize()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = routes[what]()
                    t = (time.perf_counter() - t0) * 1e3
                    last[what] = r
                    if i >= a.warmup:
                        rec[what + "_ms"].append(t)
                        if what == "gated":
                            rec["gated_device_ms"].append(r["kernel_ms"])
                        elif what == "plain":
                            rec["plain_device_ms"].append(g.voxelRollingStats()["last_insert_ms"])
            cell = {k: _summ(v) for k, v in rec.items()}
            # (a) and (c) leave the same map
            g.setRollingVoxelMap(*state)
            res_a = gated()
            map_a = g.rollingVoxelMap()
            g.setRollingVoxelMap(*state)
            host_route()
            equal = all(np.array_equal(x, y) for x, y in zip(map_a, g.rollingVoxelMap()))
            cell.update(neighbors=K, points=int(len(scan)), map_voxels=int(len(state[0])), n_class=res_a["n_class"], n_kept=int(res_a["n_kept"]),
                        gated_equals_host_route=bool(equal), gate_price_ms=cell["gated_ms"]["median_ms"] - cell["plain_ms"]["median_ms"],
                        host_route_over_gated=cell["host_route_ms"]["median_ms"] / cell["gated_ms"]["median_ms"])
            out["cases"][f"{case}:DIRECT{K}"] = cell
            print(case, K, json.dumps(cell), file=sys.stderr, flush=True)
        g.close(); sub.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
