"""The voxel fitness (voxelFitnessBatch, k_voxel_fitness<K> + k_voxel_fitness_final) against the scores a user has
without it, all in one process, warmed, the compared routes alternating repetition by repetition.

  python scripts/voxel_fitness_bench.py [--sizes 20k,100k] [--neighbors 1,7,27] [--lanes 1,8,64] [--reps 15] [--warmup 3]
                                        [--out profiles/voxel_fitness_bench.json]
one JSON line on stdout (and in --out).

Per size (20k -> 60k: clouds.scan_to_submap(20_000, 3); 100k -> 500k: clouds.scan_to_submap(100_000, 5)), at 1 m, per neighbourhood K and
per lane count B, the B poses being small motions around the pose align() ends at:
  voxel_fitness_target     voxelFitnessBatch(Ts) on a handle with the target set (the map built from it before anything is timed)
  voxel_fitness_rolling    the same call on a handle whose map is a rolling map holding the same target, no target set
  exact_fitness            fitnessBatch(Ts) on the same pair: the exact 1-NN score, which needs the target cloud and its index
  robust_terms_route       what a rolling-map user has today: robust_terms(T) - two downloads of n x K doubles under the correspondences of
                           the last linearisation - and a host reduction, per pose.  Measured for ONE pose (its own repetitions) and
                           reported per pose; the B-pose figure is B times that, marked as scaled.
host_ms: time.perf_counter around the call, host to host.  kernel_ms: the engine's event time around the two kernels of the call
(voxelFitnessKernelMs()).  Medians with p10 .. p90 over --reps repetitions after --warmup discarded ones.

bytes_per_point_pose: the algorithmic traffic of one point under one pose, from the shapes: 64 B of point and covariance, per slot a
16 B probe of the table, per occupied slot an 80 B record; the occupied slots per point are counted at the final pose
(voxel_correspondences() after a linearize).  effective_GBps = that x n x B / kernel time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 1.0
SIZES = {"20k": (20_000, 3), "100k": (100_000, 5)}


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _host_reduce(s):
    """the rolling-map user's reduction of robust_terms' s (n, K): per point the smallest term of its slots, the mean over the matched"""
    has = s >= 0
    best = np.where(has, s, np.inf).min(axis=1)
    ok = has.any(axis=1)
    return float(best[ok].mean()) if ok.any() else float(np.finfo(np.float64).max), int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20k,100k")
    ap.add_argument("--neighbors", default="1,7,27")
    ap.add_argument("--lanes", default="1,8,64")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_fitness_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_fitness_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    lanes = [int(x) for x in a.lanes.split(",")]
    out = {"metric": "voxel_fitness_vs_exact_fitness_and_robust_terms", "device": torch.cuda.get_device_name(0), "resolution": RES, "reps": a.reps,
           "warmup": a.warmup, "sizes": {}}
    rng = np.random.default_rng(7)
    for size in a.sizes.split(","):
        n_src, n_kf = SIZES[size]
        w = clouds.scan_to_submap(n_src, n_kf)
        gt, gr, mapper = ng.NanoGICP(), ng.NanoGICP(), ng.NanoGICP()
        for g in (gt, gr, mapper):
            g.setVoxelResolution(RES)
        gt.setInputSource(w.source); gt.setInputTarget(w.target)
        mapper.setVoxelRolling(True); gr.setVoxelRolling(True)
        mapper.setInputSource(w.target)
        mapper.insertIntoVoxelMap(mapper, np.eye(4, dtype=np.float32))
        gr.setRollingVoxelMap(*mapper.rollingVoxelMap(), mapper.voxelRollingStats()["inserts"])  # (no target on this handle)
        mapper.close()
        gr.setInputSource(w.source)
        per_size = {"n_src": int(len(w.source)), "n_tgt": int(len(w.target)), "neighbors": {}}
        for K in [int(x) for x in a.neighbors.split(",")]:
            for g in (gt, gr):
                g.setNeighborSearchMethod(K)
                g.align(w.guess)  # (the map, the covariances and - for robust_terms - the correspondences exist from here on)
            T0 = gt.getFinalTransformation().copy()
            Ts = np.stack([(T0 @ clouds.make_pose(tuple(rng.normal(0, 0.02, 3)), tuple(rng.normal(0, 0.2, 3)))).astype(np.float32) for _ in range(max(lanes))])
            Ts[0] = T0
            gt.linearize(T0.astype(np.float64))
            cn = gt.voxel_correspondences()
            hits = float((cn >= 0).sum(axis=1).mean())
            bytes_pp = 64.0 + 16.0 * K + 80.0 * hits
            cellK = {"voxels": int(gt.getVoxelMapSize()), "rolling_voxels": int(gr.getVoxelMapSize()), "occupied_slots_per_point": hits, "bytes_per_point_pose": bytes_pp, "lanes": {}}
            # the robust_terms route, one pose
            rt = []
            for rep in range(a.warmup + a.reps):
                t, _ = _timed(lambda: _host_reduce(gr.robust_terms(T0)[0]))
                if rep >= a.warmup:
                    rt.append(t)
            cellK["robust_terms_route_per_pose"] = {"host_ms": _summ(rt)}
            for B in lanes:
                rec = {}

                def note(name, host, kernel=None):
                    r = rec.setdefault(name, {"host_ms": [], "kernel_ms": []})
                    r["host_ms"].append(host)
                    if kernel is not None:
                        r["kernel_ms"].append(kernel)

                for rep in range(a.warmup + a.reps):
                    routes = [("voxel_fitness_target", gt, lambda: gt.voxelFitnessBatch(Ts[:B])), ("voxel_fitness_rolling", gr, lambda: gr.voxelFitnessBatch(Ts[:B])),
                              ("exact_fitness", None, lambda: gt.fitnessBatch(Ts[:B]))]
                    for name, h, fn in (routes if rep % 2 == 0 else routes[::-1]):
                        t, got = _timed(fn)
                        if rep >= a.warmup:
                            note(name, t, h.voxelFitnessKernelMs() if h is not None else None)
                cell = {name: {k: _summ(v) for k, v in r.items() if v} for name, r in rec.items()}
                k_ms = cell["voxel_fitness_target"]["kernel_ms"]["median_ms"]
                cell["effective_GBps"] = bytes_pp * len(w.source) * B / (k_ms * 1e-3) / 1e9
                cell["robust_terms_route_scaled"] = {"host_ms_median": B * cellK["robust_terms_route_per_pose"]["host_ms"]["median_ms"], "scaled_from_one_pose": True}
                cell["exact_over_voxel_host"] = cell["exact_fitness"]["host_ms"]["median_ms"] / cell["voxel_fitness_target"]["host_ms"]["median_ms"]
                cell["robust_route_over_voxel_host"] = cell["robust_terms_route_scaled"]["host_ms_median"] / cell["voxel_fitness_rolling"]["host_ms"]["median_ms"]
                cellK["lanes"][str(B)] = cell
                print(size, K, B, json.dumps(cell), file=sys.stderr, flush=True)
            per_size["neighbors"][str(K)] = cellK
        out["sizes"][size] = per_size
        gt.close(); gr.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
