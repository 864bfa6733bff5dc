"""Voxelized GICP (setVoxelResolution) next to exact GICP in the same run, on the same handle, clouds, covariances and settings.

  python scripts/vgicp_bench.py [--workloads c3,c5] [--resolutions 0.5,1.0,2.0] [--neighbors 1,7,27] [--reps 30] [--out profiles/vgicp_bench.json]
one JSON line on stdout (and in --out).  Its us_per_pass are HIP-event times.  Kernel times from the profiler: a run of its own under
  rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/vgicp_bench.py --reps 5
(k_vgicp_pass against k_gicp_pass in its kernel table, which belongs next to the JSON as profiles/vgicp_kernel_stats.csv; its averages
include the few launches enqueued ahead of the solver's `done`, which return at once).

Workloads: c3 100k -> 500k scan-to-submap (bench.py's), c5 250k -> 2M OS1-128; DLO's scan-to-map settings (32 iterations at most,
transformation epsilon 0.01, the workload's correspondence gate - which the voxelized mode does not consult).  Per mode:
  us_per_pass        device time of the pass kernel from HIP events attached to its dispatches (ngicp_set_profiling), a run apart from
                     the timed ones (the events cost stream time)
  us_per_iteration   device time of the loop (the engine's own 100 MHz stamps, first pass to the solver's `done`) / passes
  align_ms           host-to-host, median and p10..p90 of --reps alignments after 3 warm-ups; the two modes alternate inside one loop
  map_build_ms       device time of the voxel-map build (ngicp_stats.voxelmap_ms), median of --reps rebuilds
  iterations, trials, the final pose's distance from the ground truth (m, rad), the share of source points with a correspondence.
--neighbors: the neighbourhoods (setNeighborSearchMethod) to run at every resolution, DIRECT1 always among them.  DIRECT1's figures
stay where they were (resolutions[r]); the others are under resolutions[r]["neighbors"][K] with the same device figures plus
us_per_pass_vs_direct1, the per-pass time relative to DIRECT1 of the same run, resolution and handle - the figure of interest - and
valid_fraction there counts pairs per point.  Changing the neighbourhood keeps the voxel map, so no build is timed for them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DLO = dict(setMaximumIterations=32, setTransformationEpsilon=0.01)


def _workload(clouds, name):
    if name == "c3":
        return clouds.scan_to_submap(100_000, 5)
    if name == "c5":
        return clouds.scan_to_submap(250_000, 8, shape="os1")
    if name == "s20k":
        return clouds.scan_to_submap(20_000, 3)
    raise SystemExit(f"unknown workload {name}")


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}


def _device_figures(g, clouds, w):
    """One profiled alignment (pass kernel events) and one plain one (loop time)."""
    g.setProfiling(1)
    g.align(w.guess)
    s = g.stats()
    us_pass = 1e3 * s["pass_ms_total"] / max(1, s["passes_timed"])
    g.setProfiling(0)
    g.align(w.guess)
    s = g.stats()
    dt, dr = clouds.pose_error(g.getFinalTransformation(), w.gt)
    return {"us_per_pass": us_pass, "us_per_iteration": 1e3 * s["loop_ms"] / max(1, s["passes"]), "loop_ms": s["loop_ms"], "passes": s["passes"],
            "iterations": g.nr_iterations_ + 1, "lm_trials": s["lm_trials"], "converged": bool(g.converged_), "valid_fraction": s["valid_fraction"],
            "error_vs_ground_truth_m": dt, "error_vs_ground_truth_rad": dr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c5")
    ap.add_argument("--resolutions", default="0.5,1.0,2.0")
    ap.add_argument("--neighbors", default="1,7,27")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    out = {"metric": "vgicp_vs_exact_gicp", "device": torch.cuda.get_device_name(0), "settings": DLO, "reps": a.reps, "workloads": {}}
    for name in a.workloads.split(","):
        w = _workload(clouds, name)
        g = ng.NanoGICP()
        g.setCorrespondenceRandomness(20)
        g.setMaxCorrespondenceDistance(w.max_corr_dist)
        for k, v in DLO.items():
            getattr(g, k)(v)
        g.setInputTarget(w.target)
        g.setInputSource(w.source)
        g.calculateSourceCovariances()
        g.setTargetCovariances(ng.keyframe_covariances(w.target, w.keyframe_sizes, 20))  # per keyframe, as DLO supplies them
        dt0, dr0 = clouds.pose_error(w.guess, w.gt)
        res = {"source_points": int(len(w.source)), "target_points": int(len(w.target)), "guess_error_m": dt0, "guess_error_rad": dr0, "resolutions": {}}
        for _ in range(3):
            g.align(w.guess)
        res["exact"] = _device_figures(g, clouds, w)
        for r in [float(v) for v in a.resolutions.split(",")]:
            builds = []
            for _ in range(a.reps):
                g.setVoxelResolution(0)
                g.setVoxelResolution(r)  # drops the map: the next use rebuilds it
                n_vox = g.getVoxelMapSize()
                builds.append(g.stats()["voxelmap_ms"])
            for _ in range(3):
                g.align(w.guess)
            v = _device_figures(g, clouds, w)
            tv, te = [], []
            for _ in range(a.reps):  # the two modes alternate; switching drops the map, so it is rebuilt outside the timed call
                g.setVoxelResolution(r)
                g.getVoxelMapSize()
                t0 = time.perf_counter()
                g.align(w.guess)
                t1 = time.perf_counter()
                g.setVoxelResolution(0)
                t2 = time.perf_counter()
                g.align(w.guess)
                t3 = time.perf_counter()
                tv.append((t1 - t0) * 1e3)
                te.append((t3 - t2) * 1e3)
            v.update(voxels=int(n_vox), map_build_ms=float(np.median(builds)), align=_summ(tv), exact_align_same_loop=_summ(te))
            v["neighbors"] = {}
            g.setVoxelResolution(r)
            for K in [int(k) for k in a.neighbors.split(",") if int(k) != 1]:
                g.setNeighborSearchMethod(K)
                for _ in range(3):
                    g.align(w.guess)
                vk = _device_figures(g, clouds, w)
                tk = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    g.align(w.guess)
                    tk.append((time.perf_counter() - t0) * 1e3)
                vk.update(align=_summ(tk), us_per_pass_vs_direct1=vk["us_per_pass"] / v["us_per_pass"] if v["us_per_pass"] else None)
                v["neighbors"][str(K)] = vk
            g.setNeighborSearchMethod(1)
            g.setVoxelResolution(0)
            res["resolutions"][str(r)] = v
            print(name, r, json.dumps(v), file=sys.stderr, flush=True)
        print(name, "exact", json.dumps(res["exact"]), file=sys.stderr, flush=True)
        g.close()
        out["workloads"][name] = res
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
