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

  python scripts/vgicp_bench.py --batch 2,8 [--workloads c1,s20k,c3,c5] [--resolutions 1.0] [--neighbors 1,7,27] [--reps 30]
is a measurement of its own (nothing of the above runs): alignBatchVoxel(B guesses) against B sequential voxel-mode align() calls on
the same handle in the same loop, host to host, per neighbourhood, at scripts/batch_bench.py's sizes, guesses and fixed 20 iterations;
medians and p10..p90.  The yardstick is the loop of single aligns.  It writes profiles/vgicp_batch_bench.json unless --out says otherwise.
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
    if name == "c1":
        return clouds.scan_to_scan(10_000)
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


def _batch_guesses(clouds, w, B):
    """scripts/batch_bench.py's: the workload's guess and B - 1 poses a few centimetres and a few tenths of a degree off it."""
    rng = np.random.default_rng(11)
    out = [np.asarray(w.guess, np.float32)]
    for _ in range(B - 1):
        t = rng.uniform(-0.03, 0.03, 3)
        r = rng.uniform(-0.3, 0.3, 3)
        out.append((np.asarray(w.guess, np.float64) @ clouds.make_pose(tuple(t), tuple(r))).astype(np.float32))
    return np.stack(out)


def batch_main(a, torch, clouds, ng):
    """--batch: alignBatchVoxel(B) against a loop of B voxel-mode align() calls."""
    fixed20 = dict(setMaximumIterations=20, setRotationEpsilon=1e-12, setTransformationEpsilon=1e-12)  # every lane runs all 20 iterations
    lanes = [int(v) for v in a.batch.split(",")]
    out = {"metric": "voxel_align_batch_vs_loop", "device": torch.cuda.get_device_name(0), "iterations": 20, "reps": a.reps, "workloads": {}}
    for name in (a.workloads or "c1,s20k,c3,c5").split(","):
        w = _workload(clouds, name)
        g = ng.NanoGICP()
        g.setCorrespondenceRandomness(20)
        for k, v in fixed20.items():
            getattr(g, k)(v)
        g.setInputTarget(w.target)
        g.setInputSource(w.source)
        g.calculateSourceCovariances()
        g.calculateTargetCovariances()
        res = {"source_points": int(len(w.source)), "target_points": int(len(w.target)), "resolutions": {}}
        for r in [float(v) for v in (a.resolutions or "1.0").split(",")]:
            g.setVoxelResolution(r)
            per_k = {}
            for K in [int(k) for k in a.neighbors.split(",")]:
                g.setNeighborSearchMethod(K)
                per_b = {}
                for B in lanes:
                    G = _batch_guesses(clouds, w, B)

                    def loop():
                        for q in G:
                            g.align(q)

                    for _ in range(3):  # warm both (the map, the buffers of either path)
                        g.alignBatchVoxel(G)
                        loop()
                    tb, tl = [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        rr = g.alignBatchVoxel(G)
                        t1 = time.perf_counter()
                        loop()
                        t2 = time.perf_counter()
                        tb.append((t1 - t0) * 1e3)
                        tl.append((t2 - t1) * 1e3)
                    b, l = _summ(tb), _summ(tl)
                    spread = max(b["p90_ms"] - b["p10_ms"], l["p90_ms"] - l["p10_ms"])
                    per_b[str(B)] = {"batch": b, "loop": l, "loop_over_batch": l["median_ms"] / b["median_ms"],
                                     "wins_beyond_spread": bool(l["median_ms"] - b["median_ms"] > spread), "iterations_per_lane": [int(v) for v in rr[2]]}
                    print(name, r, K, B, json.dumps(per_b[str(B)]), file=sys.stderr, flush=True)
                per_k[str(K)] = per_b
            res["resolutions"][str(r)] = {"voxels": int(g.getVoxelMapSize()), "neighbors": per_k}
        g.close()
        out["workloads"][name] = res
    line = json.dumps(out)
    path = a.out or os.path.join(ROOT, "profiles", "vgicp_batch_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="")
    ap.add_argument("--resolutions", default="")
    ap.add_argument("--batch", default="", help="B[,B...]: time alignBatchVoxel(B guesses) against B sequential voxel-mode align() calls instead")
    ap.add_argument("--neighbors", default="1,7,27")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    if a.batch:
        return batch_main(a, torch, clouds, ng)
    a.workloads = a.workloads or "c3,c5"
    a.resolutions = a.resolutions or "0.5,1.0,2.0"
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
