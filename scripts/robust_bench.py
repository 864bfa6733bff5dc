"""What a robust kernel costs when it is on: NONE against Huber, Cauchy and Geman-McClure (width 1.0) in the same run on the same handle,
clouds, covariances and settings.

  python scripts/robust_bench.py [--reps 10] [--out profiles/robust_bench.json]
one JSON line on stdout (and in --out).

Routes: c3 (100k -> 500k scan-to-submap, bench.py's workload) on the exact route and, at 1 m, DIRECT1 and DIRECT7; DLO's scan-to-map
settings (32 iterations at most, transformation epsilon 0.01, the workload's gate).  Per route and kernel, after 3 warm-ups:
  us_per_pass        device time of the pass kernel from HIP events attached to its dispatches (ngicp_set_profiling), median of --reps
                     profiled alignments (runs apart from the timed ones: the events cost stream time)
  us_per_iteration   device time of the loop (the engine's 100 MHz stamps, first pass to the solver's `done`) / passes: median and
                     p10..p90 of --reps alignments
  align_ms           host to host: median and p10..p90 of the same alignments; the kernels alternate inside one loop
  passes, iterations a robust run takes another number of them, which is why the per-iteration figure stands beside the total
  *_vs_none          the medians relative to NONE's of the same route
and the final pose's distance from the ground truth.  k_robust_terms is timed at c3's 100k source points for K = 1 (exact) and K = 7:
host-to-host robust_terms() (it includes the download of 2 n K doubles), median of --reps calls.
Figures are reported as measured.
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
ROUTES = {"exact": 0, "direct1": 1, "direct7": 7}
KERNELS = ["NONE", "HUBER", "CAUCHY", "GEMAN_MCCLURE"]


def _q(v):
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("robust_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    w = clouds.scan_to_submap(100_000, 5)
    g = ng.NanoGICP()
    g.setCorrespondenceRandomness(20)
    g.setMaxCorrespondenceDistance(w.max_corr_dist)
    for k, v in DLO.items():
        getattr(g, k)(v)
    g.setInputTarget(w.target)
    g.setInputSource(w.source)
    g.calculateSourceCovariances()
    g.setTargetCovariances(ng.keyframe_covariances(w.target, w.keyframe_sizes, 20))  # per keyframe, as DLO supplies them
    out = {"metric": "robust_kernel_cost", "device": torch.cuda.get_device_name(0), "workload": "c3", "settings": DLO, "width": a.width, "reps": a.reps,
           "source_points": int(len(w.source)), "target_points": int(len(w.target)), "routes": {}, "robust_terms": {}}
    for route, K in ROUTES.items():
        g.setVoxelResolution(1.0 if K else 0.0)
        if K:
            g.setNeighborSearchMethod(K)
        kinds = {name: getattr(ng.RobustKernel, name) for name in KERNELS}
        per = {name: {"align_ms": [], "us_per_iteration": [], "us_per_pass": []} for name in KERNELS}
        for name, kind in kinds.items():  # warm-up, and the figures that do not vary
            g.setRobustKernel(kind, a.width)
            for _ in range(3):
                g.align(w.guess)
            s = g.stats()
            dt, dr = clouds.pose_error(g.getFinalTransformation(), w.gt)
            per[name].update(passes=int(s["passes"]), iterations=int(g.nr_iterations_ + 1), lm_trials=int(s["lm_trials"]), converged=bool(g.converged_),
                             error_vs_ground_truth_m=dt, error_vs_ground_truth_rad=dr)
        for _ in range(a.reps):  # the kernels alternate inside one loop
            for name, kind in kinds.items():
                g.setRobustKernel(kind, a.width)
                t0 = time.perf_counter()
                g.align(w.guess)
                per[name]["align_ms"].append((time.perf_counter() - t0) * 1e3)
                s = g.stats()
                per[name]["us_per_iteration"].append(1e3 * s["loop_ms"] / max(1, s["passes"]))
        g.setProfiling(1)
        for _ in range(a.reps):
            for name, kind in kinds.items():
                g.setRobustKernel(kind, a.width)
                g.align(w.guess)
                s = g.stats()
                per[name]["us_per_pass"].append(1e3 * s["pass_ms_total"] / max(1, s["passes_timed"]))
        g.setProfiling(0)
        for name in KERNELS:
            for key in ("align_ms", "us_per_iteration", "us_per_pass"):
                per[name][key] = _q(per[name][key])
        for name in KERNELS[1:]:
            for key in ("align_ms", "us_per_iteration", "us_per_pass"):
                per[name][key + "_vs_none"] = per[name][key]["median"] / per["NONE"][key]["median"]
        out["routes"][route] = per
        print(route, json.dumps(per), file=sys.stderr, flush=True)
        if K in (0, 7):  # k_robust_terms at 100k points, K = 1 and 7 (the state is that of the last alignment)
            g.setRobustKernel(ng.RobustKernel.CAUCHY, a.width)
            g.align(w.guess)
            ms = []
            for _ in range(a.reps + 3):
                t0 = time.perf_counter()
                s_, w_ = g.robust_terms()
                ms.append((time.perf_counter() - t0) * 1e3)
            out["robust_terms"][f"K{max(K, 1)}"] = {"n_src": int(len(w.source)), "host_to_host_ms": _q(ms[3:]), "terms": int((s_ >= 0).sum()),
                                                    "mean_weight": float(w_[s_ >= 0].mean())}
    g.setRobustKernel(ng.RobustKernel.NONE)
    g.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
