"""What the pose prior costs when it is set, and what it does to the headline workload.

  python scripts/pose_prior_bench.py [--reps 10] [--prior both|off|on] [--out profiles/pose_prior_bench.json]
one JSON line on stdout (and in --out).

Workloads: c3 (100k -> 500k scan-to-submap, bench.py's clouds) and the 20k -> 60k pair, each on the exact route and on DIRECT1 at 1 m,
with bench.py's FIXED20 settings (20 iterations, both epsilons 1e-12, the workload's gate).  The prior: T_p = the guess,
L = --weight (default 1.0: a weak prior, sigma = 1 rad / 1 m) times the identity.  Prior off and prior on alternate inside one loop on
ONE handle; per workload, route and setting, after 3 warm-ups:
  us_per_iteration      device time of the loop (the engine's 100 MHz stamps, first pass to the solver's `done`) / passes: median and
                        p10..p90 of --reps alignments
  us_solver_and_gaps    the same less the pass kernel's own device time per pass (HIP events attached to its dispatches, from --reps
                        profiled alignments run apart from the timed ones): what an iteration spends outside the pass kernel - the solver
                        launch and the gaps around it
  align_ms              host to host, median and p10..p90
  error_vs_ground_truth the final pose's distance from ground truth (c3 FIXED20 without a prior is VERDICT.md's "slide along a valley")
and, on the exact route, effect_exact: the final pose's distance from ground truth and from the guess for L = weight * I over
--effect-weights (0: no prior), with the extreme diagonal entries of the final (summed) Hessian beside them for scale.
k_lm_solve's own duration per launch comes from a kernel trace, each setting in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/pose_prior_bench.py --prior off   (and --prior on)
Figures are reported as measured; nothing is gated.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXED20 = dict(setMaximumIterations=20, setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)
WORKLOADS = {"c3": (100_000, 5), "20k_60k": (20_000, 3)}
ROUTES = {"exact": 0, "direct1": 1}


def _q(v):
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weight", type=float, default=1.0)
    ap.add_argument("--effect-weights", default="1,1e2,1e4,1e5,1e6,1e7")
    ap.add_argument("--prior", choices=["both", "off", "on"], default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_prior_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    settings = [s for s in ("off", "on") if a.prior in ("both", s)]
    out = {"metric": "pose_prior_cost", "device": torch.cuda.get_device_name(0), "settings": FIXED20, "prior": f"T_p = guess, L = {a.weight} * I (rad^-2, m^-2)",
           "reps": a.reps, "workloads": {}}
    for wname, (n, kf) in WORKLOADS.items():
        w = clouds.scan_to_submap(n, kf)
        g = ng.NanoGICP()
        g.setCorrespondenceRandomness(20)
        g.setMaxCorrespondenceDistance(w.max_corr_dist)
        for k, v in FIXED20.items():
            getattr(g, k)(v)
        g.setInputTarget(w.target)
        g.setInputSource(w.source)
        g.calculateSourceCovariances()
        g.setTargetCovariances(ng.keyframe_covariances(w.target, w.keyframe_sizes, 20))
        Tp, Lam = np.asarray(w.guess, np.float64), a.weight * np.eye(6)

        def select(s):
            if s == "on":
                g.setPosePrior(Tp, Lam)
            else:
                g.clearPosePrior()

        res = {"source_points": int(len(w.source)), "target_points": int(len(w.target)),
               "guess_vs_ground_truth_m": float(clouds.pose_error(w.guess, w.gt)[0]), "routes": {}}
        for route, K in ROUTES.items():
            g.setVoxelResolution(1.0 if K else 0.0)
            if K:
                g.setNeighborSearchMethod(K)
            per = {s: {"align_ms": [], "us_per_iteration": [], "us_pass": []} for s in settings}
            for s in settings:
                select(s)
                for _ in range(3):
                    g.align(w.guess)
                st = g.stats()
                dt, dr = clouds.pose_error(g.getFinalTransformation(), w.gt)
                per[s].update(passes=int(st["passes"]), iterations=int(g.nr_iterations_ + 1), converged=bool(g.converged_),
                              error_vs_ground_truth_m=float(dt), error_vs_ground_truth_rad=float(dr),
                              moved_from_guess_m=float(clouds.pose_error(g.getFinalTransformation(), w.guess)[0]))
            for _ in range(a.reps):  # the settings alternate inside one loop
                for s in settings:
                    select(s)
                    t0 = time.perf_counter()
                    g.align(w.guess)
                    per[s]["align_ms"].append((time.perf_counter() - t0) * 1e3)
                    st = g.stats()
                    per[s]["us_per_iteration"].append(1e3 * st["loop_ms"] / max(1, st["passes"]))
            g.setProfiling(1)
            for _ in range(a.reps):
                for s in settings:
                    select(s)
                    g.align(w.guess)
                    st = g.stats()
                    per[s]["us_pass"].append(1e3 * st["pass_ms_total"] / max(1, st["passes_timed"]))
            g.setProfiling(0)
            for s in settings:
                pass_med = float(np.median(per[s]["us_pass"]))
                per[s]["us_solver_and_gaps"] = _q(np.asarray(per[s]["us_per_iteration"]) - pass_med)
                for key in ("align_ms", "us_per_iteration", "us_pass"):
                    per[s][key] = _q(per[s][key])
            if len(settings) == 2:
                per["on_less_off_us_per_iteration"] = per["on"]["us_per_iteration"]["median"] - per["off"]["us_per_iteration"]["median"]
            res["routes"][route] = per
            print(wname, route, json.dumps(per), file=sys.stderr, flush=True)
        # the effect on the final pose, exact route: T_p = the guess, L = weight * I for a sweep of weights (one alignment each)
        g.setVoxelResolution(0.0)
        res["effect_exact"] = []
        for wt in [0.0] + [float(x) for x in a.effect_weights.split(",")]:
            if wt > 0.0:
                g.setPosePrior(Tp, wt * np.eye(6))
            else:
                g.clearPosePrior()
            g.align(w.guess)
            T = g.getFinalTransformation()
            res["effect_exact"].append({"weight": wt, "error_vs_ground_truth_m": float(clouds.pose_error(T, w.gt)[0]),
                                        "error_vs_ground_truth_rad": float(clouds.pose_error(T, w.gt)[1]),
                                        "moved_from_guess_m": float(clouds.pose_error(T, w.guess)[0]), "iterations": int(g.nr_iterations_ + 1),
                                        "max_diag_H": float(np.abs(np.diag(g.getFinalHessian())).max()), "min_diag_H": float(np.abs(np.diag(g.getFinalHessian())).min())})
        g.close()
        out["workloads"][wname] = res
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
