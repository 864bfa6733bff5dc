"""alignBatch(B guesses) against B sequential align() calls on the same handle (include/ngicp.h "more than one initial guess").

  python scripts/batch_bench.py [--workloads c1,s20k,c3,c5] [--lanes 1,2,4,8,16] [--reps 50] [--out profiles/batch_bench.json]
one JSON line on stdout (and in --out).  Kernel times: a run of its own under
  rocprofv3 --kernel-trace --stats -- python scripts/batch_bench.py --lanes 8 --reps 10

Workloads: c1 10k -> 10k scan-to-scan, s20k 20k -> 60k scan-to-submap, c3 100k -> 500k (bench.py's), c5 250k -> 2M OS1-128.  The
iteration count is fixed at 20 (tests/_pass_check.py FIXED20: epsilons 1e-12); the guesses are the workload's own and small
perturbations of it, so the lanes do the same work and the comparison is work for work.  Host-to-host times; the two ways alternate
inside one loop after both were warmed up.  The sequential loop is the single path, which the batch leaves as it was: the yardstick is
the code without the batch, not the code under test.
  wins_beyond_spread   loop median - batch median > the larger p10..p90 spread of the two
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


def _workload(clouds, name):
    if name == "c1":
        return clouds.scan_to_scan(10_000)
    if name == "s20k":
        return clouds.scan_to_submap(20_000, 3)
    if name == "c3":
        return clouds.scan_to_submap(100_000, 5)
    if name == "c5":
        return clouds.scan_to_submap(250_000, 8, shape="os1")
    raise SystemExit(f"unknown workload {name}")


def _guesses(clouds, w, B):
    rng = np.random.default_rng(11)
    out = [np.asarray(w.guess, np.float32)]
    for _ in range(B - 1):
        t = rng.uniform(-0.03, 0.03, 3)
        r = rng.uniform(-0.3, 0.3, 3)
        out.append((np.asarray(w.guess, np.float64) @ clouds.make_pose(tuple(t), tuple(r))).astype(np.float32))
    return np.stack(out)


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c1,s20k,c3,c5")
    ap.add_argument("--lanes", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    out = {"metric": "align_batch_vs_loop", "device": torch.cuda.get_device_name(0), "iterations": 20, "reps": a.reps, "workloads": {}}
    for name in a.workloads.split(","):
        w = _workload(clouds, name)
        g = ng.NanoGICP()
        g.setCorrespondenceRandomness(20)
        g.setMaxCorrespondenceDistance(w.max_corr_dist)
        for k, v in FIXED20.items():
            getattr(g, k)(v)
        g.setInputTarget(w.target)
        g.setInputSource(w.source)
        g.calculateSourceCovariances()
        g.calculateTargetCovariances()
        res = {"source_points": int(len(w.source)), "target_points": int(len(w.target)), "lanes": {}}
        for B in [int(v) for v in a.lanes.split(",")]:
            G = _guesses(clouds, w, B)

            def loop():
                for q in G:
                    g.align(q)

            for _ in range(3):  # warm both (buffers, launch orders)
                g.alignBatch(G)
                loop()
            tb, tl = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = g.alignBatch(G)
                t1 = time.perf_counter()
                loop()
                t2 = time.perf_counter()
                tb.append((t1 - t0) * 1e3)
                tl.append((t2 - t1) * 1e3)
            b, l = _summ(tb), _summ(tl)
            spread = max(b["p90_ms"] - b["p10_ms"], l["p90_ms"] - l["p10_ms"])
            res["lanes"][str(B)] = {"batch": b, "loop": l, "loop_over_batch": l["median_ms"] / b["median_ms"],
                                    "wins_beyond_spread": bool(l["median_ms"] - b["median_ms"] > spread),
                                    "lm_trials_per_lane": [int(len(g.lm_trace(lane=i))) for i in range(B)], "iterations_per_lane": [int(v) for v in r[2]]}
            print(name, B, json.dumps(res["lanes"][str(B)]), file=sys.stderr, flush=True)
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
