"""The on-device pose-graph optimiser (poseGraphOptimize) against the same Levenberg-Marquardt loop on the host with
scipy.sparse normal equations and scipy.sparse.linalg.spsolve (tests/_pose_graph_model.py with its direct solve), on chains with one loop
edge per 50 nodes.   python scripts/pose_graph_bench.py [--sizes 100,1000,10000,100000] [--reps 5] [--out profiles/pose_graph_bench.json]

Per size: both routes optimise the same graph from the same drifted start, alternating, after one warm-up each; times are host to host
(time.perf_counter around the call, which ends in a synchronising read-back), reported as median and p10-p90.  Also: the device time of the
optimise (HIP events), CG iterations, device time per CG iteration, launches per LM try (2 + 3 per CG iteration + 3, one more after an
accepted try) and, at the smallest size, the share of the time that is launch overhead - estimated as launches times the cost of an empty
launch measured in the same run (cg_max_iterations launches of a solve that has already converged return at once on the device's flag).
Needs a GPU: there is no CPU fallback for the device route."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pose_graph_cases as pc  # noqa: E402
import _pose_graph_model as pgm  # noqa: E402


def chain_with_loops(n, seed=40):
    truth = pc.laps(n, seed)
    rng = np.random.default_rng(seed + 1)
    pairs = pc.chain_pairs(n)
    for k in range(max(1, n // 50)):
        a, b = sorted(rng.choice(n, 2, replace=False))
        pairs.append((int(a), int(b)))
    flags = np.r_[np.zeros(n - 1, bool), np.ones(len(pairs) - (n - 1), bool)]
    g, _ = pc.build(truth, pairs, [0], seed, flags=flags, drift_scale=0.3, noise_scale=0.3)
    return g


def spread(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,10000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=3, help="outer iterations of both routes (a run to convergence of a long chain takes minutes)")
    ap.add_argument("--cg-max", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_graph_bench needs a GPU")
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    opt = dict(max_iterations=args.max_iterations, rot_eps=1e-4, trans_eps=1e-4, cg_tol=1e-8, cg_max_iterations=args.cg_max)
    rows = []
    for n in [int(v) for v in args.sizes.split(",")]:
        g = chain_with_loops(n)
        e = NanoGICP()
        e.poseGraphAddNodes(g.poses, g.fixed)
        e.poseGraphAddEdges(g.ij, g.Z, g.info, g.flags)

        def device():
            e.poseGraphSetPoses(0, g.poses)
            t = time.perf_counter()
            r = e.poseGraphOptimize(**opt)
            return time.perf_counter() - t, r

        def host():
            h = g.copy()
            t = time.perf_counter()
            r = pgm.optimize(h, "direct", **opt)
            return time.perf_counter() - t, r, h.poses
        device(), host()  # warm-up: code objects, buffers, scipy's symbolic work
        td, th, kern = [], [], []
        for _ in range(args.reps):
            a, rd = device()
            td.append(a)
            kern.append(e.poseGraphKernelMs())
            b, rh, hp = host()
            th.append(b)
        diff = pc.pose_difference(e.poseGraphPoses(), hp)
        cg = rd["cg_iterations"]
        tries = len(rd["trace"])
        launches = tries * 5 + 3 * cg + rd["accepted"] + 3
        row = dict(nodes=n, edges=int(g.m), tries=tries, accepted=rd["accepted"], cg_iterations=cg, capped_solves=int((rd["trace"][:, 3] >= args.cg_max).sum()),
                   same_accept_sequence=[int(t[4]) for t in rd["trace"]] == [t[4] for t in rh["trace"]], pose_difference_to_host=diff,
                   device_s=spread(td), host_s=spread(th), device_kernel_ms=spread(kern), launches=launches, launches_per_try=launches / max(1, tries),
                   device_us_per_cg_iteration=1e3 * float(np.median(kern)) / max(1, cg))
        if not rows:
            # an empty launch: a graph with b = 0 (already optimal) ends its solve at once, so every launch of the capped loop up to the
            # host's next glance returns on the flag
            z = NanoGICP()
            z.poseGraphAddNodes(g.poses[:2], [True, False])
            z.poseGraphAddEdges([[0, 1]], (pgm.inv_pose(g.poses[0]) @ g.poses[1])[None], np.eye(6)[None])
            z.poseGraphOptimize(**opt)
            t = time.perf_counter()
            for _ in range(50):
                z.poseGraphOptimize(**opt)
            per_call = (time.perf_counter() - t) / 50
            row["tiny_graph_call_s"] = per_call  # 9 launches, two read-backs: a floor for any call
            row["launch_overhead_share"] = min(1.0, (per_call / 9.0) * launches / float(np.median(td)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        e.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(options=opt, reps=args.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
