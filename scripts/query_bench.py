"""Timing of the query surface (include/ngicp.h "queries"): getFitnessScore, k-NN and radius search on the bench's clouds.

  python scripts/query_bench.py            one JSON line on stdout
Kernel times: run it once under  rocprofv3 --kernel-trace --stats -- python scripts/query_bench.py  (a run of its own).

  fitness_c3 / fitness_c5   after the bench's alignment (c3: 100k -> 500k VLP-16, bench.py's workload; c5: 250k -> 2M OS1-128):
                            host-to-host median / p99 over 50 calls, and the device time of the two kernels (HIP events);
                            cpu_oracle_kdtree_1nn_ms: the oracle's kd-tree (oracle/, NOT PCL) doing the same 1-NN queries at 16
                            threads, tree build excluded
  knn_k1 / knn_k20          ngicp_knn_search: the 100k transformed c3 source points as queries into the 500k target
  radius                    ngicp_radius_search + ngicp_radius_fetch: 10k of them, radius 0.25 (a SQUARED distance: 0.5 m)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GICP_ITERS = 20  # bench.py


def _timed(fn, reps, g):
    host, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(g.stats()["query_ms"])
    return out, {"host_median_ms": float(np.median(host)), "host_p99_ms": float(np.percentile(host, 99)), "device_median_ms": float(np.median(dev)), "calls": reps}


def _aligned(ng, clouds, w):
    tgt_covs = ng.keyframe_covariances(w.target, w.keyframe_sizes, 20)
    g = ng.NanoGICP()
    g.setCorrespondenceRandomness(20); g.setMaxCorrespondenceDistance(w.max_corr_dist)
    g.setMaximumIterations(GICP_ITERS); g.setTransformationEpsilon(1e-12); g.setRotationEpsilon(1e-12)
    g.setInputTarget(w.target); g.setTargetCovariances(tgt_covs)
    g.setInputSource(w.source); g.calculateSourceCovariances()
    for _ in range(3):
        g.align(w.guess)
    return g


def _fitness(ng, clouds, orc, w, reps=50):
    g = _aligned(ng, clouds, w)
    g.fitness()  # warm-up
    (score, n), t = _timed(g.fitness, reps, g)
    tr = g.transformSource(g.getFinalTransformation())
    tree = orc.OracleTree(w.target)
    t0 = time.perf_counter()
    d2 = tree.knn(tr, 1, threads=16)[1][:, 0]
    cpu_ms = (time.perf_counter() - t0) * 1e3
    ref = float(np.mean(d2.astype(np.float64)))
    t.update({"source_points": int(len(w.source)), "target_points": int(len(w.target)), "score": score, "n_inliers": int(n),
              "cpu_oracle_kdtree_1nn_ms": cpu_ms, "cpu_label": "oracle kd-tree, not PCL; 16 threads; tree build excluded",
              "score_rel_diff_vs_oracle_mean": abs(score - ref) / ref})
    return g, tr, t


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("query_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    from oracle import oracle as orc
    build.build()
    orc.build(ref=False)
    out = {"metric": "query_surface", "device": torch.cuda.get_device_name(0)}
    g, tr, out["fitness_c3"] = _fitness(ng, clouds, orc, clouds.scan_to_submap(100_000, 5))
    for k in (1, 20):
        g.nearestKSearch(tr, k)
        _, t = _timed(lambda: g.nearestKSearch(tr, k), 10, g)
        t.update({"queries": int(len(tr)), "cloud_points": int(g.stats()["n_tgt"]), "k": k})
        out[f"knn_k{k}"] = t
    q = np.ascontiguousarray(tr[::10])
    g.radiusSearch(q, 0.25)
    (off, _, _), t = _timed(lambda: g.radiusSearch(q, 0.25), 10, g)
    hits = int(off[-1])
    t.update({"queries": int(len(q)), "radius_sq": 0.25, "total_hits": hits, "max_hits_per_query": int(np.diff(off).max()),
              "hits_per_s_host": hits / (t["host_median_ms"] * 1e-3), "note": "host time includes ngicp_radius_fetch; device time is the search's kernels"})
    out["radius"] = t
    g.close()
    g5, _, out["fitness_c5"] = _fitness(ng, clouds, orc, clouds.scan_to_submap(250_000, 8, shape="os1"))
    g5.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
