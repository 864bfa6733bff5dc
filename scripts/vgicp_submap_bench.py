"""The voxel map of a sliding submap built from the submap's points against the same map merged from per-keyframe voxel sums
(setVoxelSubmapMerge), in the same process, on the same handle and keyframe store, the two routes interleaved.

  python scripts/vgicp_submap_bench.py [--variants unfiltered,filtered] [--resolutions 0.5,1.0,2.0] [--reps 30] [--warmup 14]
                                       [--points 100000] [--out profiles/vgicp_submap_bench.json]
one JSON line on stdout (and in --out).  Kernel times from the profiler: a run of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/vgicp_submap_bench.py --reps 5
whose kernel table belongs next to the JSON as profiles/vgicp_submap_kernel_stats.csv (tracing slows the host: no host-to-host figure
of that run is used).

Workload: a DLO-like keyframe store of 12 VLP-16 keyframes 2 m apart (c3's shape: --points per scan, transformed on the device), the
submap being 5 consecutive ones; it advances by one keyframe per step, up the store and down again, so every step replaces exactly one
keyframe of the submap.  `unfiltered` keeps every point of a keyframe (addKeyframeTransformed); `filtered` is DLO's shipped setting
(addKeyframeTransformedFiltered, leaf 0.5 m).  DLO's scan-to-map settings (32 iterations at most, transformation epsilon 0.01).  The
source of a step is a scan from the middle of its submap, set (uploaded, indexed, covariances) before anything is timed.

Per step and route, host to host (time.perf_counter around calls that end in a device synchronisation):
  submap_ms    setSubmapKeyframes alone: concatenation, index, covariance scatter.  Both routes pay it; this change leaves it in place.
  build_ms     the forced map build, getVoxelMapSize()
  align_ms     one align() on the map just built
and from the engine: voxelmap_ms (device events around the build, either route) and, for the merged route, the split of
voxelMapMergeStats (parts, merge).  A step's two routes run back to back on the same submap, in alternating order; between them the
target is made a one-keyframe submap (untimed) so that the second route rebuilds the submap too.  The first --warmup steps are
discarded: they load code, grow buffers, and - one sweep up the store - build every keyframe's part.  What those steps cost on the
merged route, where one part is built in the same step, is reported apart (merged_with_one_part_built); so is the first merged build
after a change of resolution, which builds all five.
Medians and p10..p90 over --reps timed steps per cell; point_over_merged is the ratio of the two build medians of the same cell.
The final pose's distance from the ground truth is a sanity figure: that of the last timed step, which both routes run on the same submap
and source (final_pose_of_step / submap_first_keyframe name it).
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
N_KEYFRAMES, WINDOW, LEAF = 12, 5, 0.5


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _windows(n_steps):
    """first keyframe of the submap per step: up the store and down again, one keyframe replaced per step"""
    last = N_KEYFRAMES - WINDOW
    cycle = list(range(1, last + 1)) + list(range(last - 1, -1, -1))
    return [cycle[i % len(cycle)] for i in range(n_steps)]


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="unfiltered,filtered")
    ap.add_argument("--resolutions", default="0.5,1.0,2.0")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=14)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgicp_submap_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_submap_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    sc = clouds.make_scene()
    cols = a.points // 16
    kf_poses = [clouds.make_pose(((i - (N_KEYFRAMES - 1) / 2.0) * 2.0, 0.0, 0.0)) for i in range(N_KEYFRAMES)]
    kf_scans = [clouds.vlp16(sc, p, 100 + i, cols=cols) for i, p in enumerate(kf_poses)]
    # one source per submap position: a scan from the middle of the submap, displaced as bench.py's ground truth is
    src_gt = [clouds.make_pose(((s + (WINDOW - 1) / 2.0 - (N_KEYFRAMES - 1) / 2.0) * 2.0, 0.0, 0.0)) @ clouds.gt_transform() for s in range(N_KEYFRAMES - WINDOW + 1)]
    src_scans = [clouds.vlp16(sc, p, 1 + s, cols=cols) for s, p in enumerate(src_gt)]
    src_guess = [(p @ clouds.make_pose((0.05, -0.03, 0.02), (0.2, -0.3, 0.5))).astype(np.float32) for p in src_gt]

    out = {"metric": "voxel_map_build_point_vs_merged", "device": torch.cuda.get_device_name(0), "settings": DLO, "reps": a.reps, "warmup": a.warmup,
           "keyframes": N_KEYFRAMES, "submap_keyframes": WINDOW, "points_per_scan": int(len(kf_scans[0])), "variants": {}}
    for variant in a.variants.split(","):
        prod, g = ng.NanoGICP(), ng.NanoGICP()
        for h in (prod, g):
            h.setCorrespondenceRandomness(20)
        for k, v in DLO.items():
            getattr(g, k)(v)
        for scan, pose in zip(kf_scans, kf_poses):
            prod.setInputSource(scan)
            if variant == "filtered":
                g.addKeyframeTransformedFiltered(prod, pose, LEAF)
            else:
                g.addKeyframeTransformed(prod, pose)
        sizes = [g.keyframeSize(k) for k in range(N_KEYFRAMES)]
        res_out = {}
        for r in [float(v) for v in a.resolutions.split(",")]:
            g.setVoxelResolution(r)  # (the parts of another resolution are rebuilt when a merged build next asks for them)
            rec = {route: {"submap_ms": [], "build_ms": [], "align_ms": [], "voxelmap_ms": []} for route in ("point", "merged")}
            split = {"parts_ms": [], "merge_ms": []}
            one_part = {"build_ms": [], "voxelmap_ms": [], "parts_ms": [], "merge_ms": []}
            first_merged = None
            err, n_vox, n_tgt = {}, 0, 0
            steps = _windows(a.warmup + a.reps)
            for i, s in enumerate(steps):
                ids = list(range(s, s + WINDOW))
                g.setInputSource(src_scans[s])
                g.calculateSourceCovariances()
                for route in (("point", "merged") if i % 2 == 0 else ("merged", "point")):
                    g.setSubmapKeyframes([ids[0]])  # untimed: the timed call below then rebuilds the submap for this route too
                    g.setVoxelSubmapMerge(route == "merged")
                    before = g.voxelMapMergeStats()
                    t_sub, changed = _timed(lambda: g.setSubmapKeyframes(ids))
                    assert changed
                    t_build, n_vox = _timed(g.getVoxelMapSize)
                    st = g.stats()
                    ms = g.voxelMapMergeStats()
                    t_align, _ = _timed(lambda: g.align(src_guess[s]))
                    n_tgt = int(g.stats()["n_tgt"])
                    assert ms["merged_builds"] - before["merged_builds"] == (1 if route == "merged" else 0)
                    built = ms["parts_built"] - before["parts_built"]
                    if route == "merged" and first_merged is None:
                        first_merged = {"parts_built": built, "build_ms": t_build, "voxelmap_ms": st["voxelmap_ms"], "parts_ms": ms["last_parts_ms"], "merge_ms": ms["last_merge_ms"]}
                    elif route == "merged" and built == 1:
                        for k, v in (("build_ms", t_build), ("voxelmap_ms", st["voxelmap_ms"]), ("parts_ms", ms["last_parts_ms"]), ("merge_ms", ms["last_merge_ms"])):
                            one_part[k].append(v)
                    if i < a.warmup:
                        continue
                    assert built == 0, "a part was built in a timed step: --warmup must cover one sweep up the store"
                    for k, v in (("submap_ms", t_sub), ("build_ms", t_build), ("align_ms", t_align), ("voxelmap_ms", st["voxelmap_ms"])):
                        rec[route][k].append(v)
                    if route == "merged":
                        split["parts_ms"].append(ms["last_parts_ms"])
                        split["merge_ms"].append(ms["last_merge_ms"])
                    dt, dr = clouds.pose_error(g.getFinalTransformation(), src_gt[s])
                    err[route] = {"final_pose_of_step": i, "submap_first_keyframe": s, "error_vs_ground_truth_m": dt, "error_vs_ground_truth_rad": dr,
                                  "iterations": g.nr_iterations_ + 1, "converged": bool(g.converged_)}
            cell = {route: {k: _summ(v) for k, v in rec[route].items()} for route in rec}
            for route in rec:
                cell[route].update(err[route])
            cell["merged"]["split"] = {k: _summ(v) for k, v in split.items()}
            cell["merged_with_one_part_built"] = {k: _summ(v) for k, v in one_part.items()} if one_part["build_ms"] else None
            cell["first_merged_build_after_the_resolution_changed"] = first_merged
            bp, bm = cell["point"]["build_ms"], cell["merged"]["build_ms"]
            cell["point_over_merged"] = {"build_ms": bp["median_ms"] / bm["median_ms"],
                                         "voxelmap_ms": cell["point"]["voxelmap_ms"]["median_ms"] / cell["merged"]["voxelmap_ms"]["median_ms"],
                                         "beyond_spread": bool(abs(bp["median_ms"] - bm["median_ms"]) > max(bp["p90_ms"] - bp["p10_ms"], bm["p90_ms"] - bm["p10_ms"]))}
            cell["step_total_median_ms"] = {route: sum(cell[route][k]["median_ms"] for k in ("submap_ms", "build_ms", "align_ms")) for route in rec}
            cell.update(voxels=int(n_vox), target_points=n_tgt)
            res_out[str(r)] = cell
            print(variant, r, json.dumps(cell), file=sys.stderr, flush=True)
        out["variants"][variant] = {"keyframe_points": sizes, "resolutions": res_out}
        prod.close(); g.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
