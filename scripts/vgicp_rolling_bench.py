"""Scan-to-map odometry against a rolling voxel map (setVoxelRolling) against the same drive through the keyframe store
and the merged voxel map, in the same process, the two routes alternating frame by frame.

  python scripts/vgicp_rolling_bench.py [--variants filtered,unfiltered] [--resolutions 0.5,1.0] [--frames 40] [--warmup 10] [--points 100000] [--evict-every 3]
                                        [--out profiles/vgicp_rolling_bench.json]
one JSON line on stdout (and in --out).

Workload: a synthetic drive through clouds.make_scene(): one VLP-16 scan of --points rays per frame, 0.32 m and 1 degree of yaw apart along the x axis.
`filtered` passes every scan through the engine's scan filter first (preprocessScan, VoxelGrid leaf 0.5 m, untimed: both routes get the
same filtered cloud), as DLO's shipped configuration filters what becomes a keyframe; `unfiltered` aligns and inserts all --points rays.
Every frame is aligned from its ground truth displaced by (0.05 m, 0.5 deg), DLO's scan-to-map settings (32 iterations at most,
transformation epsilon 0.01), DIRECT7, and then added to the map at the pose the alignment returned.  Each route has its own handle;
the frame's source is set on it (uploaded, indexed) before anything is timed, its covariances are left to the align that needs them.

Per frame and route, host to host (time.perf_counter around calls that end in a device synchronisation):
  rolling    align_ms, insert_ms (insertIntoVoxelMap at the result), evict_ms every --evict-every frames (evictVoxelMap by stamp: what no
             scan of the last WINDOW touched goes - the keyframe route's window); frame_ms = align + insert + evict (0 where none ran)
  keyframe   add_ms (addKeyframeTransformed at the result: index + k-NN covariances of the transformed scan), submap_ms
             (setSubmapKeyframes of the last WINDOW keyframes), build_ms (the merged map build, getVoxelMapSize), align_ms;
             frame_ms = their sum
The first --warmup frames are discarded.  Medians and p10..p90 over --frames timed frames.
From the engine: the insert's device event time per frame with the map's voxel count before it, and a sweep of its own - the same scan
inserted at poses 60 m apart into a map that is never evicted, then once more where it already is - for the claim that an insert
costs the scan and not the map: insert_ms against voxels in the map, with a least-squares slope in microseconds per 100k map voxels.
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
WINDOW, LEAF = 5, 0.5


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="filtered,unfiltered")
    ap.add_argument("--resolutions", default="0.5,1.0")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--evict-every", type=int, default=3)
    ap.add_argument("--sweep", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgicp_rolling_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_rolling_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    sc = clouds.make_scene()
    cols = a.points // 16
    n_frames = a.warmup + a.frames
    gts = [clouds.make_pose((-0.16 * (n_frames - 1) + 0.32 * i, 0.0, 0.0), (0.0, 0.0, 1.0 * i - 0.5 * n_frames)) for i in range(n_frames)]
    scans = [clouds.vlp16(sc, p, 400 + i, cols=cols) for i, p in enumerate(gts)]
    guesses = [(p @ clouds.make_pose((0.05, -0.03, 0.02), (0.2, -0.3, 0.5))).astype(np.float32) for p in gts]

    out = {"metric": "scan_to_map_frame_rolling_vs_keyframe", "device": torch.cuda.get_device_name(0), "settings": DLO, "neighbors": 7, "frames": a.frames,
           "warmup": a.warmup, "window": WINDOW, "evict_every": a.evict_every, "rays_per_scan": int(len(scans[0])), "filter_leaf": LEAF, "variants": {}}
    raw = scans
    for variant, r in [(v, float(x)) for v in a.variants.split(",") for x in a.resolutions.split(",")]:
        if variant == "filtered":
            pre = ng.NanoGICP()
            scans = [np.ascontiguousarray(pre.preprocessScan(s, voxel_res=LEAF)[:, :3], np.float32) for s in raw]
            pre.close()
        else:
            scans = raw
        roll, kf = ng.NanoGICP(), ng.NanoGICP()
        for h in (roll, kf):
            h.setCorrespondenceRandomness(20)
            h.setVoxelResolution(r)
            h.setNeighborSearchMethod(7)
            for k, v in DLO.items():
                getattr(h, k)(v)
        roll.setVoxelRolling(True)
        kf.setVoxelSubmapMerge(True)
        # frame 0 founds both maps at its ground truth
        T0 = gts[0].astype(np.float32)
        roll.setInputSource(scans[0]); roll.insertIntoVoxelMap(roll, T0)
        kf.setInputSource(scans[0]); ids = [kf.addKeyframeTransformed(kf, T0)]
        kf.setSubmapKeyframes(ids); kf.getVoxelMapSize()
        rec = {"rolling": {k: [] for k in ("align_ms", "insert_ms", "evict_ms", "frame_ms", "insert_device_ms", "evict_device_ms")},
               "keyframe": {k: [] for k in ("align_ms", "add_ms", "submap_ms", "build_ms", "frame_ms", "build_device_ms")}}
        per_frame, err = [], {"rolling": [], "keyframe": []}
        for i in range(1, n_frames):
            timed = i >= a.warmup
            for route in (("rolling", "keyframe") if i % 2 == 0 else ("keyframe", "rolling")):
                if route == "rolling":
                    roll.setInputSource(scans[i])
                    t_align, _ = _timed(lambda: roll.align(guesses[i]))
                    T = roll.getFinalTransformation().copy()
                    n_before = roll.voxelRollingStats()["n_vox"]
                    t_ins, (n_new, n_touched) = _timed(lambda: roll.insertIntoVoxelMap(roll, T))
                    st = roll.voxelRollingStats()
                    t_ev, n_gone, ev_dev = 0.0, 0, None
                    if i % a.evict_every == 0:
                        t_ev, n_gone = _timed(lambda: roll.evictVoxelMap(T[:3, 3], 0.0, st["inserts"] - WINDOW + 1))
                        ev_dev = roll.voxelRollingStats()["last_evict_ms"]
                    if timed:
                        for k, v in (("align_ms", t_align), ("insert_ms", t_ins), ("frame_ms", t_align + t_ins + t_ev), ("insert_device_ms", st["last_insert_ms"])):
                            rec[route][k].append(v)
                        if ev_dev is not None:
                            rec[route]["evict_ms"].append(t_ev)
                            rec[route]["evict_device_ms"].append(ev_dev)
                        per_frame.append({"frame": i, "map_voxels_before": int(n_before), "scan_voxels": int(n_touched), "new_voxels": int(n_new),
                                          "insert_device_ms": st["last_insert_ms"], "evicted": int(n_gone)})
                        err[route].append(clouds.pose_error(T, gts[i]) + (bool(roll.converged_), roll.nr_iterations_ + 1))
                else:
                    kf.setInputSource(scans[i])
                    t_align, _ = _timed(lambda: kf.align(guesses[i]))
                    T = kf.getFinalTransformation().copy()
                    t_add, kid = _timed(lambda: kf.addKeyframeTransformed(kf, T))
                    ids = (ids + [kid])[-WINDOW:]
                    t_sub, _ = _timed(lambda: kf.setSubmapKeyframes(ids))
                    t_build, _ = _timed(kf.getVoxelMapSize)
                    if timed:
                        for k, v in (("align_ms", t_align), ("add_ms", t_add), ("submap_ms", t_sub), ("build_ms", t_build),
                                     ("frame_ms", t_align + t_add + t_sub + t_build), ("build_device_ms", kf.stats()["voxelmap_ms"])):
                            rec[route][k].append(v)
                        err[route].append(clouds.pose_error(T, gts[i]) + (bool(kf.converged_), kf.nr_iterations_ + 1))
        cell = {route: {k: _summ(v) for k, v in rec[route].items() if v} for route in rec}
        for route in rec:
            e = np.array([(x[0], x[1]) for x in err[route]])
            cell[route].update(worst_error_vs_ground_truth_m=float(e[:, 0].max()), worst_error_vs_ground_truth_rad=float(e[:, 1].max()),
                               all_converged=bool(all(x[2] for x in err[route])), median_iterations=float(np.median([x[3] for x in err[route]])))
        fr, fk = cell["rolling"]["frame_ms"], cell["keyframe"]["frame_ms"]
        cell["keyframe_over_rolling"] = {"frame_ms": fk["median_ms"] / fr["median_ms"],
                                         "beyond_spread": bool(abs(fk["median_ms"] - fr["median_ms"]) > max(fk["p90_ms"] - fk["p10_ms"], fr["p90_ms"] - fr["p10_ms"]))}
        cell["map_voxels"] = {"rolling": int(roll.voxelRollingStats()["n_vox"]), "keyframe_window": int(kf.getVoxelMapSize())}
        cell["rolling_frames"] = per_frame
        # the sweep: the same scan at poses 60 m apart, nothing evicted - the map grows by the scan's voxels per insert, the scan stays the same
        roll.clearVoxelMap()
        roll.setInputSource(scans[0]); roll.calculateSourceCovariances()
        sweep = []
        for j in range(a.sweep):
            for rep in range(3):  # the first insert at a pose creates its voxels, the next two find them all present
                n_before = roll.voxelRollingStats()["n_vox"]
                t_host, (n_new, n_touched) = _timed(lambda: roll.insertIntoVoxelMap(roll, clouds.make_pose((60.0 * j, 0.0, 0.0)).astype(np.float32)))
                sweep.append({"map_voxels_before": int(n_before), "scan_voxels": int(n_touched), "new_voxels": int(n_new), "insert_device_ms": roll.voxelRollingStats()["last_insert_ms"],
                              "insert_host_ms": t_host})
        present = [s for s in sweep if s["new_voxels"] == 0 and s["map_voxels_before"] > 0][1::2]  # the second all-present insert at every pose: no growth in it
        x = np.array([s["map_voxels_before"] for s in present], float); y = np.array([s["insert_device_ms"] for s in present])
        slope = float(np.polyfit(x, y, 1)[0]) if len(present) > 2 else None
        cell["insert_vs_map_size"] = {"inserts": sweep, "all_present_inserts": present,
                                      "slope_us_per_100k_map_voxels": None if slope is None else slope * 1e3 * 1e5,
                                      "all_present_insert_device_ms": _summ(y) if len(y) else None,
                                      "map_voxels_from_to": [int(x.min()), int(x.max())] if len(x) else None, "stats": roll.voxelRollingStats()}
        cell["points_per_scan_median"] = int(np.median([len(s) for s in scans]))
        out["variants"].setdefault(variant, {})[str(r)] = cell
        print(variant, r, json.dumps({k: v for k, v in cell.items() if k not in ("rolling_frames", "insert_vs_map_size")}), file=sys.stderr, flush=True)
        print(variant, r, "insert vs map size:", json.dumps({k: v for k, v in cell["insert_vs_map_size"].items() if k != "inserts"}), file=sys.stderr, flush=True)
        roll.close(); kf.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
