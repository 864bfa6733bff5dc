"""The voxel pose search (voxelPoseSearch; k_ps_map_box / k_ps_src_box / k_ps_occ_fill / k_ps_score / k_ps_topk) against
what a user has without it, all in one process, warmed.

  python scripts/pose_search_bench.py [--sizes 5k,100k] [--reps 15] [--warmup 3] [--out profiles/pose_search_bench.json]
one JSON line on stdout (and in --out).

Two sizes, both on a rolling map at 0.5 m, and the window of the issue: 72 yaws at 5 degrees times 25 x 25 x 3 shifts = 135 000 poses.
  5k    a 5k-ray VLP-16 scan against the 50-scan map of scripts/vgicp_rollmap_bench.py (50 scans of 100k rays along its drive, about
        22k voxels); the scan is taken at the drive's 26th pose yawed by 37 degrees and moved by (2.3, -1.7, 0) m, the lattice starts at
        that pose of the drive
  100k  clouds.scan_to_submap(100_000, 5): a 100k scan against a map of its 500k-point target, the lattice starts at the pair's guess
  pose_search            voxelPoseSearch(yawLattice(guess, 72, 5 deg), (12, 12, 1), 8), host to host (time.perf_counter around the call:
                         the upload of the poses, both read-backs and the candidate poses included) and its kernels' event time
                         (voxelPoseSearchKernelMs()).  Medians with p10 .. p90 over --reps repetitions after --warmup discarded ones.
  voxel_fitness_route    what a user has today: voxelFitnessBatch under DIRECT1 over candidate poses.  Measured over a SUBSAMPLE - every
                         100th pose of the lattice in index order, 1 350 poses - and reported scaled by 100 (scaled_from_subsample: true).
                         The two do not compute the same number for a border point (the search counts on cells), and the fitness also
                         pays a Mahalanobis term per point; it is the call a user would reach for.
  numpy_model            tests/_pose_search_model.py score_volume over 2 of the 72 base poses, scaled by 36 (scaled_from_subsample: true).
The best candidate of every size is checked against the model restricted to its base pose before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = 0.5
SIZES = ("5k", "100k")
EXTENT, N_YAWS, YAW_STEP = (12, 12, 1), 72, np.radians(5.0)
SUBSAMPLE = 100


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5k,100k")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_search_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_search_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    import _pose_search_model as psm
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    out = {"metric": "voxel_pose_search_vs_voxel_fitness_and_numpy", "device": torch.cuda.get_device_name(0), "resolution": RES, "extent": list(EXTENT),
           "n_yaws": N_YAWS, "poses": N_YAWS * 25 * 25 * 3, "reps": a.reps, "warmup": a.warmup, "sizes": {}}
    for size in a.sizes.split(","):
        if size not in SIZES:
            raise SystemExit(f"unknown size {size}: one of {SIZES}")
        g = ng.NanoGICP()
        g.setVoxelResolution(RES)
        g.setVoxelRolling(True)
        g.setNeighborSearchMethod(1)
        if size == "5k":
            sc, n_scans = clouds.make_scene(), 50
            gts = [clouds.make_pose((-0.16 * (n_scans - 1) + 0.32 * i, 0.0, 0.0), (0.0, 0.0, 1.0 * i - 0.5 * n_scans)) for i in range(n_scans)]
            for i, p in enumerate(gts):
                g.setInputSource(clouds.vlp16(sc, p, 400 + i, cols=100_000 // 16))
                g.insertIntoVoxelMap(g, p.astype(np.float32))
            source = clouds.vlp16(sc, gts[25] @ clouds.make_pose((2.3, -1.7, 0.0), (0.0, 0.0, 37.0)), 900, cols=5_000 // 16)
            T0, n_tgt = gts[25], n_scans * (100_000 // 16) * 16
        else:
            w = clouds.scan_to_submap(100_000, 5)
            g.setInputSource(w.target)
            g.insertIntoVoxelMap(g, np.eye(4, dtype=np.float32))
            source, T0, n_tgt = w.source, w.guess, len(w.target)
        g.setInputSource(source)
        map_ijk = g.voxelMap()[0]
        Ts = ng.NanoGICP.yawLattice(np.asarray(T0, np.float64), N_YAWS, YAW_STEP)
        pose, shift, score, cand = g.voxelPoseSearch(Ts, EXTENT, 8)
        b0 = int(pose[0])
        want = psm.score_volume(Ts[b0:b0 + 1], source, map_ijk, RES, EXTENT)
        if not np.array_equal(g.voxelPoseSearchScores()[b0:b0 + 1], want):
            raise SystemExit(f"{size}: the engine's volume of base pose {b0} is not the model's")
        rec = {"n_src": int(len(source)), "n_tgt": int(n_tgt), "voxels": int(len(map_ijk)),
               "best": {"pose": b0, "shift": shift[0].tolist(), "score": int(score[0])}}
        host, kern = [], []
        for rep in range(a.warmup + a.reps):
            t, _ = _timed(lambda: g.voxelPoseSearch(Ts, EXTENT, 8))
            if rep >= a.warmup:
                host.append(t); kern.append(g.voxelPoseSearchKernelMs())
        rec["pose_search"] = {"host_ms": _summ(host), "kernel_ms": _summ(kern)}
        # the fitness route over every 100th pose of the lattice
        S = psm.shifts(EXTENT)
        idx = np.arange(0, N_YAWS * len(S), SUBSAMPLE)
        sub = np.stack([ng.NanoGICP.poseSearchCandidate(Ts[i // len(S)], S[i % len(S)], RES) for i in idx])
        g.voxelFitnessBatch(sub[:8])  # (the source's covariances exist from here on)
        fh, fk = [], []
        for rep in range(a.warmup + a.reps):
            t, _ = _timed(lambda: g.voxelFitnessBatch(sub))
            if rep >= a.warmup:
                fh.append(t); fk.append(g.voxelFitnessKernelMs())
        rec["voxel_fitness_route"] = {"poses_measured": int(len(sub)), "scale": SUBSAMPLE, "scaled_from_subsample": True, "host_ms_measured": _summ(fh),
                                      "kernel_ms_measured": _summ(fk), "host_ms_scaled_median": SUBSAMPLE * float(np.median(fh)),
                                      "kernel_ms_scaled_median": SUBSAMPLE * float(np.median(fk))}
        nm = [_timed(lambda: psm.score_volume(Ts[:2], source, map_ijk, RES, EXTENT))[0] for _ in range(3)]
        rec["numpy_model"] = {"poses_measured": 2 * len(S), "scale": N_YAWS // 2, "scaled_from_subsample": True, "host_ms_measured": _summ(nm),
                              "host_ms_scaled_median": (N_YAWS // 2) * float(np.median(nm))}
        rec["fitness_route_over_search_host"] = rec["voxel_fitness_route"]["host_ms_scaled_median"] / rec["pose_search"]["host_ms"]["median_ms"]
        rec["numpy_over_search_host"] = rec["numpy_model"]["host_ms_scaled_median"] / rec["pose_search"]["host_ms"]["median_ms"]
        out["sizes"][size] = rec
        print(size, json.dumps(rec), file=sys.stderr, flush=True)
        g.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
