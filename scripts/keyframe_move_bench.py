"""Moving every keyframe of a device-resident store (transformKeyframes, one kernel launch) against what a user had
before it: rebuilding the store from host copies.  All in one process, the routes alternating repetition by repetition.

  python scripts/keyframe_move_bench.py [--stores 12x7000,100x7000,500x7000,12x100000] [--reps 9] [--warmup 2]
                                        [--out profiles/keyframe_move_bench.json]
one JSON line on stdout (and in --out).

Per store of K keyframes of about n points (VLP-16 scans of the synthetic scene taken along a drive, 12 distinct ones reused in turn, each
put into the world frame on the host): the store is filled once, then every repetition corrects ALL K keyframes, each by its own small
rigid motion, three ways:
  move       transformKeyframes(range(K), Ts): the table upload, ONE kernel, the read-back of boxes and flag
  rebuild    clearKeyframes(), then per keyframe transformCloud(host copy, T), setInputSource, calculateSourceCovariances (k = 20),
             addKeyframe: an upload, an index build and an exact k-NN covariance pass per keyframe - what the API offered before
  rebuild_rot the same with the covariances rotated on the host (numpy, R C R^T of the host copy) and handed over through
             setSourceCovariances instead of the k-NN pass
host_ms: time.perf_counter around the whole route.  kernel_ms: keyframeTransformKernelMs(), the event time of k_keyframe_move.  Its
traffic is 128 bytes per point (16 + 48 in, 16 + 48 out); kernel_gbps is that over kernel_ms, copy_gbps the engine's own float4
stream copy (measureCopyBandwidth, read + write) in the same process.  Medians and p10..p90 over --reps after --warmup discarded ones
(the 500-keyframe store runs a third of the repetitions of the rebuild routes, at least 3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stores", default="12x7000,100x7000,500x7000,12x100000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_move_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("keyframe_move_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    prod, g = ng.NanoGICP(), ng.NanoGICP()
    prod.setCorrespondenceRandomness(20)
    out = {"metric": "keyframe_move_vs_rebuild", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "bytes_per_point": 128,
           "copy_gbps": float(g.measureCopyBandwidth(1 << 28, 10)), "stores": {}}
    sc = clouds.make_scene()
    for spec in a.stores.split(","):
        K, n = (int(x) for x in spec.split("x"))
        rng = np.random.default_rng(K * 31 + n)
        track = [clouds.make_pose((-2.2 + 0.4 * i, 0.1 * i - 0.6, 0.0), (0.0, 0.0, 5.0 * i)) for i in range(12)]  # (inside the scene's room)
        scans = [clouds.vlp16(sc, track[i], 500 + i, cols=max(n // 16, 2)) for i in range(min(K, 12))]
        poses = [track[i % 12] @ clouds.make_pose((0.01 * (i // 12), 0.0, 0.0)) for i in range(K)]  # (a reused scan is a keyframe of its own)
        host = [clouds.transform_points(poses[i], scans[i % len(scans)]) for i in range(K)]
        # a loop closure's corrections: up to a degree and 0.3 m per keyframe
        Ts = np.stack([clouds.make_pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-1.0, 1.0, 3)) for _ in range(K)]).astype(np.float32)
        R64 = Ts[:, :3, :3].astype(np.float64)
        host_covs = []

        def rebuild(rotate):
            g.clearKeyframes()
            for i in range(K):
                prod.setInputSource(g.transformCloud(host[i], Ts[i]))
                if rotate:
                    c = np.zeros_like(host_covs[i])
                    c[:, :3, :3] = R64[i] @ host_covs[i][:, :3, :3] @ R64[i].T
                    prod.setSourceCovariances(c)
                else:
                    prod.calculateSourceCovariances()
                g.addKeyframe(prod)

        g.clearKeyframes()
        for i in range(K):  # the store as it stands before the correction; the host copies of the covariances for rebuild_rot
            prod.setInputSource(host[i]); prod.calculateSourceCovariances()
            g.addKeyframe(prod)
            host_covs.append(prod.getSourceCovariances())
        ids = np.arange(K, dtype=np.int32)
        points = int(sum(len(h) for h in host))
        rec = {"move": [], "rebuild": [], "rebuild_rot": [], "kernel": []}
        heavy_every = 3 if K >= 500 else 1
        for rep in range(a.warmup + a.reps):
            keep = rep >= a.warmup
            routes = [("move", lambda: g.transformKeyframes(ids, Ts))]
            if rep % heavy_every == 0 or not keep:
                routes += [("rebuild", lambda: rebuild(False)), ("rebuild_rot", lambda: rebuild(True))]
            for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
                t, _ = _timed(fn)
                if keep:
                    rec[name].append(t)
                    if name == "move":
                        rec["kernel"].append(g.keyframeTransformKernelMs())
        cell = {"keyframes": K, "points": points, "move_host": _summ(rec["move"]), "move_kernel": _summ(rec["kernel"]),
                "rebuild_host": _summ(rec["rebuild"]), "rebuild_rot_host": _summ(rec["rebuild_rot"])}
        cell["kernel_gbps"] = 128.0 * points / (cell["move_kernel"]["median_ms"] * 1e-3) / 1e9
        cell["kernel_over_copy"] = cell["kernel_gbps"] / out["copy_gbps"]
        cell["rebuild_over_move"] = cell["rebuild_host"]["median_ms"] / cell["move_host"]["median_ms"]
        cell["rebuild_rot_over_move"] = cell["rebuild_rot_host"]["median_ms"] / cell["move_host"]["median_ms"]
        out["stores"][spec] = cell
        print(spec, json.dumps(cell), file=sys.stderr, flush=True)
    prod.close(); g.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
