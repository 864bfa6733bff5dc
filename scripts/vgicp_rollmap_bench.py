"""The rolling voxel map's record routes (restore, insert of records, handle-to-handle insert, move in place) against
the scan insert, all in one process on one handle pair, the routes alternating repetition by repetition.

  python scripts/vgicp_rollmap_bench.py [--sizes 1600,16000,60000] [--reps 15] [--warmup 3] [--scans 50] [--points 100000]
                                        [--out profiles/vgicp_rollmap_bench.json]
one JSON line on stdout (and in --out).

Per map size V (voxels): V synthetic records - distinct random voxels of a 0.5 m lattice, a mean inside each, a count of 1..12 and a
positive definite covariance sum - live on handle `src`; the yardstick is a synthetic cloud with 6 points in each of the same V voxels
on handle `prod`, its covariances computed before anything is timed, so that the scan insert sees a scan of exactly V voxels.
Every repetition runs, on the destination handle `dst`:
  scan_insert_new / _present        insertIntoVoxelMap(prod, T) into the cleared map, then again where every voxel is present
  insert_map_new / _present         insertVoxelMapFrom(src, T) likewise (device to device)
  insert_voxels_new / _present      insertVoxelsIntoVoxelMap(host arrays, T) likewise (76 bytes per record uploaded)
  set                               setRollingVoxelMap(host arrays) (88 bytes per voxel uploaded; host side: validation and the duplicate check)
  transform                         transformVoxelMap(T) of the map just restored
host_ms: time.perf_counter around the call (the record inserts leave their commit in the stream: the call returns after its second
synchronisation, which is before the commit).  device_ms: the engine's event time around the insert's kernels, commit included
(voxelRollingStats()['last_insert_ms'], which waits for the commit); `set` has no event pair, its device time is not measured.
T is a translation by whole voxels (3, -2, 1): every point and every record's mean moves to the same shifted voxel, so the scan
insert and the record inserts touch exactly V voxels each (a kernel's work does not depend on the values in T).  Medians and p10..p90
over --reps repetitions after --warmup discarded ones.

The 50-scan map: --scans VLP-16 scans of --points rays along a drive, inserted one by one (setInputSource + covariances + insert: what
a user who kept the scans pays to rebuild the map; the insert calls alone are reported beside it) against ONE setRollingVoxelMap of the
saved state.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES, PER_VOXEL = 0.5, 6


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _spd(n, rng):
    A = rng.normal(0, 0.05, (n, 3, 3))
    return A @ A.transpose(0, 2, 1) + 1e-4 * np.eye(3)


def synthetic(V, seed):
    """V distinct voxels around the origin at about 5 % fill; their records; a cloud with PER_VOXEL points in each"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil((V / 0.05) ** (1.0 / 3.0)))
    flat = rng.choice(side ** 3, V, replace=False)
    ijk = (np.stack([flat % side, (flat // side) % side, flat // side ** 2], 1) - side // 2).astype(np.int32)
    cnt = rng.integers(1, 13, V).astype(np.int32)
    mean = (ijk + rng.uniform(0.2, 0.8, (V, 3))) * RES
    S = mean * cnt[:, None]
    C = _spd(V, rng) * cnt[:, None, None]
    pts = ((np.repeat(ijk, PER_VOXEL, 0) + rng.uniform(0.2, 0.8, (V * PER_VOXEL, 3))) * RES).astype(np.float32)
    return ijk, S, C, cnt, np.ones(V, np.int64), np.ascontiguousarray(pts[rng.permutation(len(pts))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1600,16000,60000")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scans", type=int, default=50)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgicp_rollmap_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgicp_rollmap_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    T = clouds.make_pose((3 * RES, -2 * RES, 1 * RES)).astype(np.float32)
    out = {"metric": "rolling_map_record_routes_vs_scan_insert", "device": torch.cuda.get_device_name(0), "resolution": RES, "points_per_scan_voxel": PER_VOXEL,
           "reps": a.reps, "warmup": a.warmup, "sizes": {}}

    def handle():
        h = ng.NanoGICP()
        h.setCorrespondenceRandomness(20)
        h.setVoxelResolution(RES)
        h.setVoxelRolling(True)
        return h

    src, dst, prod = handle(), handle(), ng.NanoGICP()
    for V in [int(x) for x in a.sizes.split(",")]:
        ijk, S, C, cnt, st, pts = synthetic(V, 1000 + V)
        src.setRollingVoxelMap(ijk, S, C, cnt, st, 1)
        prod.setInputSource(pts); prod.calculateSourceCovariances()
        rec = {}

        def note(name, host, device=None):
            r = rec.setdefault(name, {"host_ms": [], "device_ms": []})
            r["host_ms"].append(host)
            if device is not None:
                r["device_ms"].append(device)

        counts = {}
        for rep in range(a.warmup + a.reps):
            keep = rep >= a.warmup
            routes = [("scan_insert", lambda: dst.insertIntoVoxelMap(prod, T)), ("insert_map", lambda: dst.insertVoxelMapFrom(src, T)),
                      ("insert_voxels", lambda: dst.insertVoxelsIntoVoxelMap(S, C, cnt, T))]
            for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
                dst.clearVoxelMap()
                for phase in ("new", "present"):
                    t, got = _timed(fn)
                    device = dst.voxelRollingStats()["last_insert_ms"]  # (waits for a record insert's commit: the next call does not pay for it)
                    counts[f"{name}_{phase}"] = [int(got[0]), int(got[1])]
                    if keep:
                        note(f"{name}_{phase}", t, device)
            t, _ = _timed(lambda: dst.setRollingVoxelMap(ijk, S, C, cnt, st, 1))
            if keep:
                note("set", t)
            t, left = _timed(lambda: dst.transformVoxelMap(T))
            device = dst.voxelRollingStats()["last_insert_ms"]
            if keep:
                note("transform", t, device)
            counts["transform"] = [int(left)]
        cell = {name: {k: _summ(v) for k, v in r.items() if v} for name, r in rec.items()}
        cell["created_touched"] = counts
        cell["scan_points"] = int(len(pts))
        for name in ("insert_map", "insert_voxels"):
            for phase in ("new", "present"):
                x, y = cell[f"{name}_{phase}"], cell[f"scan_insert_{phase}"]
                cell[f"{name}_{phase}"]["over_scan_insert"] = {k: x[k]["median_ms"] / y[k]["median_ms"] for k in ("host_ms", "device_ms")}
        out["sizes"][str(V)] = cell
        print(V, json.dumps(cell), file=sys.stderr, flush=True)

    # ---- a 50-scan map: re-inserting every scan against one restore ----
    if a.scans > 0:
        sc = clouds.make_scene()
        gts = [clouds.make_pose((-0.16 * (a.scans - 1) + 0.32 * i, 0.0, 0.0), (0.0, 0.0, 1.0 * i - 0.5 * a.scans)) for i in range(a.scans)]
        scans = [clouds.vlp16(sc, p, 400 + i, cols=a.points // 16) for i, p in enumerate(gts)]
        full, only = [], []
        for rep in range(6):
            dst.clearVoxelMap()
            t_full = t_only = 0.0
            for s, p in zip(scans, gts):
                t0, _ = _timed(lambda: (prod.setInputSource(s), prod.calculateSourceCovariances()))
                t1, _ = _timed(lambda: dst.insertIntoVoxelMap(prod, p.astype(np.float32)))
                t_full += t0 + t1
                t_only += t1
            full.append(t_full); only.append(t_only)
        saved, inserts = dst.rollingVoxelMap(), dst.voxelRollingStats()["inserts"]
        sets = [_timed(lambda: dst.setRollingVoxelMap(*saved, inserts))[0] for _ in range(7)][2:]
        again = dst.rollingVoxelMap()
        out["fifty_scan_map"] = {"scans": a.scans, "rays_per_scan": int(len(scans[0])), "map_voxels": int(len(saved[0])),
                                 "reinsert_upload_covariances_insert_ms": _summ(full[1:]), "reinsert_insert_calls_only_ms": _summ(only[1:]), "set_ms": _summ(sets),
                                 "restored_bit_equal": bool(all(np.array_equal(x, y) for x, y in zip(saved, again)))}
        out["fifty_scan_map"]["reinsert_over_set"] = {"with_upload_and_covariances": float(np.median(full[1:]) / np.median(sets)),
                                                      "insert_calls_only": float(np.median(only[1:]) / np.median(sets))}
        print("fifty_scan_map", json.dumps(out["fifty_scan_map"]), file=sys.stderr, flush=True)
    for h in (src, dst, prod):
        h.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
