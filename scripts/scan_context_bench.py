"""Scan context (k_sc_build / k_sc_norms / k_sc_match / k_sc_topk) against what a caller had without it - a vectorised
numpy implementation of the same definition on the host - all in one process, warmed, the compared routes alternating repetition by
repetition.

  python scripts/scan_context_bench.py [--points 5k,100k] [--entries 100,1000,10000] [--top-k 8] [--reps 15] [--warmup 3]
                                       [--out profiles/scan_context_bench.json]
one JSON line on stdout (and in --out).

build, per cloud size (a clouds.vlp16 scan of that many points, already the source of the handle):
  device       computeScanContext(0): the descriptor built on the device, R x S floats read back
  numpy        the same descriptor from the host copy of the cloud (np.maximum.at over vectorised ring / sector counts, the engine's tables)
match, per database size (entries: rolled and rescaled copies of real scan descriptors, added as host descriptors), top_k as given:
  device_descriptor   matchScanContext(Q, 0, N, top_k) with a host descriptor as the query
  device_slot         matchScanContext(0, 0, N, top_k): the query is the source cloud (3 008 points), its descriptor built in the same call
  numpy               all N x S shift distances through one batched matrix product in double, the minimum, an argpartition and a sort
host_ms: time.perf_counter around the call, host to host.  kernel_ms: the engine's event time around the call's kernels
(scanContextKernelMs()).  Medians with p10 .. p90 over --reps repetitions after --warmup discarded ones (the numpy match at 10 000 entries
runs a third of them).  The numpy routes reorder the sums, so their distances agree with the engine's to rounding, not bit for bit; the
script checks ids and shifts of the top_k and the distances to 1e-9 before it reports anything.  GFLOPs: 2 R S S flops per candidate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
SIZES = {"5k": 5_000, "100k": 100_000}


def _summ(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def numpy_descriptor(p, E2, b, z0):
    """the definition on the host, vectorised over the points and the table entries"""
    R, half = len(E2) - 1, len(b)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r2 = x * x + y * y
    keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (r2 < E2[R])
    x, y, z, r2 = x[keep], y[keep], z[keep], r2[keep]
    ring = (r2[:, None] >= E2[None, 1:R]).sum(axis=1)
    low = (y < 0) | ((y == 0) & (x < 0))
    xs, ys = np.where(low, -x, x), np.where(low, -y, y)
    cross = b[None, 1:, 0] * ys[:, None] - b[None, 1:, 1] * xs[:, None]
    sector = (cross >= 0).sum(axis=1) + np.where(low, half, 0)
    D = np.zeros((R, 2 * half), dtype=F)
    np.maximum.at(D, (ring, sector), z + F(z0))
    return D


def numpy_match(Q, db, db_norm, top_k):
    """Q (R, S), db (N, R, S) float32, db_norm (N, S) float64 -> (ids, dist, shift) of the top_k"""
    N, R, S = db.shape
    Q64 = Q.astype(np.float64)
    nq = np.sqrt((Q64 * Q64).sum(axis=0))
    dots = np.matmul(Q64.T[None], db.astype(np.float64))          # [N][j][j']
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dots / (nq[None, :, None] * db_norm[:, None, :])
    ok = (nq[None, :, None] > 0) & (db_norm[:, None, :] > 0)
    cos = np.where(ok, cos, 0.0)
    j = np.arange(S)
    jp = (j[None, :] + j[:, None]) % S                            # [k][j] -> j'
    total = cos[:, j[None, :], jp].sum(axis=2)                    # [N][k]
    m = ok[:, j[None, :], jp].sum(axis=2)
    d = np.where(m > 0, 1.0 - total / np.maximum(m, 1), 1.0)
    dist, shift = d.min(axis=1), d.argmin(axis=1)
    k = min(top_k, N)
    part = np.argpartition(dist, k - 1)[:k] if k < N else np.arange(N)
    order = part[np.lexsort((part, dist[part]))]
    return order, dist[order], shift[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="5k,100k")
    ap.add_argument("--entries", default="100,1000,10000")
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_context_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scan_context_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()

    g = ng.NanoGICP()
    R, S, L, z0 = g.getScanContextParams()
    E2, b = g.scanContextTables()
    scene = clouds.make_scene()
    out = {"metric": "scan_context_device_vs_numpy", "device": torch.cuda.get_device_name(0), "params": [R, S, float(L), float(z0)], "top_k": a.top_k,
           "reps": a.reps, "warmup": a.warmup, "build": {}, "match": {}}

    for size in a.points.split(","):
        n = SIZES[size]
        scan = clouds.vlp16(scene, clouds.make_pose((1.0, -2.0, 0.0), (0.0, 0.0, 20.0)), noise_seed=77, cols=n // 16)
        g.setInputSource(scan)
        assert np.array_equal(g.computeScanContext(0), numpy_descriptor(scan, E2, b, z0))
        rec = {"device": {"host_ms": [], "kernel_ms": []}, "numpy": {"host_ms": []}}
        for rep in range(a.warmup + a.reps):
            routes = [("device", lambda: g.computeScanContext(0)), ("numpy", lambda: numpy_descriptor(scan, E2, b, z0))]
            for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
                t, _ = _timed(fn)
                if rep >= a.warmup:
                    rec[name]["host_ms"].append(t)
                    if name == "device":
                        rec[name]["kernel_ms"].append(g.scanContextKernelMs())
        cell = {name: {k: _summ(v) for k, v in r.items()} for name, r in rec.items()}
        cell["n_points"] = int(len(scan))
        cell["numpy_over_device_host"] = cell["numpy"]["host_ms"]["median_ms"] / cell["device"]["host_ms"]["median_ms"]
        out["build"][size] = cell
        print("build", size, json.dumps(cell), file=sys.stderr, flush=True)

    # the database: real descriptors along a drive, rolled and rescaled into as many distinct entries as asked for
    poses = [clouds.make_pose((-15.0 + 30.0 * i / 11, 8.0 * np.sin(2.0 * np.pi * i / 11), 0.0), (0.0, 0.0, 15.0 * i)) for i in range(12)]
    base = [numpy_descriptor(clouds.vlp16(scene, T, noise_seed=500 + i, cols=188), E2, b, z0) for i, T in enumerate(poses)]
    query_scan = clouds.vlp16(scene, poses[7] @ clouds.make_pose((0.32, 0.24, 0.0), (0.0, 0.0, 37.0)), noise_seed=907, cols=188)
    Q = numpy_descriptor(query_scan, E2, b, z0)
    rng = np.random.default_rng(5)
    n_max = max(int(x) for x in a.entries.split(","))
    db = np.stack([base[i % 12] if i < 12 else (np.roll(base[i % 12], int(rng.integers(0, S)), axis=1) * F(rng.uniform(0.8, 1.2))).astype(F) for i in range(n_max)])
    for d in db:
        g.addScanContextDescriptor(d)
    db64 = db.astype(np.float64)
    db_norm = np.sqrt((db64 * db64).sum(axis=1))
    g.setInputSource(query_scan)
    for N in [int(x) for x in a.entries.split(",")]:
        ids, dist, shift = g.matchScanContext(Q, 0, N, a.top_k)
        nids, ndist, nshift = numpy_match(Q, db[:N], db_norm[:N], a.top_k)
        assert ids.tolist() == nids.tolist() and shift.tolist() == nshift.tolist() and np.abs(dist - ndist).max() <= 1e-9, (N, ids, nids)
        reps_np = a.reps if N < 10_000 else max(3, a.reps // 3)
        rec = {"device_descriptor": {"host_ms": [], "kernel_ms": []}, "device_slot": {"host_ms": [], "kernel_ms": []}, "numpy": {"host_ms": []}}
        for rep in range(a.warmup + a.reps):
            routes = [("device_descriptor", lambda: g.matchScanContext(Q, 0, N, a.top_k)), ("device_slot", lambda: g.matchScanContext(0, 0, N, a.top_k))]
            if rep < a.warmup + reps_np:
                routes.append(("numpy", lambda: numpy_match(Q, db[:N], db_norm[:N], a.top_k)))
            for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
                t, _ = _timed(fn)
                if rep >= a.warmup:
                    rec[name]["host_ms"].append(t)
                    if name != "numpy":
                        rec[name]["kernel_ms"].append(g.scanContextKernelMs())
        cell = {name: {k: _summ(v) for k, v in r.items()} for name, r in rec.items()}
        k_ms = cell["device_descriptor"]["kernel_ms"]["median_ms"]
        cell["match_GFLOPs"] = 2.0 * R * S * S * N / (k_ms * 1e-3) / 1e9
        cell["numpy_over_device_host"] = cell["numpy"]["host_ms"]["median_ms"] / cell["device_descriptor"]["host_ms"]["median_ms"]
        cell["top_1"] = {"id": int(ids[0]), "distance": float(dist[0]), "shift": int(shift[0])}
        out["match"][str(N)] = cell
        print("match", N, json.dumps(cell), file=sys.stderr, flush=True)
    g.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
