"""Timing of the device-side range median (include/ngicp.h "range select") against what a caller does without it.

  python scripts/range_bench.py            one JSON line on stdout, the same object in profiles/range_bench.json
Kernel times: run it once under  rocprofv3 --kernel-trace --stats -- python scripts/range_bench.py --once  (a run of its own).

At 20k, 100k and 262 144 points (an OS1-128 frame), medians over 50 calls:
  device          ngicp_range_median on the preprocessed scan that ngicp_preprocess_scan(..., out = NULL) left on the device: host to
                  host, and the device time of its kernels (ngicp_stats.query_ms)
  host_route      what a caller does today: the download of the same cloud (ngicp_preprocess_scan with an output buffer, minus the
                  same call without one: the call's other work is the same), plus the ranges and their median on the host -
                  numpy (float64 squares, sqrt, astype(float32), np.partition), ONE thread; the reference's loop + std::nth_element
                  is the same work in C++ and was not measured
The scan is preprocessed with remove_nan only (no crop, no voxel filter), so the filtered cloud has the size asked for.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (20_000, 100_000, 262_144)
CALLS = 50


def _median_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def _host_median(xyzi):
    x, y, z = xyzi[:, 0].astype(np.float64), xyzi[:, 1].astype(np.float64), xyzi[:, 2].astype(np.float64)
    d = np.sqrt(x * x + y * y + z * z).astype(np.float32)
    return np.partition(d, len(d) // 2)[len(d) // 2]


def _case(ng, clouds, n, calls):
    scene = clouds.make_scene()
    scan = clouds.os1_128(scene, clouds.make_pose(), noise_seed=1, n=250_000)
    if n > len(scan):
        scan = np.concatenate([scan, clouds.os1_128(scene, clouds.make_pose(t=(0.5, 0.2, 0.0)), noise_seed=2, n=n - len(scan))])
    cloud = clouds.to_xyzi(np.ascontiguousarray(scan[:n]))
    g = ng.NanoGICP()
    L, h = g._L, g._h
    out = np.empty((n, 4), np.float32)
    m = C.c_size_t(0)
    ptr = cloud.ctypes.data_as(ng.c_f32p)

    def preprocess(download):
        g._ck(L.ngicp_preprocess_scan(h, ptr, n, cloud.strides[0], 16, 1, 0.0, 0.0, out.ctypes.data_as(ng.c_f32p) if download else None, n, C.byref(m)))

    preprocess(True)
    assert m.value == n
    want = _host_median(out)
    v = C.c_float(0)

    def device():
        g._ck(L.ngicp_range_median(h, 2, C.byref(v), None))

    device()
    assert np.float32(v.value).view(np.uint32) == want.view(np.uint32)
    host, dev = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        device()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(g.stats()["query_ms"])
    with_dl = _median_ms(lambda: preprocess(True), calls)
    without_dl = _median_ms(lambda: preprocess(False), calls)
    host_median_ms = _median_ms(lambda: _host_median(out), calls)
    g.close()
    download = max(with_dl - without_dl, 0.0)
    return {"points": n, "calls": calls, "median_range": float(want),
            "device": {"host_to_host_median_ms": float(np.median(host)), "host_to_host_p99_ms": float(np.percentile(host, 99)), "query_ms_median": float(np.median(dev))},
            "host_route": {"preprocess_with_download_ms": with_dl, "preprocess_without_download_ms": without_dl, "download_ms": download,
                           "numpy_ranges_and_partition_ms": host_median_ms, "total_ms": download + host_median_ms,
                           "label": "numpy, one thread: float64 squares + sqrt + astype(float32) + np.partition; not the reference's C++ loop"}}


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("range_bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    from direct_lidar_odometry_amd import build, clouds, nano_gicp as ng
    build.build()
    once = "--once" in sys.argv
    out = {"metric": "range_median", "device": torch.cuda.get_device_name(0)}
    for n in SIZES:
        out[f"n{n}"] = _case(ng, clouds, n, 3 if once else CALLS)
    line = json.dumps(out)
    if not once:
        with open(os.path.join(ROOT, "profiles", "range_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
