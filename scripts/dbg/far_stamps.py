"""Where the slowest waves of a pass spend their time around the listed-row ("far") section (NGICP_DEBUG_STAMPS + NGICP_DEBUG_SPAN): the
ring-1 drain (stamps 16 -> 17), the far section (4 -> 5) and, with a library built with -DNGICP_FAR_STAMPS (NGICP_LIB), its two parts
(queueing / draining), units and rounds.  For the slowest twentieth of the waves of the last searching pass of a warm alignment and of
the cold first pass.
usage: python scripts/dbg/far_stamps.py [c3|c5] [out.json]"""
import json, os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from direct_lidar_odometry_amd import clouds
from direct_lidar_odometry_amd.nano_gicp import NanoGICP, keyframe_covariances

cfg = sys.argv[1] if len(sys.argv) > 1 else "c3"
out = sys.argv[2] if len(sys.argv) > 2 else None
w = clouds.scan_to_submap(100_000, 5) if cfg == "c3" else clouds.scan_to_submap(250_000, 8, shape="os1")
dump_dir = tempfile.mkdtemp(prefix="far_stamps_")  # the raw stamp and span dumps


def pct(x):
    return [float(v) for v in np.percentile(x, [50, 90, 100])] if len(x) else None


def section(raw, span, label, tpu_known):
    a = raw[raw[:, 2] > 0].astype(np.float64)  # waves that searched
    r = raw[raw[:, 2] > 0]
    # ticks of the stamps' clock per microsecond: a block's life on the 100 MHz counter against its waves' first and last stamp
    blk = raw.reshape(-1, 4, 24)[: len(span)]
    ok = (span[:, 1] > 0) & (blk[:, :, 0].min(axis=1) > 0) & (blk[:, :, 9].max(axis=1) > blk[:, :, 0].min(axis=1))
    life_us = (span[ok, 1].astype(np.float64) - span[ok, 0].astype(np.float64)) / 100.0
    life_tk = blk[ok][:, :, 9].max(axis=1).astype(np.float64) - blk[ok][:, :, 0].min(axis=1).astype(np.float64)
    tpu = tpu_known or float(np.median(life_tk / np.maximum(life_us, 1e-3)))
    search = a[:, 8] - a[:, 1]  # the wave's life up to its reduction (from stamp 1: a pass that only ends the alignment rewrites stamp 0)
    slow = search >= np.percentile(search, 95)
    far = a[:, 5] - a[:, 4]
    res = {"label": label, "waves": int(len(a)), "ticks_per_us": tpu, "slowest_twentieth": int(slow.sum())}
    for name, m in (("all", np.ones(len(a), bool)), ("slow", slow), ("slow_and_far", slow & (r[:, 21] > 0))):
        e = {"n": int(m.sum()),
             "wave_life_1_8_ticks_p50_p90_max": pct(search[m]),
             "ring1_drain_16_17_ticks_p50_p90_max": pct((a[:, 17] - a[:, 16])[m]),
             "far_4_5_ticks_p50_p90_max": pct(far[m]),
             "far_4_5_us_p50_p90_max": [v / tpu for v in pct(far[m])] if m.any() else None,
             "ring1_units_p50_p90_max": pct(a[m, 19]), "ring1_max_popped_by_a_lane_p50_p90_max": pct(a[m, 18]),
             "live_rows_p50_p90_max": pct(a[m, 11])}
        if (r[:, 21] > 0).any():  # the diagnostic build's words
            enq = (r[:, 20] & np.uint64((1 << 40) - 1)).astype(np.float64); units = (r[:, 20] >> np.uint64(40)).astype(np.float64)
            drn = (r[:, 21] & np.uint64((1 << 48) - 1)).astype(np.float64); rounds = (r[:, 21] >> np.uint64(48)).astype(np.float64)
            e.update({"far_enqueue_ticks_p50_p90_max": pct(enq[m]), "far_drain_ticks_p50_p90_max": pct(drn[m]),
                      "far_enqueue_us_p50_p90_max": [v / tpu for v in pct(enq[m])] if m.any() else None,
                      "far_drain_us_p50_p90_max": [v / tpu for v in pct(drn[m])] if m.any() else None,
                      "far_units_p50_p90_max": pct(units[m]), "far_rounds_p50_p90_max": pct(rounds[m]),
                      "share_with_far_section": float((rounds[m] > 0).mean()) if m.any() else None})
        res[name] = e
    print(json.dumps(res), flush=True)
    return res


def run(cold, tpu_known=None):
    # warm: the stamped (last) pass must search, and be the pass the block spans are of; cold: the pass after the first only ends the
    # alignment and leaves the first pass's stamps (all but stamp 0) as they are
    if cold:
        os.environ.pop("NGICP_FULL_LAST_PASS", None)
    else:
        os.environ["NGICP_FULL_LAST_PASS"] = "1"
    g = NanoGICP()
    g.setMaxCorrespondenceDistance(w.max_corr_dist)
    g.setMaximumIterations(20); g.setTransformationEpsilon(1e-12); g.setRotationEpsilon(1e-12)
    if cold:  # the FIRST pass of an alignment (no previous correspondences): one Gauss-Newton iteration
        g.setOptimizer(0); g.setMaximumIterations(1)
    g.setInputTarget(w.target); g.setInputSource(w.source)
    g.setTargetCovariances(keyframe_covariances(w.target, w.keyframe_sizes, 20))
    g.calculateSourceCovariances()
    for _ in range(3):
        g.align(w.guess)
    tag = f"{cfg}_{'cold' if cold else 'warm'}"
    sf, pf = os.path.join(dump_dir, f"stamps_{tag}.bin"), os.path.join(dump_dir, f"span_{tag}.bin")
    os.environ["NGICP_DEBUG_STAMPS"], os.environ["NGICP_DEBUG_SPAN"] = sf, pf
    g.align(w.guess)
    del os.environ["NGICP_DEBUG_STAMPS"], os.environ["NGICP_DEBUG_SPAN"]
    s = g.stats()
    print(f"{tag}: align {s['align_ms']:.3f} ms loop {s['loop_ms']:.3f} passes {s['passes']} staged {s['staged_fraction']:.3f}", flush=True)
    raw = np.fromfile(sf, dtype=np.uint64).reshape(-1, 24)
    span = np.fromfile(pf, dtype=np.uint64).reshape(-1, 4)
    g.close()
    return section(raw, span, tag, tpu_known)


warm = run(False)
results = [warm, run(True, warm["ticks_per_us"])]
if out:
    with open(out, "w") as f:
        json.dump(results, f, indent=1)
