"""Child process of tests/test_gpu_variants.py: the per-pass oracle checks of _pass_check.py under the process-wide kernel variant
its environment selects (NGICP_PASS_IMPL, NGICP_FUSED, NGICP_QUEUE, NGICP_ORDER, NGICP_PASS_WPS: read once per process by ngicp_route.h's read_process_switches, so each
variant needs a process of its own).  A failed check raises (non-zero exit); on success the last line is RESULT {json}.
usage: python tests/_variant_worker.py <case> [<case> ...]   (cases: _pass_check.make_rig's names)
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    from direct_lidar_odometry_amd import nano_gicp
    from oracle import oracle as orc
    from _pass_check import make_rig

    nano_gicp.load_library()
    switches = ("NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_ORDER", "NGICP_PASS_WPS")
    variant = {k: os.environ[k] for k in switches if k in os.environ}
    out = {"variant": variant, "lib": nano_gicp._LIB_PATH, "cases": {}}
    for case in sys.argv[1:]:
        t0 = time.time()
        rig, guess = make_rig(nano_gicp, orc, case)
        per_pass = rig.run(guess, f"{case} {variant}")
        out["cases"][case] = {"passes": len(per_pass), "ties": [t[0] for t in per_pass], "seconds": round(time.time() - t0, 1)}
        rig.g.close()
        print(f"{case}: {len(per_pass)} passes checked in {time.time() - t0:.1f} s", flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
