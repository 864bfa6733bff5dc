"""Child process of tests/test_gpu_far_units.py: its sandwich and ties cases under the process-wide kernel variant the environment
selects (see tests/_variant_worker.py).  A failed check raises (non-zero exit); on success the last line is RESULT {json}."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    from direct_lidar_odometry_amd import nano_gicp
    from oracle import oracle as orc
    import test_gpu_far_units as t

    nano_gicp.load_library()
    switches = ("NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_ORDER", "NGICP_PASS_WPS")
    variant = {k: os.environ[k] for k in switches if k in os.environ}
    rig = t.sandwich_rig(nano_gicp, orc)
    out = rig.run(t.fc.GUESS, f"sandwich {variant}", fresh=False)
    staged = rig.g.stats()["staged_fraction"]
    first = rig.first_align_stats(t.fc.GUESS)["staged_fraction"]
    rig.g.close()
    assert 2 <= len(out) <= 6 and staged > 0.0 and first > 0.0, (len(out), staged, first)
    t.check_ties(nano_gicp, {})
    print("RESULT " + json.dumps({"variant": variant, "passes": len(out), "staged": staged, "first": first}), flush=True)


if __name__ == "__main__":
    main()
