"""Child process of tests/test_gpu_robust.py: an exact-route align with a robust kernel set under the process-wide kernel-variant switch
its environment carries (NGICP_PASS_IMPL, NGICP_FUSED, NGICP_QUEUE, NGICP_PERSIST, NGICP_HEAD: read once per process or per handle by the two readers of ngicp_route.h, so each needs a
process of its own - tests/_variant_worker.py's pattern).  The align must be refused with NGICP_ERR_ARG naming the robust kernel, the
setting must stay, and with NONE the align under the same switch must equal the one before the kernel was set, bit for bit.  A failed
check raises (non-zero exit); on success the last line is RESULT refused.
usage: python tests/_robust_worker.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import numpy as np
    from direct_lidar_odometry_amd import clouds, nano_gicp

    switches = ("NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_PERSIST", "NGICP_HEAD")
    variant = {k: os.environ[k] for k in switches if k in os.environ}
    assert variant, "no kernel-variant switch in the environment"
    w = clouds.scan_to_scan(2000)
    g = nano_gicp.NanoGICP()
    g.setMaxCorrespondenceDistance(1.0)
    g.setInputSource(w.source); g.setInputTarget(w.target)

    def outcome():
        g.align(w.guess)
        return g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy()

    want = outcome()
    g.setRobustKernel(nano_gicp.RobustKernel.HUBER, 1.5)
    try:
        g.align(w.guess)
    except nano_gicp.NgicpError as e:
        assert e.code == -2 and "robust" in str(e), str(e)
        print(f"{variant}: {e}", flush=True)
    else:
        raise AssertionError(f"{variant}: the align was not refused")
    assert g.getRobustKernel() == (nano_gicp.RobustKernel.HUBER, 1.5)
    g.setRobustKernel(nano_gicp.RobustKernel.NONE)
    for a, b in zip(outcome(), want):
        assert np.array_equal(a, b), f"{variant}: the align without a kernel changed"
    g.close()
    print("RESULT refused", flush=True)


if __name__ == "__main__":
    main()
