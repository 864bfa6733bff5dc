"""Child process of tests/test_gpu_pose_prior.py: an exact-route align with a pose prior set under the process-wide kernel-variant switch
its environment carries (NGICP_PASS_IMPL, NGICP_FUSED, NGICP_QUEUE, NGICP_PERSIST, NGICP_HEAD, NGICP_SERIAL_STEP: read once per process or per handle by the two readers of ngicp_route.h,
so each needs a process of its own - tests/_robust_worker.py's pattern).  The file named on the command line holds what the DEFAULT
route returned for the same inputs with the prior (T, trace, H) and without it (T0).  Either the align is refused with NGICP_ERR_ARG
naming the pose prior - then the setting must stay and, the prior cleared, the align under the switch must equal T0 - and the last
line is RESULT refused; or its result must equal the default route's, bit for bit, and the last line is RESULT applied.  Anything else
- a switch that ignores the prior included - raises (non-zero exit).
usage: python tests/_pose_prior_worker.py default_route.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def setup(nano_gicp, clouds):
    """the inputs, shared with the parent: (engine, workload, prior pose, information matrix)"""
    import numpy as np
    w = clouds.scan_to_scan(2000)
    g = nano_gicp.NanoGICP()
    g.setMaxCorrespondenceDistance(1.0)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    Tp = (clouds.make_pose((0.05, -0.04, 0.02), (0.5, -0.3, 1.0)) @ np.asarray(w.guess, np.float64))
    A = np.random.default_rng(4).normal(size=(6, 6))
    return g, w, Tp, 2e3 * (A @ A.T)


def outcome(g, w):
    g.align(w.guess)
    return g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy()


def main():
    import numpy as np
    from direct_lidar_odometry_amd import clouds, nano_gicp

    switches = ("NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_PERSIST", "NGICP_HEAD", "NGICP_SERIAL_STEP")
    variant = {k: os.environ[k] for k in switches if k in os.environ}
    assert variant, "no kernel-variant switch in the environment"
    with np.load(sys.argv[1]) as z:
        want = (z["T"], z["trace"], z["H"])
        T0 = z["T0"]
    g, w, Tp, Lam = setup(nano_gicp, clouds)
    g.setPosePrior(Tp, Lam)
    try:
        got = outcome(g, w)
    except nano_gicp.NgicpError as e:
        assert e.code == -2 and "pose prior" in str(e), str(e)
        print(f"{variant}: {e}", flush=True)
        assert g.getPosePrior() is not None and np.array_equal(g.getPosePrior()[1], Lam)
        g.clearPosePrior()
        assert np.array_equal(outcome(g, w)[0], T0), f"{variant}: the align without a prior differs from the default route's"
        g.close()
        print("RESULT refused", flush=True)
        return
    for name, a, b in zip(("T", "trace", "H"), got, want):
        assert np.array_equal(a, b), f"{variant}: {name} differs from the default route's with the prior" + (
            " - and equals its result WITHOUT the prior: the switch ignores the prior" if name == "T" and np.array_equal(a, T0) else "")
    g.close()
    print("RESULT applied", flush=True)


if __name__ == "__main__":
    main()
