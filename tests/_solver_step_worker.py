"""Child process of tests/test_gpu_solver_step.py: small alignments under the switches its environment carries (NGICP_SERIAL_STEP is
read at ngicp_create by ngicp_route.h's read_handle_switches, NGICP_FUSED once per process by its read_process_switches; the parent runs this with and without NGICP_SERIAL_STEP=1 and compares the outputs).
The last line is RESULT {json}: per scenario the results as hex strings (bit-exact comparison) and the counters that measure no time.
usage: python tests/_solver_step_worker.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np

EPS12 = dict(setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)


def _hex(a):
    return np.ascontiguousarray(a).tobytes().hex()


def record(g):
    tr = g.lm_trace().copy()
    s = g.stats()
    return dict(T=_hex(g.getFinalTransformation()), H=_hex(g.getFinalHessian()), converged=bool(g.converged_), iters=int(g.nr_iterations_),
                trace=_hex(tr), trace_rows=[[int(r[0]), int(r[1]), int(r[7])] for r in tr], passes=int(s["passes"]),
                search_passes=int(s["search_passes"]), outer_iterations=int(s["outer_iterations"]), lm_trials=int(s["lm_trials"]),
                valid_fraction=float(s["valid_fraction"]), mean_candidates=float(s["mean_candidates"]), staged_fraction=float(s["staged_fraction"]))


def handle(ng, src, tgt, k=20, gate=1.0, **settings):
    g = ng.NanoGICP()
    g.setCorrespondenceRandomness(k)
    g.setMaxCorrespondenceDistance(gate)
    for name, v in settings.items():
        getattr(g, name)(v)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    return g


def main():
    from direct_lidar_odometry_amd import clouds, nano_gicp as ng
    ng.load_library()
    small, mid, big = clouds.scan_to_scan(5000), clouds.scan_to_scan(10_000), clouds.scan_to_scan(30_000)
    robust = not any(os.environ.get(k, "0") not in ("", "0") for k in ("NGICP_FUSED", "NGICP_PERSIST"))  # (those pass variants have no robust build)
    shapes = {"2k_5k": (np.ascontiguousarray(small.source[::2][:2000]), small.target, small.guess), "30k_30k": (big.source, big.target, big.guess)}
    far = clouds.make_pose((3, -2, 0.5), (5, -5, 25))  # on top of the guess: a long way off
    out = {}
    for shape, (src, tgt, guess) in shapes.items():
        def run(name, g, T0=guess):
            g.align(np.asarray(T0, np.float32))
            out[f"{shape}/{name}"] = record(g)
            g.close()

        with tempfile.TemporaryDirectory() as tmp:  # the number of groups, from the diagnostic dump of their costs
            path = os.path.join(tmp, "costs.bin")
            os.environ["NGICP_DEBUG_COSTS"] = path
            try:
                run("dlo", handle(ng, src, tgt, k=10, setMaximumIterations=32, setTransformationEpsilon=0.01))
            finally:
                del os.environ["NGICP_DEBUG_COSTS"]
            out[f"{shape}/dlo"]["groups"] = os.path.getsize(path) // (2 * 4 + 32 * 8)
        run("eps12", handle(ng, src, tgt, setMaximumIterations=20, **EPS12))
        run("gauss_newton", handle(ng, src, tgt, setOptimizer=0, setMaximumIterations=15))
        run("one_iteration", handle(ng, src, tgt, setMaximumIterations=1))
        off = (far @ np.asarray(guess, np.float64)).astype(np.float32)
        run("far_guess", handle(ng, src, tgt, gate=2.0, setMaximumIterations=20, **EPS12), off)
        run("far_guess_lm_max1", handle(ng, src, tgt, gate=2.0, setMaximumIterations=20, setLMMaxIterations=1, **EPS12), off)
        if robust:
            g = handle(ng, src, tgt, setMaximumIterations=5, **EPS12)
            g.setRobustKernel(ng.RobustKernel.HUBER, 1.0)
            run("huber", g)
    # trials rejected one after the other (eps 1e-12: the last outer iterations of this pair reject several times before they accept)
    shape, (src, tgt, guess) = "10k_10k", (mid.source, mid.target, mid.guess)
    for name, lm in (("rejections", 10), ("rejections_lm_max2", 2)):
        g = handle(ng, src, tgt, setMaximumIterations=20, setLMMaxIterations=lm, **EPS12)
        g.align(np.asarray(guess, np.float32))
        out[f"{shape}/{name}"] = record(g)
        g.close()
    print("RESULT " + json.dumps({"serial_step": os.environ.get("NGICP_SERIAL_STEP", ""), "scenarios": out}), flush=True)


if __name__ == "__main__":
    main()
