"""Child process of tests/test_gpu_terminal_pass.py: every scenario of that module under the NGICP_FULL_LAST_PASS its environment carries
(read at ngicp_create; the parent runs this once without it and once with NGICP_FULL_LAST_PASS=1 and compares the two outputs).
The last line is RESULT {json}: per scenario the results as hex strings (bit-exact comparison) and the statistics.
usage: python tests/_terminal_pass_worker.py main
       python tests/_terminal_pass_worker.py sharded <port>     (a real RCCL group of one rank, as tests/_sharded_rccl_worker.py)
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np

EPS12 = dict(setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)
REJECTION_LIMIT = 6  # (tests/test_gpu_terminal_pass.py, test_rejected_trial_in_the_last_outer_iteration)


def shapes():
    from direct_lidar_odometry_amd import clouds
    small = clouds.scan_to_scan(5000)
    big = clouds.scan_to_scan(10_000)
    return {"2k_5k": (np.ascontiguousarray(small.source[::2][:2000]), small.target, small.guess),
            "10k_10k": (big.source, big.target, big.guess)}


def _hex(a):
    return np.ascontiguousarray(a).tobytes().hex()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(g):
    T = g.getFinalTransformation().copy()
    tr = g.lm_trace().copy()
    corr, sqd = g.correspondences()
    s = g.stats()
    # (ngicp_compute_error wants a linearize hook before it, which would replace the very state in question: robust_terms gives the terms
    # e^T M e of that error at the final pose, straight from the persisted correspondences and Mahalanobis matrices)
    terms, _ = g.robust_terms(T)
    return dict(T=_hex(T), H=_hex(g.getFinalHessian()), converged=bool(g.converged_), iters=int(g.nr_iterations_), trace=_hex(tr),
                trace_rows=[[int(r[0]), int(r[1]), int(r[7])] for r in tr], corr=_sha(corr), sqd=_sha(sqd), n_corr=int((corr >= 0).sum()),
                err=_hex(np.float64(terms[terms >= 0].sum())), terms=_sha(terms), passes=int(s["passes"]), search_passes=int(s["search_passes"]), lm_trials=int(s["lm_trials"]),
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


def read_costs(path):
    """NGICP_DEBUG_COSTS' dump: [n] costs, [n] launch order (ints), [n][32] partial rows (doubles)."""
    raw = open(path, "rb").read()
    n = len(raw) // (2 * 4 + 32 * 8)
    ints = np.frombuffer(raw[:8 * n], np.int32)
    return ints[:n].copy(), ints[n:].copy()


def main_scenarios(ng):
    out = {}
    for shape, (src, tgt, guess) in shapes().items():
        def run(name, g, T0=guess, close=True):
            g.align(np.asarray(T0, np.float32))
            out[f"{shape}/{name}"] = record(g)
            if close:
                g.close()

        for m in (1, 2, 5):  # the iteration limit (and the statistics of a two-pass alignment, m = 1)
            run(f"limit{m}", handle(ng, src, tgt, setMaximumIterations=m, **EPS12))
        run("epsilon", handle(ng, src, tgt, k=10, setMaximumIterations=32, setTransformationEpsilon=0.01))  # DLO's scan-to-scan settings
        if shape == "10k_10k":
            run("rejection", handle(ng, src, tgt, setMaximumIterations=REJECTION_LIMIT, **EPS12))
        for lm in (1, 2):
            run(f"lm_max{lm}", handle(ng, src, tgt, setMaximumIterations=REJECTION_LIMIT, setLMMaxIterations=lm, **EPS12))
        run("gauss_newton", handle(ng, src, tgt, setOptimizer=0, setMaximumIterations=15))
        g = handle(ng, src, tgt, setMaximumIterations=5, **EPS12)
        g.setRobustKernel(ng.RobustKernel.HUBER, 1.0)
        run("huber", g)
        g = handle(ng, src, tgt, setMaximumIterations=3, **EPS12)
        g.align(np.asarray(guess, np.float32))
        g.swapSourceAndTarget()
        run("swapped", g, np.linalg.inv(np.asarray(guess, np.float64)).astype(np.float32))
        # two alignments in a row on one handle; after the first, the launch order its successor's first pass will read
        g = handle(ng, src, tgt, setMaximumIterations=5, **EPS12)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "costs.bin")
            os.environ["NGICP_DEBUG_COSTS"] = path
            try:
                run("first_of_two", g, close=False)
            finally:
                del os.environ["NGICP_DEBUG_COSTS"]
            costs, order = read_costs(path)
        out[f"{shape}/first_of_two"].update(costs=costs.tolist(), order=order.tolist())
        run("second_of_two", g)
    return out


def sharded_scenarios(ng, port):
    import torch
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    torch.cuda.set_device(0)
    from direct_lidar_odometry_amd import sharding
    src, tgt, guess = shapes()["10k_10k"]
    out = {}
    for name, settings in (("sharded_epsilon", dict()), ("sharded_limit2", dict(setMaximumIterations=2, **EPS12))):
        full = handle(ng, src, tgt, **settings)
        full.align(np.asarray(guess, np.float32))
        e = handle(ng, src, tgt, **settings)
        e.setSourceCovariances(full.getSourceCovariances())
        e.setTargetCovariances(full.getTargetCovariances())
        T = sharding.sharded_align(e, np.asarray(guess, np.float32), dist, "cuda:0")
        s = e.stats()
        out[f"10k_10k/{name}"] = dict(T=_hex(T), H=_hex(e.getFinalHessian()), converged=bool(e.converged_), iters=int(e.nr_iterations_),
                                      passes=int(s["passes"]), search_passes=int(s["search_passes"]), lm_trials=int(s["lm_trials"]),
                                      equals_align=bool(np.array_equal(T, full.getFinalTransformation()) and np.array_equal(e.getFinalHessian(), full.getFinalHessian())),
                                      align_passes=int(full.stats()["passes"]))
        e.close()
        full.close()
    dist.destroy_process_group()
    return out


def main():
    from direct_lidar_odometry_amd import nano_gicp
    if sys.argv[1] == "sharded":
        out = sharded_scenarios(nano_gicp, int(sys.argv[2]))  # (the process group comes up before anything else touches the GPU)
    else:
        nano_gicp.load_library()
        out = main_scenarios(nano_gicp)
    print("RESULT " + json.dumps({"full_last_pass": os.environ.get("NGICP_FULL_LAST_PASS", ""), "scenarios": out}), flush=True)


if __name__ == "__main__":
    main()
