"""The shared guess set of the batched-alignment tests (test_batch_cases_cpu.py, test_gpu_batch.py): one scan-to-submap pair and
twelve initial guesses that end after very different numbers of iterations - some in the first pair of launches, one five times
later than the median, some in wrong minima, one 30 m away where few points have a neighbour inside the gate."""
import numpy as np

from direct_lidar_odometry_amd import clouds

K, GATE, TRANS_EPS = 20, 0.5, 0.01
YAWS_DEG = (2, 5, 10, 20, 45, 90, 180)
GOOD_LANES = range(0, 7)   # lanes that end in the correct minimum (fitness 0.0569 on the oracle; the others 0.28 .. 239)
WELL_CONDITIONED = range(0, 6)  # at most 4 iterations, correct minimum


def workload():
    return clouds.scan_to_submap(20_000, 3)


def guesses(w) -> np.ndarray:
    """(12, 4, 4) float32."""
    gt = w.gt
    out = [w.guess, gt, np.eye(4)]
    out += [gt @ clouds.make_pose((0.3, -0.2, 0.05), (0, 0, yaw)) for yaw in YAWS_DEG]
    out += [gt @ clouds.make_pose((1.5, 1.0, 0)), gt @ clouds.make_pose((30, 0, 0))]
    return np.ascontiguousarray(np.stack([np.asarray(g, dtype=np.float32) for g in out]))


def configure(e, max_iter: int, gn: bool = False):
    """The settings of the case on a GPU handle or an oracle."""
    e.setCorrespondenceRandomness(K)
    e.setMaxCorrespondenceDistance(GATE)
    e.setTransformationEpsilon(TRANS_EPS)
    e.setMaximumIterations(max_iter)
    if gn:
        e.setOptimizer(0)


def oracle_fitness(orc, w, T, max_range=None):
    """pcl::Registration::getFitnessScore on the oracle's kd-tree: mean float32 squared 1-NN distance of the source transformed by the
    float matrix T, over the points with d2 <= max_range."""
    T = np.asarray(T, dtype=np.float32)
    moved = orc.transform_cloud(w.source, T)
    _, d2 = orc.OracleTree(w.target).knn(moved, 1, threads=16)
    d2 = d2[:, 0].astype(np.float64)
    if max_range is not None:
        d2 = d2[d2 <= max_range]
    return float(d2.mean()) if d2.size else float(np.finfo(np.float64).max)
