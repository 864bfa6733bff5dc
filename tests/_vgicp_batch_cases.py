"""The voxelized variant of the selection recipe ("More than one candidate pose"), shared by test_vgicp_batch_cpu.py (the
numpy model) and test_gpu_vgicp_batch.py (the engine): the 20k -> 60k pair and the twelve guesses of tests/_batch_cases.py, aligned
against the voxelized target with DIRECT27 at 1 m and scored with the fitness score; the lowest score must belong to a lane that ended
where the workload's own guess ends, within test_gpu_batch.py's bound for two poses being the same (1e-4 m, 1e-4 rad).

The convergence thresholds are NOT those of _batch_cases.configure (a translation step below 1 cm ends an alignment there).  A stopping
rule of 1 cm cannot place a pose within 0.1 mm: on the numpy model the seven lanes that reach the right minimum then end 1.7e-4 to
2.6e-4 m apart, beyond the bound, although they are in the same basin.  With steps below 1e-5 (m and rad) required, the same lanes end
within 3e-6 m and 4e-7 rad of each other on the model - well inside the bound - and the lanes in other minima stay metres away.  Not
collected by pytest (no test_ prefix)."""
RES, NEIGHBORS = 1.0, 27
MAX_ITER, TRANS_EPS, ROT_EPS = 32, 1e-5, 1e-5
MAX_RANGE = 1.0  # the squared gate of the fitness score (test_gpu_batch.py scores with it too)


def configure(e):
    """The settings of the case on a GPU handle."""
    e.setVoxelResolution(RES)
    e.setNeighborSearchMethod(NEIGHBORS)
    e.setMaximumIterations(MAX_ITER)
    e.setTransformationEpsilon(TRANS_EPS)
    e.setRotationEpsilon(ROT_EPS)
