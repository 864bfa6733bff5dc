"""-m gpu: the covariance kernel (csrc/ngicp_knn.h k_covariances) where it can go wrong without the rest of the suite noticing.

(a) exactly degenerate neighbourhoods: planes with exact zeros in C, lines (rank 1), coincident points (rank 0), k = 1 and k = 2,
    coordinates kilometres from the origin - every family of tests/_cov_model.py, every k, all five regularisations, against the
    CPU oracle at 1e-9 where the result is well defined and by the PLANE properties where it is not (the rules, and the proof
    that the oracle itself meets them, are in _cov_model.py and test_cov_model_cpu.py);
(b) tiny clouds: n == k, n == k + 1 and n == 1 for each compiled list size (K = 10, 20, 32);
(c) the target slot, once per kind of input;
(d) the block path ngicp_covs_shard_begin / _compute / _commit with `first > 0` and `n < cloud size`, which the only other GPU
    test of it (tests/_sharded_rccl_worker.py, world size 1) never reaches: blocks whose bounds avoid the multiples of the 64
    queries of a thread block, out of order, an empty one, one twice; two and three emulated ranks on one GPU, one handle per
    rank, the blocks exchanged with torch copies in place of the collective; the error codes.

No full-size case is added: every cloud here has fewer than 160 000 points and runs k_covariances<K, 6>; the narrow-window variant
k_covariances<K, 4> of larger clouds stays covered by test_gpu_fullsize.py."""
import numpy as np
import pytest

import _cov_model as cm
from direct_lidar_odometry_amd import clouds, sharding

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_K = -2, -3, -4  # include/ngicp.h: NGICP_ERR_ARG, NGICP_ERR_STATE, NGICP_ERR_K_TOO_LARGE
SENTINEL = -7.0
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _engine(ng, pts, k, reg=3, which=0):
    g = ng.NanoGICP()
    g.setCorrespondenceRandomness(k)
    g.setRegularizationMethod(reg)
    (g.setInputTarget if which else g.setInputSource)(pts)
    return g


def _covariances(ng, pts, k, reg=3, which=0):
    g = _engine(ng, pts, k, reg, which)
    if which:
        g.calculateTargetCovariances()
        out = g.getTargetCovariances()
    else:
        g.calculateSourceCovariances()
        out = g.getSourceCovariances()
    g.close()
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------ (a) degenerate neighbourhoods, (b) tiny clouds
@pytest.mark.parametrize("reg", list(cm.REGS))
@pytest.mark.parametrize("name,k", cm.cases())
def test_covariances_on_degenerate_and_tiny_clouds(ng, oracle_mod, name, k, reg):
    r = cm.REGS[reg]
    out = _covariances(ng, cm.families()[name], k, r)
    fig = cm.check_case(out, cm.oracle_covariances(name, k, r), name, k, r)
    print(f"{name} k={k} {reg}: {fig}")


@pytest.mark.parametrize("reg", list(cm.REGS))
@pytest.mark.parametrize("n", [1, 2, 10, 20, 32])
def test_whole_cloud_neighbourhood_gives_one_covariance(ng, oracle_mod, n, reg):
    """n == k: every point's neighbour set is the whole cloud, so all n covariances are the same matrix; only the order in which
    each point's list adds the neighbours differs."""
    r = cm.REGS[reg]
    name = f"tiny_n{n}"
    pts = cm.families()[name]
    out = _covariances(ng, pts, n, r)
    nbr, ambiguous, _, absw = cm.reference(name, n)
    assert not ambiguous.any() and np.all(np.sort(nbr, axis=1) == np.arange(n))
    model, _ = cm.model_covariances(pts, nbr, r)
    if r == cm.REGS["PLANE"] and not cm.plane_separated(absw).all():  # n <= 2: rank <= 1, judged by the PLANE properties in the test above
        return
    assert np.abs(out - out[0]).max() <= 1e-12
    assert np.abs(out - model).max() < cm.TOL


@pytest.mark.parametrize("n", [1, 2, 10, 20, 32])
def test_k_above_the_cloud_size_is_refused(ng, n):
    g = _engine(ng, cm.families()[f"tiny_n{n}"], n + 1)
    with pytest.raises(ng.NgicpError) as e:
        g.calculateSourceCovariances()
    assert e.value.code == ERR_K
    assert g.sourceCovariancesSize() == 0
    g.setCorrespondenceRandomness(n)
    g.calculateSourceCovariances()  # still usable
    assert g.sourceCovariancesSize() == n


# ------------------------------------------------------------------ (c) the target slot
@pytest.mark.parametrize("name", ["plane_z", "dups4", "far"])
def test_target_slot_computes_the_same(ng, oracle_mod, name):
    for k, reg in ((10, "PLANE"), (20, "NONE"), (3, "NORMALIZED_MIN_EIG")):
        r = cm.REGS[reg]
        out = _covariances(ng, cm.families()[name], k, r, which=1)
        cm.check_case(out, cm.oracle_covariances(name, k, r), name, k, r)
        assert np.array_equal(_bits(out), _bits(_covariances(ng, cm.families()[name], k, r, which=0)))


# ------------------------------------------------------------------ (d) the block path on one GPU
def _get(g, which):
    return g.getTargetCovariances() if which else g.getSourceCovariances()


def _partition(n):
    """Blocks of [0, n) whose bounds avoid the multiples of 64 (kKnnPairs), in the order they are issued: not ascending, the empty
    block among them.  Every block but the last ends before n."""
    blocks = [(65, 513), (0, 1), (63, 64), (65, 65), (1, 63), (64, 65), (513, n)]
    covered = sorted(b for b in blocks if b[0] < b[1])
    assert covered[0][0] == 0 and covered[-1][1] == n and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    return blocks


class _ShardRun:
    """A handle between covsShardBegin and covsShardCommit, its buffer aliased by a torch tensor, driven on a torch side stream."""

    def __init__(self, ng, pts, k, which):
        import torch
        self.torch = torch
        self.g = _engine(ng, pts, k, which=which)
        self.which = which
        ptr, self.n = self.g.covsShardBegin(which)
        assert self.n == len(pts)
        self.view = sharding.device_doubles(ptr, self.n * 6, DEV)
        assert self.view.numel() == self.n * 6 and self.view.dtype == torch.float64
        self.side = torch.cuda.Stream(torch.device(DEV))
        self.side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
        assert self.side.cuda_stream != 0
        with torch.cuda.stream(self.side):
            self.view.fill_(SENTINEL)
        self.side.synchronize()

    def rows(self):
        """The buffer as it is now: (n, 6) on the host."""
        with self.torch.cuda.stream(self.side):
            host = self.view.cpu()
        self.side.synchronize()
        return host.numpy().reshape(self.n, 6).copy()

    def compute(self, lo, hi):
        self.g.covsShardCompute(self.which, lo, hi, self.side.cuda_stream)
        self.side.synchronize()

    def commit(self):
        self.side.synchronize()
        self.g.covsShardCommit(self.which)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("k", [10, 20, 32])
@pytest.mark.parametrize("name", ["lidar", "dups4"])
def test_blocks_write_their_rows_and_nothing_else(ng, name, k, which):
    pts = cm.families()[name]
    run = _ShardRun(ng, pts, k, which)
    n = run.n
    assert np.all(run.rows() == SENTINEL)
    for lo, hi in _partition(n):
        before = run.rows()
        run.compute(lo, hi)
        after = run.rows()
        changed = np.any(_bits(after) != _bits(before), axis=1)
        off_sentinel = np.any(after != SENTINEL, axis=1)
        assert changed[lo:hi].all() and off_sentinel[lo:hi].all(), (lo, hi, np.flatnonzero(~changed[lo:hi])[:5] + lo)
        assert not changed[:lo].any() and not changed[hi:].any(), (lo, hi, np.flatnonzero(changed)[:5], np.flatnonzero(changed)[-5:])
    whole = run.rows()
    assert np.all(np.isfinite(whole)) and np.all(np.any(whole != SENTINEL, axis=1))
    # one block again, over rows put back to the sentinel: the same rows, the same bits
    with run.torch.cuda.stream(run.side):
        run.view[1 * 6:63 * 6].fill_(SENTINEL)
    run.side.synchronize()
    run.compute(1, 63)
    assert np.array_equal(_bits(run.rows()), _bits(whole))
    run.commit()
    assert np.array_equal(_bits(_get(run.g, which)), _bits(_covariances(ng, pts, k, which=which)))
    run.g.close()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("k", [10, 20, 32])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["lidar", "dups4"])
def test_emulated_ranks_assemble_the_single_handle_result(ng, name, world, k, which):
    """One handle per rank, as real ranks would have; each computes shard_bounds(n, world, rank) into its own buffer; torch copies
    between the aliased buffers stand in for the all-gather / broadcasts of sharding.sharded_covariances; every handle commits.
    Bit-equality with one handle's calculate*Covariances() on EVERY rank also pins what sharding.py relies on: the index build is
    deterministic, so the packed sorted layout is the same on every rank."""
    import torch
    pts = cm.families()[name]
    single = _covariances(ng, pts, k, which=which)
    ranks = [_ShardRun(ng, pts, k, which) for _ in range(world)]
    n = ranks[0].n
    bounds = [sharding.shard_bounds(n, world, r) for r in range(world)]
    assert bounds[0][0] == 0 and bounds[-1][1] == n and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    if world == 3 and name == "lidar":
        assert len({hi - lo for lo, hi in bounds}) == 2  # 2000 points do not divide by 3: the blocks differ in size
    for r, (lo, hi) in enumerate(bounds):
        ranks[r].compute(lo, hi)
        rows = ranks[r].rows()
        mine = np.any(rows != SENTINEL, axis=1)
        assert mine[lo:hi].all() and not mine[:lo].any() and not mine[hi:].any(), (r, lo, hi)
    for src, (lo, hi) in enumerate(bounds):  # the exchange
        for dst in range(world):
            if dst != src:
                with torch.cuda.stream(ranks[dst].side):
                    ranks[dst].view[lo * 6:hi * 6].copy_(ranks[src].view[lo * 6:hi * 6])
    for run in ranks:
        run.commit()
    for r, run in enumerate(ranks):
        assert np.array_equal(_bits(_get(run.g, which)), _bits(single)), r
        run.g.close()


@pytest.mark.parametrize("which", [0, 1])
def test_block_path_errors_by_code_and_the_handle_survives(ng, which):
    w = clouds.scan_to_scan(2000)
    pts = cm.families()["lidar"]
    other = cm.families()["dups4"]
    set_cloud = "setInputTarget" if which else "setInputSource"

    def code(call, *a):
        with pytest.raises(ng.NgicpError) as e:
            call(*a)
        return e.value.code

    g = _engine(ng, pts, 10, which=which)
    assert code(g.covsShardCompute, which, 0, 10) == ERR_STATE  # compute before begin
    assert code(g.covsShardCommit, which) == ERR_STATE          # commit before begin
    assert code(g.covsShardBegin, 2) == ERR_ARG
    _, n = g.covsShardBegin(which)
    assert n == len(pts)
    assert code(g.covsShardCompute, which, 11, 10) == ERR_ARG     # lo > hi
    assert code(g.covsShardCompute, which, 0, n + 1) == ERR_ARG   # hi > n
    assert code(g.covsShardCompute, which, n + 1, n + 2) == ERR_ARG
    assert code(g.covsShardCompute, 1 - which, 0, 10) == ERR_STATE  # the other slot was never begun
    g.covsShardCompute(which, 0, n)
    g.covsShardCommit(which)
    assert np.array_equal(_bits(_get(g, which)), _bits(_covariances(ng, pts, 10, which=which)))
    assert code(g.covsShardCommit, which) == ERR_STATE          # a second commit
    assert code(g.covsShardCompute, which, 0, 10) == ERR_STATE  # and the committed set is no longer open for blocks
    # begin, then another cloud in the slot: the open set belongs to a cloud that is gone
    g.covsShardBegin(which)
    getattr(g, set_cloud)(other)
    assert code(g.covsShardCompute, which, 0, 10) == ERR_STATE
    assert code(g.covsShardCommit, which) == ERR_STATE
    # k above the cloud size is found at compute (begin does not look at k)
    small = cm.families()["tiny_n10"]
    getattr(g, set_cloud)(small)
    g.setCorrespondenceRandomness(11)
    _, n = g.covsShardBegin(which)
    assert n == 10
    assert code(g.covsShardCompute, which, 0, 10) == ERR_K
    assert code(g.covsShardCompute, which, 3, 3) == ERR_K
    # after all of it the handle still aligns, and to the bits of a handle that saw no error
    fresh = ng.NanoGICP()
    for e in (g, fresh):
        e.setCorrespondenceRandomness(20)
        e.setMaxCorrespondenceDistance(1.0)
        e.setInputSource(w.source)
        e.setInputTarget(w.target)
        e.align()
    assert np.array_equal(g.getFinalTransformation(), fresh.getFinalTransformation())
    assert g.nr_iterations_ == fresh.nr_iterations_ and g.converged_ == fresh.converged_
    assert not np.array_equal(g.getFinalTransformation(), np.eye(4, dtype=np.float32))  # it moved
    g.close()
    fresh.close()
