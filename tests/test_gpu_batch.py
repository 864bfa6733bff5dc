"""GPU tests (-m gpu) of the batched alignment: ngicp_align_batch / alignBatch runs several initial guesses on one source / target
pair in the same launches (csrc/ngicp_batch.h), ngicp_fitness_score_batch scores the results in one launch.

The yardstick is the single path, which tests/_pass_check.py pins against the oracle pass by pass: lane g of a batch must be the same
BITS as align(guesses[g]) on a fresh handle - transformation, convergence flag, iteration count, Hessian and LM trace.  The guess set
(tests/_batch_cases.py) spreads the lanes from 0 to 22 iterations (tests/test_batch_cases_cpu.py shows that on the oracle alone)."""
import ctypes as C
import sys
import threading

import numpy as np
import pytest

import _batch_cases as bc
from _pass_check import FIXED20, Rig
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

# The criterion under which tests/test_gpu_parity.py compares align() with the oracle on its 10k workloads (_assert_pose_close with that
# file's TOL_T / TOL_R: translation error in metres, rotation angle in radians, clouds.pose_error).  Restated, not invented here.
TOL_T, TOL_R = 1e-4, 1e-4


def _assert_pose_close(Tg, To, tt=TOL_T, tr=TOL_R):
    dt, dr = clouds.pose_error(Tg, To)
    assert dt <= tt and dr <= tr, (dt, dr)


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def case():
    w = bc.workload()
    return w, bc.guesses(w)


def _handle(ng, src, tgt, configure):
    g = ng.NanoGICP()
    configure(g)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    return g


def _single(g, guesses):
    """align() per guess on handle g -> per guess (T, converged, iterations, H, trace)."""
    out = []
    for q in guesses:
        g.align(q)
        out.append((g.getFinalTransformation().copy(), bool(g.hasConverged()), int(g.nr_iterations_), g.getFinalHessian().copy(), g.lm_trace().copy()))
    return out


def _assert_lanes_equal(g, res, refs, label=""):
    """The batch result `res` of handle g (whose last call was that batch), lane by lane, against the single aligns `refs`."""
    T, conv, its, H = res
    assert T.shape == (len(refs), 4, 4) and T.dtype == np.float32 and H.shape == (len(refs), 6, 6)
    for lane, (rT, rconv, rits, rH, rtrace) in enumerate(refs):
        where = f"{label} lane {lane}"
        assert np.array_equal(T[lane], rT), where
        assert bool(conv[lane]) == rconv and int(its[lane]) == rits, (where, conv[lane], its[lane], rconv, rits)
        assert np.array_equal(H[lane], rH), where
        assert np.array_equal(g.lm_trace(lane=lane), rtrace), where


_refs = {}


def _case_refs(ng, case, max_iter, gn=False):
    """The single aligns of the whole guess set on a fresh handle (computed once per setting)."""
    key = (max_iter, gn)
    if key not in _refs:
        w, G = case
        g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, max_iter, gn))
        _refs[key] = _single(g, G)
        g.close()
    return _refs[key]


# ------------------------------------------------------------------ 1. lane = single align, bit for bit
@pytest.mark.parametrize("B,max_iter,gn", [(1, 8, False), (2, 8, False), (3, 8, False), (12, 8, False), (1, 32, False), (2, 32, False),
                                            (3, 32, False), (12, 32, False), (12, 32, True)])
def test_lane_is_the_single_align_bit_for_bit(ng, case, B, max_iter, gn):
    w, G = case
    refs = _case_refs(ng, case, max_iter, gn)
    print("single aligns: iterations", [r[2] for r in refs[:B]], "converged", [r[1] for r in refs[:B]])
    g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, max_iter, gn))
    _assert_lanes_equal(g, g.alignBatch(G[:B]), refs[:B], f"B={B} max_iter={max_iter} gn={gn}")
    g.close()


def test_no_iterations_returns_the_guesses(ng, case):
    """max_iter <= 0: every lane returns its guess, as ngicp_align does."""
    w, G = case
    refs = _case_refs(ng, case, 0)
    g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 0))
    res = g.alignBatch(G)
    _assert_lanes_equal(g, res, refs, "max_iter=0")
    assert not res[1].any() and not res[2].any()
    g.close()


# ------------------------------------------------------------------ 2. lane independence
def test_lanes_do_not_see_each_other(ng, case):
    w, G = case
    refs = _case_refs(ng, case, 32)
    g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 32))
    perm = np.random.default_rng(7).permutation(len(G))
    assert not np.array_equal(perm, np.arange(len(G)))
    _assert_lanes_equal(g, g.alignBatch(G[perm]), [refs[i] for i in perm], "permuted")
    # the same guess in lanes 0, 5 and 11
    G2 = G.copy()
    G2[0] = G2[5] = G2[11] = G[6]
    refs2 = list(refs)
    refs2[0] = refs2[5] = refs2[11] = refs[6]
    res = g.alignBatch(G2)
    _assert_lanes_equal(g, res, refs2, "repeated guess")
    for a in (5, 11):
        assert np.array_equal(res[0][0], res[0][a]) and np.array_equal(res[3][0], res[3][a]) and res[2][0] == res[2][a]
    # twice on one handle
    again = g.alignBatch(G2)
    for a, b in zip(res, again):
        assert np.array_equal(a, b)
    g.close()


# ------------------------------------------------------------------ 3. the handle's single-alignment state is untouched
def test_batch_leaves_the_results_of_the_last_align_alone(ng, case):
    w, G = case
    g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 32))

    def snapshot():
        corr = g.correspondences()
        return (g.getFinalTransformation().copy(), g.getFinalHessian().copy(), bool(g.hasConverged()), int(g.nr_iterations_),
                [np.array(c).copy() for c in (corr if isinstance(corr, tuple) else (corr,))], g.lm_trace().copy(), g.stats()["passes"])

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
        assert len(a[4]) == len(b[4]) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))
        assert np.array_equal(a[5], b[5]) and a[6] == b[6]

    g.align(w.guess)
    before = snapshot()
    g.alignBatch(G)
    same(before, snapshot())
    # ... also when the trace of the align was not fetched before the batch
    g.align(w.guess)
    g.alignBatch(G)
    same(before, snapshot())
    g.align(w.guess)
    same(before, snapshot())
    # ... and when the batch runs with larger budgets than the align did: the handle's own state, trace and correspondence buffers,
    # whose sizes follow the iteration budgets and the source, are not the batch's to resize
    for setter, v in ((g.setMaximumIterations, 300), (g.setLMMaxIterations, 40)):
        setter(v)
        g.alignBatch(G[:3])
        same(before, snapshot())
    g.close()


def test_batch_with_larger_budgets_before_the_trace_was_fetched(ng, case):
    """align, then a batch with raised budgets BEFORE trace and correspondences were fetched: they stay those of the align."""
    w, G = case
    g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 8))
    g.align(G[6])
    f = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 8))
    f.align(G[6])
    want = (f.getFinalTransformation().copy(), f.getFinalHessian().copy(), f.correspondences(), f.lm_trace().copy(), f.stats()["passes"])
    f.close()
    g.setMaximumIterations(500)
    g.setLMMaxIterations(50)
    g.alignBatch(G[:4])
    got = (g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.correspondences(), g.lm_trace().copy(), g.stats()["passes"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1])
    assert np.array_equal(got[3], want[3]) and got[4] == want[4]
    g.close()


# ------------------------------------------------------------------ 4. against the oracle directly
def test_well_conditioned_lanes_against_the_oracle(ng, oracle_mod, case):
    """Lanes 0..5 (at most 4 iterations, correct minimum): the oracle's align(guess) takes the same decisions and ends at the same pose
    under test_gpu_parity.py's criterion.  For lanes 6..11 - up to 22 iterations into poor or wrong minima - whether engine and oracle
    take the same LM decisions is a property of the single path that nobody has measured; there bit-equality with align() is the
    yardstick (test_lane_is_the_single_align_bit_for_bit)."""
    w, G = case
    rig = Rig(ng, oracle_mod, w.source, w.target, bc.K, bc.GATE, dict(setMaximumIterations=32, setTransformationEpsilon=bc.TRANS_EPS))
    rig.g.setMaximumIterations(32)
    rig.o.setMaximumIterations(32)
    T, conv, its, _ = rig.g.alignBatch(G)
    for lane in bc.WELL_CONDITIONED:
        rig.o.align(G[lane])
        print("lane", lane, "gpu", bool(conv[lane]), int(its[lane]), "oracle", rig.o.converged, rig.o.nr_iterations, "pose error",
              clouds.pose_error(T[lane], rig.o.final_transformation))
        assert bool(conv[lane]) == bool(rig.o.converged) and int(its[lane]) == int(rig.o.nr_iterations), lane
        _assert_pose_close(T[lane], rig.o.final_transformation)
    rig.g.close()


# ------------------------------------------------------------------ 5. buffers grow and are reused
def test_buffers_follow_the_source_size_and_the_lane_count(ng, case):
    """One handle through 12 lanes on the 20k source, 5 lanes on a 10k and on a 40k source, 12 lanes on the 20k source again.  The
    reference is a second, fresh handle taken through the same sequence of setInputSource calls: a handle sizes the voxels of a new
    index from the last cloud of similar size it indexed (the auto-voxel memo, ngicp_api.hip), so the 40k source, which falls into the
    size class of the 60k target, is cut into other query batches - another summation order, other last bits of H - than on a handle
    that has not seen that target yet.  That is the single path's history, not the batch's."""
    w, G = case
    conf = lambda e: bc.configure(e, 32)  # noqa: E731
    g = _handle(ng, w.source, w.target, conf)
    f = _handle(ng, w.source, w.target, conf)
    _assert_lanes_equal(g, g.alignBatch(G), _case_refs(ng, case, 32), "20k, 12 lanes")
    for n in (10_000, 40_000):
        src = clouds.scan_to_submap(n, 3).source
        f.setInputSource(src)
        g.setInputSource(src)
        _assert_lanes_equal(g, g.alignBatch(G[:5]), _single(f, G[:5]), f"{n}, 5 lanes")
    f.setInputSource(w.source)
    g.setInputSource(w.source)
    _assert_lanes_equal(g, g.alignBatch(G), _single(f, G), "20k again, 12 lanes")
    f.close()
    g.close()


# ------------------------------------------------------------------ 6. full size: the grid that selects the 4-waves build
def test_full_size_four_lanes(ng):
    w = clouds.scan_to_submap()
    assert w.source.shape[0] == 100_000 and w.target.shape[0] == 500_000

    def conf(e):
        e.setCorrespondenceRandomness(20)
        e.setMaxCorrespondenceDistance(w.max_corr_dist)
        for name, v in FIXED20.items():
            getattr(e, name)(v)

    G = np.stack([w.guess] + [(w.guess.astype(np.float64) @ clouds.make_pose(t, r)).astype(np.float32)
                              for t, r in (((0.02, 0.0, 0.0), (0, 0, 0.2)), ((0.0, -0.03, 0.01), (0.1, 0, -0.3)), ((-0.04, 0.02, 0.0), (0, 0.2, 0.4)))])
    f = _handle(ng, w.source, w.target, conf)
    refs = _single(f, G)
    f.close()
    g = _handle(ng, w.source, w.target, conf)
    _assert_lanes_equal(g, g.alignBatch(G), refs, "c3 fixed20")
    g.close()


# ------------------------------------------------------------------ 7. fitness
def test_batched_fitness_and_the_pick(ng, case):
    w, G = case
    g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 32))
    T = g.alignBatch(G)[0]
    for max_range in (sys.float_info.max, 1.0):
        scores, cnt = g.fitnessBatch(T, max_range)
        single = [g.fitness(max_range, t) for t in T]
        print("fitness, max_range", max_range, ["%.4g" % s for s in scores], cnt.tolist())
        assert scores.dtype == np.float64 and scores.shape == (12,)
        assert np.array_equal(scores, np.array([s[0] for s in single])) and cnt.tolist() == [s[1] for s in single]
        assert int(np.argmin(scores)) in bc.GOOD_LANES
    one, n_one = g.fitnessBatch(T[3:4], 1.0)
    assert (float(one[0]), int(n_one[0])) == g.fitness(1.0, T[3])
    g.close()


# ------------------------------------------------------------------ 8. errors
def test_errors_leave_the_handle_usable(ng, case):
    w, G = case
    L = ng.load_library()
    f32p, i32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)
    g = ng.NanoGICP()
    bc.configure(g, 32)
    gc = np.ascontiguousarray(np.transpose(G, (0, 2, 1))).reshape(-1, 16)
    T = np.empty((12, 16), np.float32); conv = np.zeros(12, np.int32); its = np.zeros(12, np.int32); H = np.empty((12, 36))
    sc = np.empty(12); cnt = np.zeros(12, np.uint64)

    def call(n=12, guesses=gc, T_=T, conv_=conv, its_=its, H_=H):
        p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)  # noqa: E731
        return L.ngicp_align_batch(g._h, n, p(guesses, f32p), p(T_, f32p), p(conv_, i32p), p(its_, i32p), p(H_, f64p))

    def failed(rc, code):
        assert rc == code, (rc, code)
        assert L.ngicp_last_error(g._h)

    failed(call(), -3)  # neither cloud
    with pytest.raises(ng.NgicpError) as e:
        g.alignBatch(G)
    assert e.value.code == -3
    g.setInputSource(w.source)
    failed(call(), -3)  # no target
    failed(L.ngicp_fitness_score_batch(g._h, 12, T.ctypes.data_as(f32p), 1.0, sc.ctypes.data_as(f64p), cnt.ctypes.data_as(C.POINTER(C.c_size_t))), -3)
    g.clearSource()
    g.setInputTarget(w.target)
    failed(call(), -3)  # no source
    g.setInputSource(w.source)
    failed(call(n=0), -2)
    failed(call(n=ng.BATCH_MAX_LANES + 1), -2)
    failed(call(guesses=None), -2)
    failed(call(T_=None), -2)
    failed(call(conv_=None), -2)
    failed(call(its_=None), -2)
    failed(L.ngicp_fitness_score_batch(g._h, 0, T.ctypes.data_as(f32p), 1.0, sc.ctypes.data_as(f64p), None), -2)
    failed(L.ngicp_fitness_score_batch(g._h, 12, None, 1.0, sc.ctypes.data_as(f64p), None), -2)
    failed(L.ngicp_fitness_score_batch(g._h, 12, T.ctypes.data_as(f32p), 1.0, None, None), -2)
    n_rows = C.c_size_t(0)
    failed(L.ngicp_batch_get_lm_trace(g._h, 0, None, 0, C.byref(n_rows)), -2)  # no batch has run
    assert call(H_=None) == 0  # the Hessians are optional
    failed(L.ngicp_batch_get_lm_trace(g._h, 12, None, 0, C.byref(n_rows)), -2)  # lanes 0..11
    # the handle still aligns, singly and in a batch
    refs = _case_refs(ng, case, 32)
    assert [int(v) for v in its] == [r[2] for r in refs]
    g.align(G[5])
    assert np.array_equal(g.getFinalTransformation(), refs[5][0])
    _assert_lanes_equal(g, g.alignBatch(G), refs, "after the errors")
    g.close()


# ------------------------------------------------------------------ two handles on two threads
def test_batches_from_two_threads_give_the_serial_results(ng, case):
    w, G = case
    sets = [G, G[::-1].copy()]
    refs = _case_refs(ng, case, 32)
    want = [refs, refs[::-1]]
    results, errors = [None, None], []

    def work(t):
        try:
            g = _handle(ng, w.source, w.target, lambda e: bc.configure(e, 32))
            out = []
            for _ in range(3):
                res = g.alignBatch(sets[t])
                out.append((res, [g.lm_trace(lane=i) for i in range(len(sets[t]))]))
            g.close()
            results[t] = out
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errors, errors
    assert all(not th.is_alive() for th in threads)
    for t in range(2):
        for (T, conv, its, H), traces in results[t]:
            for lane, (rT, rconv, rits, rH, rtrace) in enumerate(want[t]):
                assert np.array_equal(T[lane], rT) and bool(conv[lane]) == rconv and int(its[lane]) == rits and np.array_equal(H[lane], rH)
                assert np.array_equal(traces[lane], rtrace)
