"""The rule behind K4-only passes (ngicp_lm.h set_lin_unneeded), pinned on oracle/numpy_model.py's LM loop (no GPU).

A trial is flagged when its step already meets the convergence test, or when it belongs to the last outer iteration
(it + 1 >= max_iterations).  The claim: the linearisation at a flagged trial's pose is never used - in the model's sequence of events every
flagged trial is followed by the end of the alignment or by another trial from the unchanged linearisation, never by linearize()."""
import numpy as np
import pytest

from oracle.numpy_model import NumpyGICP


class Recording(NumpyGICP):
    """The model with its events written down: ("lin", pose) for linearize(), ("trial", pose, flagged) for the error of a trial."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.events = []

    def linearize(self, T):
        self.events.append(("lin", np.array(T)))
        return super().linearize(T)

    def accumulate(self, T, want=True):
        if not want:  # compute_error(xi): the trial the loop has just made from the last linearisation's pose
            x0 = [e for e in self.events if e[0] == "lin"][-1][1]
            it = sum(1 for e in self.events if e[0] == "lin") - 1
            inv = np.eye(4)
            inv[:3, :3] = x0[:3, :3].T
            inv[:3, 3] = -x0[:3, :3].T @ x0[:3, 3]
            delta = T @ inv  # xi = delta * x0
            self.events.append(("trial", np.array(T), bool(self.is_converged(delta) or it + 1 >= self.max_iter)))
        return super().accumulate(T, want)


def _clouds(n=48, seed=5):
    rng = np.random.default_rng(seed)
    tgt = np.c_[rng.uniform(-2, 2, (n, 2)), 0.3 * np.sin(rng.uniform(-2, 2, n))].astype(np.float32)
    tgt[n // 2:, 2] += rng.uniform(0.5, 1.5, n - n // 2).astype(np.float32)
    a = 0.03
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    src = ((tgt.astype(np.float64) - [0.05, -0.04, 0.02]) @ R + 0.02 * rng.standard_normal((n, 3))).astype(np.float32)  # (noise: a floor the error stops at)
    c = np.diag([0.01, 0.01, 0.01, 0.0])
    return src, tgt, np.repeat(c[None], n, 0), np.repeat(c[None], n, 0)


CASES = {
    "iteration limit 1": dict(max_iter=1, trans_eps=1e-12, rot_eps=1e-12),
    "iteration limit 3": dict(max_iter=3, trans_eps=1e-12, rot_eps=1e-12),
    "convergence by epsilon": dict(max_iter=32, trans_eps=0.01, rot_eps=2e-3),
    "noise floor": dict(max_iter=12, trans_eps=1e-12, rot_eps=1e-12),          # rejected trials once the error stops falling
    "lm_max_iterations 1": dict(max_iter=12, trans_eps=1e-12, rot_eps=1e-12, lm_max_iter=1),
    "lm_max_iterations 2": dict(max_iter=12, trans_eps=1e-12, rot_eps=1e-12, lm_max_iter=2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_flagged_trial_is_never_followed_by_a_linearisation(case):
    src, tgt, cs, ct = _clouds()
    m = Recording(src, tgt, cs, ct, max_corr_dist=1.0, **CASES[case])
    m.align(np.eye(4, dtype=np.float32))
    ev = m.events
    trials = [i for i, e in enumerate(ev) if e[0] == "trial"]
    flagged = [i for i in trials if ev[i][2]]
    print(f"{case}: {sum(1 for e in ev if e[0] == 'lin')} linearisations, {len(trials)} trials, {len(flagged)} flagged, "
          f"{sum(1 for r in m.trace if r[7] == 0)} rejected, converged {m.converged}")
    lm_failed = len(m.trace) > 0 and m.trace[-1][7] == 0 and not m.converged  # "lm not converged": may come before any trial is flagged
    assert len(trials) == len(m.trace) and (flagged or lm_failed), "the case makes no flagged trial"
    for i in flagged:
        assert i + 1 == len(ev) or ev[i + 1][0] == "trial", f"{case}: event {i} is a flagged trial and is followed by a linearisation"
    # the other direction, where the alignment ends by convergence or at the iteration limit: its last trial was flagged
    if not lm_failed:
        assert ev[-1][0] == "trial" and ev[-1][2]
    # and an unflagged trial that is accepted IS followed by the linearisation at its pose (what a full pass speculates on)
    for i, row in zip(trials, m.trace):
        if not ev[i][2] and row[7] == 1:
            assert ev[i + 1][0] == "lin" and np.array_equal(ev[i + 1][1], ev[i][1])


def test_the_cases_cover_both_reasons_and_a_rejection():
    src, tgt, cs, ct = _clouds()
    m = Recording(src, tgt, cs, ct, max_corr_dist=1.0, **CASES["convergence by epsilon"])
    m.align(np.eye(4, dtype=np.float32))
    assert m.converged and m.nr_iterations + 1 < 32  # flagged by the step, not by the limit
    m = Recording(src, tgt, cs, ct, max_corr_dist=1.0, **CASES["iteration limit 3"])
    m.align(np.eye(4, dtype=np.float32))
    assert not m.converged and m.nr_iterations == 2  # flagged by the limit
