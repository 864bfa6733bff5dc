"""Shared inputs of the deskew tests (test_deskew_model_cpu.py, test_deskew_shim.py, test_gpu_deskew.py): seeded trajectories, time
sets that hit every knot and both ends, and raw point records with the time inside.  Every case is valid input."""
import numpy as np

import _deskew_model as dm


def random_trajectory(M, seed, max_rot=0.5, span=0.1, t0=0.0):
    """M poses (M, 4, 4) at ascending times: per segment a rotation of up to max_rot rad about a random axis and a step of up to 1 m."""
    rng = np.random.default_rng(seed)
    tau = t0 + (np.sort(np.r_[0.0, rng.uniform(0.05, 0.95, M - 2) * span, span]) if M > 2 else np.array([0.0, span]))
    assert (np.diff(tau) > 0).all()
    R = dm.so3_exp_matrix(rng.uniform(-1, 1, 3))
    t = rng.uniform(-5, 5, 3)
    poses = np.tile(np.eye(4), (M, 1, 1))
    for k in range(M):
        poses[k, :3, :3], poses[k, :3, 3] = R, t
        axis = rng.normal(size=3)
        R = R @ dm.so3_exp_matrix(axis / np.linalg.norm(axis) * rng.uniform(0.0, max_rot))
        t = t + rng.uniform(-1, 1, 3)
    return tau, poses


def times_for(tau, n, seed):
    """n times: every knot exactly, one below tau_0 and one above tau_{M-1} (as far as n allows), the rest uniform a little beyond both
    ends; shuffled, so that neighbouring points fall into unrelated segments."""
    rng = np.random.default_rng(seed)
    span = tau[-1] - tau[0]
    s = rng.uniform(tau[0] - 0.05 * span, tau[-1] + 0.05 * span, n)
    fixed = np.r_[tau[0] - 0.01 * span, tau[-1] + 0.01 * span, tau][:n]
    s[:len(fixed)] = fixed
    return s[rng.permutation(n)]


def twist_trajectory(v, w, duration, M):
    """M poses of the constant body twist (v m/s, w rad/s): T(t) = exp(t [w, v]) of SE(3), sampled at equal steps over [0, duration]."""
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    tau = np.linspace(0.0, duration, M)
    poses = np.tile(np.eye(4), (M, 1, 1))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    wn = np.linalg.norm(w)
    for k, t in enumerate(tau):
        th = wn * t
        if th < 1e-9:
            R, V = np.eye(3) + K * t, np.eye(3) + 0.5 * K * t
        else:
            R = np.eye(3) + np.sin(th) / wn * K + (1 - np.cos(th)) / wn**2 * (K @ K)
            V = np.eye(3) + (1 - np.cos(th)) / (wn**2 * t) * K + (th - np.sin(th)) / (wn**3 * t) * (K @ K)
        poses[k, :3, :3], poses[k, :3, 3] = R, V @ v * t
    return tau, poses


def records(xyz, stride, time_raw=None, time_off=None, intensity=None, intensity_off=None):
    """Raw point records as a C-contiguous float32 array (n, stride / 4): xyz at byte 0, the raw time (float32, float64 or uint32, by
    its dtype) at byte time_off, a float32 intensity at byte intensity_off, junk everywhere else."""
    n = len(xyz)
    buf = np.full((n, stride // 4), 777.0, np.float32)
    buf[:, :3] = xyz
    b = buf.view(np.uint8).reshape(n, stride)
    if intensity is not None:
        b[:, intensity_off:intensity_off + 4] = np.ascontiguousarray(intensity, np.float32).view(np.uint8).reshape(n, 4)
    if time_raw is not None:
        t = np.ascontiguousarray(time_raw)
        b[:, time_off:time_off + t.itemsize] = t.view(np.uint8).reshape(n, t.itemsize)
    return buf
