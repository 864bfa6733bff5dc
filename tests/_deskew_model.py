"""The motion deskew of include/ngicp.h ("motion deskew"; csrc/ngicp_deskew.h) restated in numpy float64, operation by operation in the
engine's order (sums left to right, no FMA), so3_log and so3_exp_matrix of csrc/ngicp_math.h included.  What differs from the device
is the libm behind sin, cos, sqrt and atan2, and nothing else.

test_deskew_model_cpu.py proves this file against an independent statement (scipy's Slerp); test_gpu_deskew.py proves the engine
against this file."""
import numpy as np

TIME_F32_S, TIME_F64_S, TIME_U32_NS = 0, 1, 2
UNIT = {TIME_F32_S: 1.0, TIME_F64_S: 1.0, TIME_U32_NS: 1e-9}
DTYPE = {TIME_F32_S: np.float32, TIME_F64_S: np.float64, TIME_U32_NS: np.uint32}


def seconds(raw, time_format, time_offset=0.0) -> np.ndarray:
    """s = double(raw) * unit + time_offset: two roundings, in that order."""
    return np.asarray(raw, DTYPE[time_format]).astype(np.float64) * UNIT[time_format] + np.float64(time_offset)


def _dot3(a0, a1, a2, b0, b1, b2):
    return a0 * b0 + a1 * b1 + a2 * b2  # pose_mul_r: ((a0 b0 + a1 b1) + a2 b2)


def _matmul_tn(A, B):
    """A^T B of (..., 3, 3) arrays, element (i, j) = sum_l A[l, i] B[l, j] in pose_mul_r's order."""
    out = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = _dot3(A[..., 0, i], A[..., 1, i], A[..., 2, i], B[..., 0, j], B[..., 1, j], B[..., 2, j])
    return out


def _matmul_nn(A, B):
    out = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = _dot3(A[..., i, 0], A[..., i, 1], A[..., i, 2], B[..., 0, j], B[..., 1, j], B[..., 2, j])
    return out


def so3_log(R) -> np.ndarray:
    """(..., 3, 3) -> (..., 3): ngk::so3_log."""
    R = np.asarray(R, np.float64)
    vx, vy, vz = 0.5 * (R[..., 2, 1] - R[..., 1, 2]), 0.5 * (R[..., 0, 2] - R[..., 2, 0]), 0.5 * (R[..., 1, 0] - R[..., 0, 1])
    c = 0.5 * ((R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]) - 1.0)
    s2 = vx * vx + vy * vy + vz * vz
    series = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0 + s2 * (15.0 / 336.0)))
    s = np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        closed = np.where(s > 0.0, np.arctan2(s, c) / s, 0.0)
    f = np.where((s2 < 1e-6) & (c > 0.0), series, closed)
    return np.stack([f * vx, f * vy, f * vz], axis=-1)


def so3_exp_matrix(w) -> np.ndarray:
    """(..., 3) -> (..., 3, 3): ngk::so3_exp_matrix (the quaternion of gicp/so3.hpp, then Eigen's toRotationMatrix)."""
    w = np.asarray(w, np.float64)
    theta_sq = w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2]
    quad = theta_sq * theta_sq
    small = theta_sq < 1e-10
    theta = np.sqrt(np.where(small, 1.0, theta_sq))
    half = 0.5 * theta
    imag = np.where(small, 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * quad, np.sin(half) / theta)
    real = np.where(small, 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * quad, np.cos(half))
    qw, qx, qy, qz = real, imag * w[..., 0], imag * w[..., 1], imag * w[..., 2]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    R = np.empty(w.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R


def table(pose_times, poses, T_ref=None):
    """Steps 1 and 2: (tau (M), R' (M, 3, 3), t' (M, 3), phi (M, 3); phi of the last pose is zero)."""
    tau = np.asarray(pose_times, np.float64)
    P = np.asarray(poses, np.float64)
    Tr = np.eye(4) if T_ref is None else np.asarray(T_ref, np.float64)
    Rr = Tr[:3, :3]
    Rp = _matmul_tn(Rr[None], P[:, :3, :3])
    d = P[:, :3, 3] - Tr[:3, 3]
    tp = np.stack([_dot3(Rr[0, i], Rr[1, i], Rr[2, i], d[:, 0], d[:, 1], d[:, 2]) for i in range(3)], axis=-1)
    phi = np.zeros((len(tau), 3))
    phi[:-1] = so3_log(_matmul_tn(Rp[:-1], Rp[1:]))
    return tau, Rp, tp, phi


def pose_at(s, tab):
    """Steps 3 and 4 for finite times s (N): (R(s) (N, 3, 3), t(s) (N, 3))."""
    tau, Rp, tp, phi = tab
    s = np.asarray(s, np.float64)
    k = np.clip(np.searchsorted(tau, s, side="right") - 1, 0, len(tau) - 2)  # the largest k with tau_k <= s, clamped
    alpha = np.clip((s - tau[k]) / (tau[k + 1] - tau[k]), 0.0, 1.0)
    R = _matmul_nn(Rp[k], so3_exp_matrix(alpha[:, None] * phi[k]))
    t = tp[k] + alpha[:, None] * (tp[k + 1] - tp[k])
    return R, t


def deskew_f64(xyz, s, pose_times, poses, T_ref=None) -> np.ndarray:
    """Step 5 before the final rounding, for finite points and finite times: (N, 3) float64."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    R, t = pose_at(s, table(pose_times, poses, T_ref))
    return np.stack([_dot3(R[:, i, 0], R[:, i, 1], R[:, i, 2], p[:, 0], p[:, 1], p[:, 2]) + t[:, i] for i in range(3)], axis=-1)


def deskew(xyz, s, pose_times, poses, T_ref=None) -> np.ndarray:
    """The whole definition, edge cases (step 6) included: (N, 3) float32.  `s`: the times in seconds (see seconds())."""
    p = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    s = np.asarray(s, np.float64)
    out = p.copy()
    finite_p = np.isfinite(p).all(axis=1)
    finite_s = np.isfinite(s)
    out[finite_p & ~finite_s] = np.nan
    ok = finite_p & finite_s
    if ok.any():
        out[ok] = deskew_f64(p[ok], s[ok], pose_times, poses, T_ref).astype(np.float32)
    return out


def max_abs_t(pose_times, poses, T_ref=None) -> float:
    """max |t'_k|: the translation scale of the tolerance's float64 term."""
    return float(np.abs(table(pose_times, poses, T_ref)[2]).max())
