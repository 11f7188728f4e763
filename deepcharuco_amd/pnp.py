"""Board pose without OpenCV: ``solve_pnp`` (/root/reference/src/inference.py:15-29) as a fp64 solver, on the host and on the GPU.

The reference hands its keypoints to ``cv2.solvePnP(obj, img, K, dist)`` with default flags (SOLVEPNP_ITERATIVE, no extrinsic
guess).  This module restates what that call does on a planar board and runs it on the device straight from the corner pool
``infer_batch_device`` leaves in HBM (``dcx_solve_pnp_pool``, csrc/dcx_pnp.hip), so no host sync is needed between detection and
pose.  Steps, all in float64:

1. undistort the image points to normalised coordinates (``undistortPoints``' fixed-point iteration, 5 rounds; 0 / 4 / 5 / 8
   distortion coefficients);
2. initialise: the board is planar (z = 0), so the plane frame is the object points minus their centroid; a homography is fitted
   by DLT on Hartley-normalised points (the 9x9 normal matrix's smallest eigenvector by cyclic Jacobi sweeps), normalised to
   h33 = 1 and decomposed the OpenCV way (h1, h2 normalised, t = h3 * 2 / (|h1| + |h2|), h3 = h1 x h2, orthonormalised: the
   polar factor, which is what Rodrigues' SVD gives), then the centroid is composed back in;
3. refine by Levenberg-Marquardt on the pixel reprojection error of the full distortion model: 6 parameters (Rodrigues rvec,
   tvec), analytic Jacobian, Marquardt damping diag(JtJ) * (1 + lambda), lambda from 1e-3 by x10 / /10, a rejected step is
   retried from the same point with a larger lambda, at most 20 accepted steps, stop when |dp| / |p| < FLT_EPSILON.

``solve_pnp_host`` is the readable definition and the test pin; ``solve_pnp_device`` / ``solve_pnp_batch_device`` /
``solve_pnp_pool`` run the same steps in the HIP kernel.  The two agree to rounding (summation order), not bit for bit, and
neither is bit-identical to OpenCV (its internal summation orders and its homography refinement are not restated).

Deviation from ``cv2.solvePnP``: input the reference never meets -- collinear points, a rank-deficient homography, a point
behind the camera, a non-finite result -- is reported as ``ret = False`` (status DEGENERATE / NONFINITE) instead of a
meaningless pose.  A step of the refinement that would put a point behind the camera counts as a rejected step.
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

# per-frame status (include/deepcharuco_amd.h)
PNP_OK, PNP_TOO_FEW, PNP_TRUNCATED, PNP_BAD_ID, PNP_DEGENERATE, PNP_NONFINITE = range(6)
POSE_WORDS = 8                 # pose[b] = rvec(3), tvec(3), rms reprojection error (px), accepted LM steps

LM_MAX_ITER = 20
LM_EPS = float(np.finfo(np.float32).eps)
UNDISTORT_ITERS = 5
JACOBI_MAX_SWEEPS = 16

__all__ = ["solve_pnp_host", "solve_pnp_host_full", "solve_pnp_device", "solve_pnp_batch_device", "solve_pnp_pool",
           "unpack_poses", "object_points", "PNP_OK", "PNP_TOO_FEW", "PNP_TRUNCATED", "PNP_BAD_ID", "PNP_DEGENERATE",
           "PNP_NONFINITE"]


# ------------------------------------------------------------------------------------------------ arguments

def _camera(camera_matrix) -> np.ndarray:
    K = np.asarray(camera_matrix, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("camera_matrix must be 3x3")
    if K[0, 1] != 0.0:
        raise ValueError("camera_matrix with skew (K[0,1] != 0) is not supported")
    if not (np.isfinite(K).all() and K[0, 0] != 0.0 and K[1, 1] != 0.0):
        raise ValueError("camera_matrix needs finite entries and non-zero fx, fy")
    return K


def _dist(dist_coeffs) -> np.ndarray:
    """-> 8 coefficients (k1, k2, p1, p2, k3, k4, k5, k6), zero padded; 12 / 14 (thin prism, tilt) are refused."""
    d = np.zeros(0) if dist_coeffs is None else np.asarray(dist_coeffs, dtype=np.float64).ravel()
    if d.size not in (0, 4, 5, 8):
        raise ValueError(f"{d.size} distortion coefficients: only 0, 4, 5 or 8 are supported")
    if not np.isfinite(d).all():
        raise ValueError("distortion coefficients must be finite")
    out = np.zeros(8)
    out[:d.size] = d
    return out


def object_points(ids, col_count: int, row_count: int, square_len: float) -> np.ndarray:
    """Board-frame corners of ``ids`` exactly as inference.py:20-26 builds them (float32, z = 0), without the full table:
    id i -> ((1 + i % (row_count-1)) * square_len, (1 + i // (row_count-1)) * square_len, 0), each product taken in float64 and
    rounded to float32.  IndexError for an id outside [0, (col_count-1)*(row_count-1))."""
    ids = np.asarray(ids).astype(np.int64)
    n = (col_count - 1) * (row_count - 1)
    if ids.size and (ids.min() < 0 or ids.max() >= n):
        raise IndexError(f"corner id outside [0, {n}) for a {col_count}x{row_count} board")
    out = np.zeros((ids.size, 3), np.float32)
    out[:, 0] = (1 + ids % (row_count - 1)) * float(square_len)
    out[:, 1] = (1 + ids // (row_count - 1)) * float(square_len)
    return out


# ------------------------------------------------------------------------------------------------ the fp64 steps

def _undistort(img: np.ndarray, K: np.ndarray, k: np.ndarray) -> np.ndarray:
    """undistortPoints: pixels -> normalised coordinates, 5 fixed-point rounds (none without distortion)."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x0 = (img[:, 0] - cx) / fx
    y0 = (img[:, 1] - cy) / fy
    if not k.any():
        return np.stack([x0, y0], 1)
    out = np.empty((img.shape[0], 2))
    for i in range(img.shape[0]):
        x, y = x0[i], y0[i]
        for _ in range(UNDISTORT_ITERS):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            if icdist < 0:            # as OpenCV: give up on this point, keep the distorted coordinates
                x, y = x0[i], y0[i]
                break
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
            x = (x0[i] - dx) * icdist
            y = (y0[i] - dy) * icdist
        out[i] = x, y
    return out


def _jacobi(a: np.ndarray):
    """Cyclic Jacobi on a symmetric matrix (sweeps over the pairs p < q in row order): -> (eigenvalues, V) with
    a = V diag(w) V^T.  Stops when the off-diagonal mass is below 1e-30 of the diagonal's, or after 16 sweeps."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    v = np.eye(n)
    for _ in range(JACOBI_MAX_SWEEPS):
        off = sum(a[p, q] * a[p, q] for p in range(n) for q in range(p + 1, n))
        dia = sum(a[p, p] * a[p, p] for p in range(n))
        if not off > 1e-30 * dia:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                ap, aq = a[:, p].copy(), a[:, q].copy()
                a[:, p] = c * ap - s * aq
                a[:, q] = s * ap + c * aq
                ap, aq = a[p, :].copy(), a[q, :].copy()
                a[p, :] = c * ap - s * aq
                a[q, :] = s * ap + c * aq
                a[p, q] = a[q, p] = 0.0
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p] = c * vp - s * vq
                v[:, q] = s * vp + c * vq
    return np.diag(a).copy(), v


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def _rodrigues(r: np.ndarray) -> np.ndarray:
    th = math.sqrt(float(r @ r))
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    K = _skew(k)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _rvec_of(R: np.ndarray) -> np.ndarray:
    """Rodrigues vector of an orthonormal matrix (cvRodrigues2's matrix -> vector branch after its SVD)."""
    rx, ry, rz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    s = math.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
    c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5, -1.0), 1.0)
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        x = math.sqrt(max((R[0, 0] + 1) * 0.5, 0.0))
        y = math.sqrt(max((R[1, 1] + 1) * 0.5, 0.0)) * (-1.0 if R[0, 1] < 0 else 1.0)
        z = math.sqrt(max((R[2, 2] + 1) * 0.5, 0.0)) * (-1.0 if R[0, 2] < 0 else 1.0)
        if abs(x) < abs(y) and abs(x) < abs(z) and (R[1, 2] > 0) != (y * z > 0):
            z = -z
        r = np.array([x, y, z])
        return r * (math.pi / math.sqrt(float(r @ r)))
    return np.array([rx, ry, rz]) * (theta / (2 * s))


def _right_jacobian(r: np.ndarray) -> np.ndarray:
    """J_r of SO(3): d(R(r) u)/dr = -R [u]x J_r(r)."""
    th2 = float(r @ r)
    if th2 < 1e-8:
        a, b = 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = math.sqrt(th2)
        a, b = (1 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    S = _skew(r)
    return np.eye(3) - a * S + b * (S @ S)


def _project(obj: np.ndarray, img: np.ndarray, p: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool):
    """Residuals (projected - observed, px) at pose p = (rvec, tvec), their cost, and with ``jac`` the 2N x 6 Jacobian.
    cost = inf when a point is not in front of the camera."""
    R = _rodrigues(p[:3])
    X = obj @ R.T + p[3:]
    if not (X[:, 2] > 0).all():
        return None, math.inf, None
    iz = 1.0 / X[:, 2]
    x, y = X[:, 0] * iz, X[:, 1] * iz
    r2 = x * x + y * y
    num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]))
    g = num / den
    xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    fx, fy = K[0, 0], K[1, 1]
    res = np.stack([fx * xd + K[0, 2] - img[:, 0], fy * yd + K[1, 2] - img[:, 1]], 1)
    cost = float((res * res).sum())
    if not jac:
        return res, cost, None
    dg = ((k[0] + r2 * (2 * k[1] + 3 * k[4] * r2)) * den - num * (k[5] + r2 * (2 * k[6] + 3 * k[7] * r2))) / (den * den)
    dxd_dx = g + 2 * x * x * dg + 2 * k[2] * y + 6 * k[3] * x
    dxd_dy = 2 * x * y * dg + 2 * k[2] * x + 2 * k[3] * y
    dyd_dx = 2 * x * y * dg + 2 * k[2] * x + 2 * k[3] * y
    dyd_dy = g + 2 * y * y * dg + 6 * k[2] * y + 2 * k[3] * x
    # d(x, y)/dX, X = (X, Y, Z) in the camera frame
    n = obj.shape[0]
    dxy_dX = np.zeros((n, 2, 3))
    dxy_dX[:, 0, 0] = iz
    dxy_dX[:, 0, 2] = -x * iz
    dxy_dX[:, 1, 1] = iz
    dxy_dX[:, 1, 2] = -y * iz
    duv_dxy = np.empty((n, 2, 2))
    duv_dxy[:, 0, 0], duv_dxy[:, 0, 1] = fx * dxd_dx, fx * dxd_dy
    duv_dxy[:, 1, 0], duv_dxy[:, 1, 1] = fy * dyd_dx, fy * dyd_dy
    duv_dX = duv_dxy @ dxy_dX                                        # (n, 2, 3)
    Jr = _right_jacobian(p[:3])
    dX_dr = -np.einsum("ij,njk->nik", R, np.einsum("nij,jk->nik", np.stack([_skew(o) for o in obj]), Jr))
    J = np.empty((n, 2, 6))
    J[:, :, :3] = duv_dX @ dX_dr
    J[:, :, 3:] = duv_dX
    return res, cost, J.reshape(2 * n, 6)


def _homography(obj: np.ndarray, mn: np.ndarray) -> Tuple[int, Optional[np.ndarray], np.ndarray]:
    """Planar DLT (board points obj, image points mn) -> (status, H, mc): H maps the centred board points (obj xy - mc) to mn,
    normalised to h33 = 1."""
    n = obj.shape[0]
    mc, ic = obj[:, :2].mean(0), mn.mean(0)
    mxy, ixy = obj[:, :2] - mc, mn - ic                # plane frame: the board's own z = 0 plane, origin at the centroid
    sxx, sxy, syy = (mxy[:, 0] ** 2).sum(), (mxy[:, 0] * mxy[:, 1]).sum(), (mxy[:, 1] ** 2).sum()
    tr, rt = sxx + syy, math.sqrt((sxx - syy) ** 2 + 4 * sxy * sxy)
    if not 0.5 * (tr - rt) > 1e-10 * 0.5 * (tr + rt):    # collinear board points: no homography
        return PNP_DEGENERATE, None, mc
    # Hartley normalisation: centred, mean distance sqrt(2)
    d1, d2 = np.sqrt((mxy ** 2).sum(1)).sum() / n, np.sqrt((ixy ** 2).sum(1)).sum() / n
    sc1 = math.sqrt(2.0) / d1 if d1 > 0 else 0.0
    sc2 = math.sqrt(2.0) / d2 if d2 > 0 else 0.0
    a, b = sc1 * mxy, sc2 * ixy
    M = np.zeros((9, 9))
    for (X, Y), (u, v) in zip(a, b):
        r1 = np.array([X, Y, 1, 0, 0, 0, -u * X, -u * Y, -u])
        r2 = np.array([0, 0, 0, X, Y, 1, -v * X, -v * Y, -v])
        M += np.outer(r1, r1) + np.outer(r2, r2)
    w, V = _jacobi(M)
    order = np.argsort(w, kind="stable")
    if not w[order[1]] > 1e-12 * np.abs(w).max():       # two (near) null directions: rank-deficient homography
        return PNP_DEGENERATE, None, mc
    # H = T2^-1 Hn T1 with T1 = diag(sc1, sc1, 1), T2^-1 = [[1/sc2, 0, icx], [0, 1/sc2, icy], [0, 0, 1]]
    H = V[:, order[0]].reshape(3, 3) * np.array([sc1, sc1, 1.0])
    H[0] = H[0] / sc2 + ic[0] * H[2]
    H[1] = H[1] / sc2 + ic[1] * H[2]
    if not abs(H[2, 2]) > 1e-12 * np.abs(H).max():
        return PNP_DEGENERATE, None, mc
    return PNP_OK, H / H[2, 2], mc


def _init_pose(obj: np.ndarray, mn: np.ndarray) -> Tuple[int, Optional[np.ndarray]]:
    """Planar initialisation (board points obj, normalised image points mn) -> (status, p0)."""
    st, H, mc = _homography(obj, mn)
    if st != PNP_OK:
        return st, None
    # OpenCV's decomposition (cvFindExtrinsicCameraParams2, planar branch)
    h1, h2, h3 = H[:, 0], H[:, 1], H[:, 2]
    n1, n2 = math.sqrt(float(h1 @ h1)), math.sqrt(float(h2 @ h2))
    h1 = h1 * (1.0 / max(n1, 2.2e-16))
    h2 = h2 * (1.0 / max(n2, 2.2e-16))
    t = h3 * (2.0 / max(n1 + n2, 2.2e-16))
    Rr = np.stack([h1, h2, np.cross(h1, h2)], 1)
    ws, W = _jacobi(Rr.T @ Rr)                  # polar factor Rr (Rr^T Rr)^-1/2 = U V^T of Rr's SVD
    if not ws.min() > 0:
        return PNP_DEGENERATE, None
    Q = Rr @ (W @ np.diag(1.0 / np.sqrt(ws)) @ W.T)
    r = _rvec_of(Q)
    t = t - _rodrigues(r)[:, :2] @ mc
    p0 = np.r_[r, t]
    if not np.isfinite(p0).all():
        return PNP_NONFINITE, None
    return PNP_OK, p0


def _cholesky_solve(A: np.ndarray, b: np.ndarray) -> Optional[np.ndarray]:
    n = A.shape[0]
    L = np.zeros_like(A)
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j] - float(L[i, :j] @ L[j, :j])
            if i == j:
                if not s > 0:
                    return None
                L[i, i] = math.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = (y[i] - float(L[i + 1:, i] @ x[i + 1:])) / L[i, i]
    return x


def _solve(obj: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray) -> Tuple[int, np.ndarray]:
    """obj (N,3) float32 board points, img (N,2) float32 pixels -> (status, pose[8])."""
    pose = np.zeros(POSE_WORDS)
    obj = obj.astype(np.float64)
    img = img.astype(np.float64)
    st, p = _init_pose(obj, _undistort(img, K, k))
    if st != PNP_OK:
        return st, pose
    res, cost, J = _project(obj, img, p, K, k, True)
    if not math.isfinite(cost):
        return PNP_DEGENERATE, pose
    prev_cost, lg, iters = cost, -3, 0
    while True:
        JtJ, Jtr = J.T @ J, J.T @ res.ravel()
        prev = p
        while True:
            A = JtJ.copy()
            A[np.diag_indices(6)] *= 1.0 + 10.0 ** lg
            x = _cholesky_solve(A, Jtr)
            if x is None:
                return PNP_DEGENERATE, pose
            p = prev - x
            _, cost, _ = _project(obj, img, p, K, k, False)
            if not cost <= prev_cost:           # (a point behind the camera: cost = inf, rejected like an increase)
                lg += 1
                if lg <= 16:
                    continue
            break
        lg = max(lg - 1, -16)
        iters += 1
        if iters >= LM_MAX_ITER or math.sqrt(float((p - prev) @ (p - prev))) < LM_EPS * math.sqrt(float(prev @ prev)):
            break
        prev_cost = cost
        res, cost, J = _project(obj, img, p, K, k, True)
    if not np.isfinite(p).all() or math.isnan(cost):
        return PNP_NONFINITE, pose
    if not math.isfinite(cost):
        return PNP_DEGENERATE, pose
    pose[:6] = p
    pose[6] = math.sqrt(cost / obj.shape[0])
    pose[7] = iters
    return PNP_OK, pose


def solve_pnp_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs):
    """``solve_pnp_host`` with the kernel's outputs: (status, pose[8] = rvec, tvec, rms px, accepted LM steps)."""
    K, k = _camera(camera_matrix), _dist(dist_coeffs)
    kp = np.asarray(keypoints)
    if kp.ndim != 2 or kp.shape[0] < 4:
        return PNP_TOO_FEW, np.zeros(POSE_WORDS)
    obj = object_points(kp[:, 2], col_count, row_count, square_len)
    return _solve(obj, kp[:, :2].astype(np.float32), K, k)


def _as_cv2(status: int, pose: np.ndarray):
    if status != PNP_OK:
        return False, None, None
    return True, pose[0:3].reshape(3, 1).copy(), pose[3:6].reshape(3, 1).copy()


def solve_pnp_host(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs):
    """``solve_pnp`` (inference.py:15-29) on the host in float64 without OpenCV -> (ret, rvec (3,1), tvec (3,1)).
    (False, None, None) for fewer than 4 points or input the solver refuses (module docstring); IndexError for an id outside
    the board, ValueError for 12 / 14 distortion coefficients or a skewed camera matrix."""
    return _as_cv2(*solve_pnp_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs))


# ------------------------------------------------------------------------------------------------ the device solver

def _camera_args(camera_matrix, dist_coeffs):
    K, k = _camera(camera_matrix), _dist(dist_coeffs)
    n = 0 if dist_coeffs is None else int(np.asarray(dist_coeffs).size)
    return (_ctypes.c_double * 9)(*K.ravel().tolist()), (_ctypes.c_double * 8)(*k.tolist()), n


def _launch(counts_p, starts_p, rows_p, xy_p, batch, pool, col_count, row_count, square_len, camera_matrix, dist_coeffs,
            status_p, pose_p):
    from . import _lib
    cam, dist, n_dist = _camera_args(camera_matrix, dist_coeffs)
    _lib.check(_lib.lib().dcx_solve_pnp_pool(counts_p, starts_p, rows_p, xy_p, int(batch), int(pool), int(col_count),
                                             int(row_count), float(square_len), cam, dist, n_dist, status_p, pose_p,
                                             _lib.current_stream()), "dcx_solve_pnp_pool")


def solve_pnp_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, camera_matrix, dist_coeffs,
                   out=None):
    """PnP of every frame of an ``infer_batch_device`` result, read in place from the corner pool: enqueued on the current
    stream, no host sync, nothing allocated when ``out`` is given (capture-safe).  ``refined``: the pool carries RefineNet's xy
    (else the integer rows' x, y are the image points).  Returns device tensors ``(status int32 [B], pose float64 [B, 8])``
    (``out`` = that pair, preallocated); ``unpack_poses`` turns them into per-frame ``(ret, rvec, tvec)``."""
    import torch
    dev = packed.device
    if packed.dtype != torch.int32 or not packed.is_contiguous() or packed.numel() < 2 * batch + (6 if refined else 4) * pool:
        raise ValueError("packed must be a contiguous int32 corner pool of at least packed_len(batch, pool) words")
    if out is None:
        out = (torch.empty((batch,), dtype=torch.int32, device=dev),
               torch.empty((batch, POSE_WORDS), dtype=torch.float64, device=dev))
    st, pose = out
    if (st.device != dev or st.dtype != torch.int32 or st.numel() != batch or not st.is_contiguous() or pose.device != dev
            or pose.dtype != torch.float64 or pose.numel() != batch * POSE_WORDS or not pose.is_contiguous()):
        raise ValueError(f"out must be (int32 [{batch}], float64 [{batch}, 8]) contiguous tensors on {dev}")
    base = packed.data_ptr()
    rows_p = base + 8 * batch
    with torch.cuda.device(dev):
        _launch(base, base + 4 * batch, rows_p, rows_p + 16 * pool if refined else None, batch, pool, col_count, row_count,
                square_len, camera_matrix, dist_coeffs, st.data_ptr(), pose.data_ptr())
    return st, pose


def unpack_poses(status, pose) -> List[tuple]:
    """(status [B], pose [B, 8]) (device tensors or host arrays) -> per-frame ``(ret, rvec (3,1), tvec (3,1))`` like cv2's;
    ``(False, None, None)`` for every status but OK."""
    if hasattr(status, "cpu"):
        status, pose = status.cpu().numpy(), pose.cpu().numpy()
    status = np.asarray(status)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, POSE_WORDS)
    return [_as_cv2(int(s), p) for s, p in zip(status.tolist(), pose)]


def _pack(keypoints_list: Sequence, dev):
    """Host keypoint lists -> a device corner pool (counts | starts | rows | xy), frames id-sorted like the reference."""
    import torch
    b = len(keypoints_list)
    kps = []
    for kp in keypoints_list:
        kp = np.asarray(kp)
        kps.append(kp.reshape(-1, 3) if kp.size else np.zeros((0, 3)))
    counts = np.array([k.shape[0] for k in kps], np.int64)
    pool = max(int(counts.sum()), 1)
    packed = np.zeros(2 * b + 6 * pool, np.int32)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    packed[:b], packed[b:2 * b] = counts, starts
    rows = packed[2 * b:2 * b + 4 * pool].reshape(pool, 4)
    xy = packed[2 * b + 4 * pool:].view(np.float32).reshape(pool, 2)
    for kp, s in zip(kps, starts.tolist()):
        if not kp.shape[0]:
            continue
        kp = kp[np.argsort(kp[:, 2], kind="stable")]           # inference.py:68-69
        ids = kp[:, 2].astype(np.int64)
        rows[s:s + kp.shape[0], 2] = np.clip(ids, -1, np.iinfo(np.int32).max)
        xy[s:s + kp.shape[0]] = kp[:, :2].astype(np.float32)
    return torch.from_numpy(packed).to(dev), b, pool


def solve_pnp_batch_device(keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs, device="cuda"):
    """``solve_pnp`` of every frame of a list of keypoint arrays in one kernel launch -> list of ``(ret, rvec, tvec)`` like
    ``solve_pnp_batch``'s (without OpenCV).  IndexError if any frame with >= 4 points carries an id outside the board."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    _camera_args(camera_matrix, dist_coeffs)                  # ValueError before anything is uploaded
    if len(keypoints_list) == 0:
        return []
    packed, b, pool = _pack(keypoints_list, dev)
    with torch.cuda.device(dev):
        st, pose = solve_pnp_pool(packed, b, pool, True, col_count, row_count, square_len, camera_matrix, dist_coeffs)
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
    if (st_h == PNP_BAD_ID).any():
        n = (col_count - 1) * (row_count - 1)
        raise IndexError(f"corner id outside [0, {n}) for a {col_count}x{row_count} board")
    return unpack_poses(st_h, pose_h)


def solve_pnp_device(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, device="cuda"):
    """``solve_pnp`` (inference.py:15-29) on the GPU, without OpenCV: same signature, returns ``(ret, rvec, tvec)`` shaped like
    cv2's (bool, (3,1) float64, (3,1) float64); ``(False, None, None)`` for fewer than 4 points or a refused input."""
    kp = np.asarray(keypoints)
    if kp.ndim != 2 or kp.shape[0] < 4:
        _camera_args(camera_matrix, dist_coeffs)
        return False, None, None
    return solve_pnp_batch_device([kp], col_count, row_count, square_len, camera_matrix, dist_coeffs, device)[0]
