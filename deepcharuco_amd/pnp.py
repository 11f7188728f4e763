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

``solve_pnp_ransac_*`` put a consensus search in front of that solver (``cv2.solvePnPRansac``'s role: a corner with a wrong id
sits a board square away from its label, and a least-squares pose has no defence).  ``solve_pnp_ransac_host_full`` is the
definition and carries the steps; ``solve_pnp_ransac_pool`` / ``_batch_device`` / ``_device`` run them in csrc/dcx_pnp_ransac.hip.
The discrete results (winner, mask) are equal on host and device wherever no row stands within rounding of the threshold.
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import List, Optional, Tuple

import numpy as np

from . import _dev, _lm
from ._dev import pool_ptrs as _pool_ptrs
from ._lm import _cholesky_solve     # noqa: F401  (its home is _lm.py; the name it has always had here stays importable)
from .corner_pool import _caller_order, layout, pack_keypoints, views

# per-frame status (include/deepcharuco_amd.h)
PNP_OK, PNP_TOO_FEW, PNP_TRUNCATED, PNP_BAD_ID, PNP_DEGENERATE, PNP_NONFINITE = range(6)
PNP_NO_CONSENSUS = 6            # RANSAC: the best hypothesis has fewer than max(min_inliers, 4) inliers
POSE_WORDS = 8                 # pose[b] = rvec(3), tvec(3), rms reprojection error (px), accepted LM steps

LM_MAX_ITER = 20
LM_EPS = float(np.finfo(np.float32).eps)
UNDISTORT_ITERS = 5
JACOBI_MAX_SWEEPS = 16
RANSAC_MAX_ITERATIONS = 4096
RANSAC_SAMPLE_TRIES = 8        # complete 4-samples drawn per hypothesis before it is given up
RANSAC_MAX_DRAWS = 256         # single slot draws per hypothesis, redraws included
_M32 = 0xFFFFFFFF

__all__ = ["solve_pnp_host", "solve_pnp_host_full", "solve_pnp_device", "solve_pnp_batch_device", "solve_pnp_pool",
           "unpack_poses", "object_points", "PNP_OK", "PNP_TOO_FEW", "PNP_TRUNCATED", "PNP_BAD_ID", "PNP_DEGENERATE",
           "PNP_NONFINITE", "PNP_NO_CONSENSUS", "solve_pnp_ransac_host", "solve_pnp_ransac_host_full", "solve_pnp_ransac_device",
           "solve_pnp_ransac_batch_device", "solve_pnp_ransac_pool", "ransac_workspace_bytes", "unpack_ransac"]


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


def _bad_id_error(col_count, row_count):
    return IndexError(f"corner id outside [0, {(col_count - 1) * (row_count - 1)}) for a {col_count}x{row_count} board")


def object_points(ids, col_count: int, row_count: int, square_len: float) -> np.ndarray:
    """Board-frame corners of ``ids`` exactly as inference.py:20-26 builds them (float32, z = 0), without the full table:
    id i -> ((1 + i % (row_count-1)) * square_len, (1 + i // (row_count-1)) * square_len, 0), each product taken in float64 and
    rounded to float32.  IndexError for an id outside [0, (col_count-1)*(row_count-1))."""
    ids = np.asarray(ids).astype(np.int64)
    n = (col_count - 1) * (row_count - 1)
    if ids.size and (ids.min() < 0 or ids.max() >= n):
        raise _bad_id_error(col_count, row_count)
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


def _distort(x, y, k, jac: bool):
    """The rational + tangential model, the one text of it: normalised (x, y) (arrays) -> (xd, yd, r2) and with ``jac`` also
    (dxd/dx, dxd/dy = dyd/dx, dyd/dy).  ``fisheye._distort`` is the other model in the same shape."""
    r2 = x * x + y * y
    num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]))
    g = num / den
    xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    if not jac:
        return xd, yd, r2
    dg = ((k[0] + r2 * (2 * k[1] + 3 * k[4] * r2)) * den - num * (k[5] + r2 * (2 * k[6] + 3 * k[7] * r2))) / (den * den)
    dxd_dx = g + 2 * x * x * dg + 2 * k[2] * y + 6 * k[3] * x
    dxd_dy = 2 * x * y * dg + 2 * k[2] * x + 2 * k[3] * y
    dyd_dy = g + 2 * y * y * dg + 6 * k[2] * y + 2 * k[3] * x
    return xd, yd, r2, dxd_dx, dxd_dy, dyd_dy


def _project_through(distort, obj: np.ndarray, img: np.ndarray, p: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool):
    """``_project`` for the camera model whose ``distort`` is given -> (residuals, cost, J, (x, y) + what ``distort`` returned, for
    the caller that goes on to the intrinsic columns); the last three of ``distort``'s values with ``jac`` are the model's
    d(xd, yd)/d(x, y) entries (a, b = the off-diagonal pair, d).  (None, inf, None, None) when a point is not in front."""
    R = _rodrigues(p[:3])
    X = obj @ R.T + p[3:]
    if not (X[:, 2] > 0).all():
        return None, math.inf, None, None
    iz = 1.0 / X[:, 2]
    x, y = X[:, 0] * iz, X[:, 1] * iz
    m = distort(x, y, k, jac)
    fx, fy = K[0, 0], K[1, 1]
    res = np.stack([fx * m[0] + K[0, 2] - img[:, 0], fy * m[1] + K[1, 2] - img[:, 1]], 1)
    cost = float((res * res).sum())
    if not jac:
        return res, cost, None, None
    a, b, d = m[-3:]
    # d(x, y)/dX, X = (X, Y, Z) in the camera frame
    n = obj.shape[0]
    dxy_dX = np.zeros((n, 2, 3))
    dxy_dX[:, 0, 0] = iz
    dxy_dX[:, 0, 2] = -x * iz
    dxy_dX[:, 1, 1] = iz
    dxy_dX[:, 1, 2] = -y * iz
    duv_dxy = np.empty((n, 2, 2))
    duv_dxy[:, 0, 0], duv_dxy[:, 0, 1] = fx * a, fx * b
    duv_dxy[:, 1, 0], duv_dxy[:, 1, 1] = fy * b, fy * d
    duv_dX = duv_dxy @ dxy_dX                                        # (n, 2, 3)
    Jr = _right_jacobian(p[:3])
    dX_dr = -np.einsum("ij,njk->nik", R, np.einsum("nij,jk->nik", np.stack([_skew(o) for o in obj]), Jr))
    J = np.empty((n, 2, 6))
    J[:, :, :3] = duv_dX @ dX_dr
    J[:, :, 3:] = duv_dX
    return res, cost, J.reshape(2 * n, 6), (x, y) + m


def _project(obj: np.ndarray, img: np.ndarray, p: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool):
    """Residuals (projected - observed, px) at pose p = (rvec, tvec), their cost, and with ``jac`` the 2N x 6 Jacobian.
    cost = inf when a point is not in front of the camera."""
    return _project_through(_distort, obj, img, p, K, k, jac)[:3]


def _project_q_through(distort, Q: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool):
    """Points Q (n, 3) in a camera's frame -> residuals (projected - observed, px) and, with ``jac``, d(u, v)/dQ (n, 2, 3):
    ``_project_through``'s model and derivatives with the pose taken out (and d(u, v)/dQ by its spelt-out products, not that
    function's matrix product: the two round differently).  Every Z must be positive (the caller checks)."""
    iz = 1.0 / Q[:, 2]
    x, y = Q[:, 0] * iz, Q[:, 1] * iz
    m = distort(x, y, k, jac)
    fx, fy = K[0, 0], K[1, 1]
    res = np.stack([fx * m[0] + K[0, 2] - img[:, 0], fy * m[1] + K[1, 2] - img[:, 1]], 1)
    if not jac:
        return res, None
    a, b, d = m[-3:]
    a0, a1, b0, b1 = fx * a, fx * b, fy * b, fy * d
    D = np.empty((Q.shape[0], 2, 3))
    D[:, 0, 0], D[:, 0, 1], D[:, 0, 2] = a0 * iz, a1 * iz, -(a0 * x + a1 * y) * iz
    D[:, 1, 0], D[:, 1, 1], D[:, 1, 2] = b0 * iz, b1 * iz, -(b0 * x + b1 * y) * iz
    return res, D


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


def _pose_of_homography(H: np.ndarray, mc: np.ndarray) -> Tuple[int, Optional[np.ndarray]]:
    """OpenCV's decomposition (cvFindExtrinsicCameraParams2, planar branch) of H (centred board points -> normalised image
    points, h33 = 1), orthonormalised, with the board centroid mc composed back in -> (status, p0)."""
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


def _init_pose(obj: np.ndarray, mn: np.ndarray) -> Tuple[int, Optional[np.ndarray]]:
    """Planar initialisation (board points obj, normalised image points mn) -> (status, p0)."""
    st, H, mc = _homography(obj, mn)
    if st != PNP_OK:
        return st, None
    return _pose_of_homography(H, mc)


LM_STATUS = (PNP_OK, None, PNP_DEGENERATE, PNP_NONFINITE)      # ``_lm.refine_pose``'s LM_* status -> this module's


def _solve_through(undistort, project, obj: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray) -> Tuple[int, np.ndarray]:
    """``_solve`` for the camera model whose (undistort, project) are given: the planar start on the undistorted points, then
    ``_lm.refine_pose`` on the model's reprojection error."""
    pose = np.zeros(POSE_WORDS)
    obj = obj.astype(np.float64)
    img = img.astype(np.float64)
    mn = undistort(img, K, k)
    if not np.isfinite(mn).all():                # a pixel outside the fisheye model (a pinhole's non-finite point would fail the
        return PNP_DEGENERATE, pose              # homography's rank test with this same answer)
    st, p = _init_pose(obj, mn)
    if st != PNP_OK:
        return st, pose
    st, p, cost, iters = _lm.refine_pose(lambda q, jac: project(obj, img, q, K, k, jac), p, LM_MAX_ITER, LM_EPS)
    if st != _lm.LM_OK:
        return LM_STATUS[st], pose
    pose[:6] = p
    pose[6] = math.sqrt(cost / obj.shape[0])
    pose[7] = iters
    return PNP_OK, pose


def _solve(obj: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray) -> Tuple[int, np.ndarray]:
    """obj (N,3) float32 board points, img (N,2) float32 pixels -> (status, pose[8])."""
    return _solve_through(_undistort, _project, obj, img, K, k)


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


# ------------------------------------------------------------------------------------------------ RANSAC: the definition

def _mix32(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _ransac_draw(seed: int, n: int, h: int, c: int) -> int:
    """Draw ``c`` of hypothesis ``h`` of a frame with ``n`` rows -> a slot in [0, n).  32-bit integer arithmetic only; nothing
    but (seed, n, h, c) enters, so a frame draws the same samples wherever it stands in a batch."""
    r = _mix32((seed & _M32) ^ _mix32(n * 0x9E3779B9 + _mix32(h * 0x85EBCA6B + c)))
    return (r * n) >> 32


def _ransac_sample_ok(ids, rm1: int) -> bool:
    """Four ids make a usable sample: all distinct and no three of their grid points (id % rm1, id // rm1) on a line."""
    if len(set(ids)) < 4:
        return False
    g = [(i % rm1, i // rm1) for i in ids]
    for a, b, c in ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2)):
        if (g[b][0] - g[a][0]) * (g[c][1] - g[a][1]) - (g[b][1] - g[a][1]) * (g[c][0] - g[a][0]) == 0:
            return False
    return True


def _ransac_sample(seed: int, n: int, h: int, ids, rm1: int):
    """The four slots of hypothesis ``h``, or None.  Slots are drawn one by one (a slot already held is redrawn); a complete
    draw whose ids ``_ransac_sample_ok`` refuses is redrawn, 8 draws at most; the draw counter runs on through all of them and
    stops the hypothesis at RANSAC_MAX_DRAWS."""
    c = 0
    for _ in range(RANSAC_SAMPLE_TRIES):
        out = []
        while len(out) < 4:
            if c >= RANSAC_MAX_DRAWS:
                return None
            i = _ransac_draw(seed, n, h, c)
            c += 1
            if i not in out:
                out.append(i)
        if _ransac_sample_ok([int(ids[i]) for i in out], rm1):
            return out
    return None


def _adjugate(m: np.ndarray) -> np.ndarray:
    return np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                     [m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                     [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])


def _projective_basis(p: np.ndarray) -> np.ndarray:
    """3x3 matrix that sends e1, e2, e3, (1,1,1) to the four points p (4,2), each up to scale: columns l_j (x_j, y_j, 1) with
    l = adj([p1 p2 p3]) p4."""
    m = np.array([[p[0, 0], p[1, 0], p[2, 0]], [p[0, 1], p[1, 1], p[2, 1]], [1.0, 1.0, 1.0]])
    lam = _adjugate(m) @ np.array([p[3, 0], p[3, 1], 1.0])
    return m * lam


def _homography4(obj: np.ndarray, mn: np.ndarray) -> Tuple[int, Optional[np.ndarray], np.ndarray]:
    """``_homography`` for exactly four points: the homography through them in closed form (H = B adj(A), A and B the
    projective bases of the centred board points and of the image points) in place of the 9x9 eigenproblem, which four
    points determine exactly anyway.  The sampler has already refused collinear board points."""
    mc = (obj[0, :2] + obj[1, :2] + obj[2, :2] + obj[3, :2]) / 4.0
    H = _projective_basis(mn) @ _adjugate(_projective_basis(obj[:, :2] - mc))
    if not abs(H[2, 2]) > 1e-12 * np.abs(H).max():
        return PNP_DEGENERATE, None, mc
    return PNP_OK, H / H[2, 2], mc


def _row_errors2(obj: np.ndarray, img: np.ndarray, p: np.ndarray, K: np.ndarray, k: np.ndarray, project=None) -> np.ndarray:
    """Squared reprojection error (px^2) of every row at pose p; inf for a row that is not in front of the camera.  ``project``:
    the camera model's ``_project`` (default: this module's)."""
    project = project or _project
    X = obj @ _rodrigues(p[:3]).T + p[3:]
    e2 = np.full(obj.shape[0], math.inf)
    front = X[:, 2] > 0
    if front.any():
        res, _, _ = project(obj[front], img[front], p, K, k, False)
        e2[front] = (res * res).sum(1)
    return e2


def _ransac_args(iterations, reproj_error, min_inliers):
    if not 1 <= int(iterations) <= RANSAC_MAX_ITERATIONS:
        raise ValueError(f"iterations must be in [1, {RANSAC_MAX_ITERATIONS}]")
    if not (math.isfinite(float(reproj_error)) and float(reproj_error) > 0):
        raise ValueError("reproj_error must be finite and positive")
    return int(iterations), float(reproj_error), int(min_inliers)


def solve_pnp_ransac_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                               reproj_error=8.0, min_inliers=4, seed=0, with_margin=False, pool_order=False):
    """The definition of the RANSAC solver (``cv2.solvePnPRansac``'s defaults: 100 iterations, 8 px) ->
    (status, pose[8], inliers bool[N] in the caller's row order, winning hypothesis or -1).

    Rows are taken in the order the corner pool holds them, which is what the sampler's slots count: a keypoint list is laid
    into a pool id-sorted (stable; ``pack_keypoints``), so that is the default; ``pool_order=True`` says the rows already stand as in the
    pool (``infer_batch_device`` leaves a frame's corners in raster order) and takes them as they are.  Hypothesis h = the planar pose through four sampled rows
    (``_ransac_sample``, ``_homography4``, ``_pose_of_homography``; no LM); its score = the rows whose reprojection error
    through the full distortion model is <= reproj_error px (a row not in front of the camera is an outlier).  All ``iterations``
    hypotheses are scored; the winner is the highest score, the lowest h among equals.  No valid hypothesis: DEGENERATE; fewer
    than max(min_inliers, 4) inliers: NO_CONSENSUS; else the pose is ``_solve`` (init + LM) on the winner's inlier rows alone,
    pose[6] their rms, and the mask is the winner's (not recomputed after the refit).  Without a pose the mask is all False.

    ``with_margin``: a fifth value, the smallest |error - reproj_error| / reproj_error of any row under any hypothesis that
    scores within one of the winner: how far the frame is from a decision rounding could flip (inf if there is no winner)."""
    return _ransac_host_full(keypoints, col_count, row_count, square_len, _camera(camera_matrix), _dist(dist_coeffs),
                             (_undistort, _project, _solve), iterations, reproj_error, min_inliers, seed, with_margin, pool_order)


def _ransac_host_full(keypoints, col_count, row_count, square_len, K, k, model, iterations, reproj_error, min_inliers, seed,
                      with_margin, pool_order):
    """``solve_pnp_ransac_host_full`` through a camera model = (undistort, project, solve): this module's, or ``fisheye``'s.  The
    sampler, the four-point pose, the scoring, the selection and the margin are here once.  A sample with a pixel the model
    cannot undistort (NaN; a pinhole has none) has no hypothesis."""
    undistort, project, solve = model
    iterations, thr, min_inliers = _ransac_args(iterations, reproj_error, min_inliers)
    kp = np.asarray(keypoints)
    n = kp.shape[0] if kp.ndim == 2 else 0

    def done(status, pose=None, mask=None, winner=-1, margin=math.inf):
        out = (status, np.zeros(POSE_WORDS) if pose is None else pose, np.zeros(n, bool) if mask is None else mask, winner)
        return out + (margin,) if with_margin else out

    if kp.ndim != 2 or kp.shape[0] < 4:
        return done(PNP_TOO_FEW)
    order = np.arange(kp.shape[0]) if pool_order else np.argsort(kp[:, 2], kind="stable")
    kp = kp[order]
    ids = kp[:, 2].astype(np.int64)
    obj32, img32 = object_points(ids, col_count, row_count, square_len), kp[:, :2].astype(np.float32)
    obj, img = obj32.astype(np.float64), img32.astype(np.float64)
    mn = undistort(img, K, k)
    best, winner, best_e2, records = -1, -1, None, []
    for h in range(iterations):
        s = _ransac_sample(seed, n, h, ids, row_count - 1)
        if s is None or not np.isfinite(mn[s]).all():
            continue
        st, H, mc = _homography4(obj[s], mn[s])
        if st == PNP_OK:
            st, p0 = _pose_of_homography(H, mc)
        if st != PNP_OK:
            continue
        e2 = _row_errors2(obj, img, p0, K, k, project)
        score = int((e2 <= thr * thr).sum())
        records.append((score, e2))
        if score > best:
            best, winner, best_e2 = score, h, e2
    if winner < 0:
        return done(PNP_DEGENERATE)
    margin = min(float(np.abs(np.sqrt(e2[np.isfinite(e2)]) - thr).min()) / thr for sc, e2 in records
                 if sc >= best - 1 and np.isfinite(e2).any())
    if best < max(min_inliers, 4):
        return done(PNP_NO_CONSENSUS, winner=winner, margin=margin)
    m = best_e2 <= thr * thr
    st, pose = solve(obj32[m], img32[m], K, k)
    if st != PNP_OK:
        return done(st, winner=winner, margin=margin)
    mask = np.empty(n, bool)
    mask[order] = m
    return done(st, pose, mask, winner, margin)


def _as_cv2_ransac(status: int, pose: np.ndarray, inliers: np.ndarray):
    return _as_cv2(status, pose) + (inliers,)


def solve_pnp_ransac_host(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                          reproj_error=8.0, min_inliers=4, seed=0):
    """``solve_pnp_host`` with consensus -> (ret, rvec (3,1), tvec (3,1), inliers bool[N]); (False, None, None, all False)
    when no pose comes out.  Same exceptions as ``solve_pnp_host``, and ValueError for a refused iterations / reproj_error."""
    return _as_cv2_ransac(*solve_pnp_ransac_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs,
                                                      iterations, reproj_error, min_inliers, seed)[:3])


# ------------------------------------------------------------------------------------------------ the device solver

def _camera_args(camera_matrix, dist_coeffs):
    K, k = _camera(camera_matrix), _dist(dist_coeffs)
    n = 0 if dist_coeffs is None else int(np.asarray(dist_coeffs).size)
    return (_ctypes.c_double * 9)(*K.ravel().tolist()), (_ctypes.c_double * 8)(*k.tolist()), n


# Every wrapper below has one body for both camera models.  A model is given as what differs: its ``_camera_args`` (this module's
# returns (camera9, dist8, n_dist), ``fisheye``'s (camera9, dist4): the arguments its C entries take at that place, in that order)
# and the C entry, or the model's own wrapper one level down.

def _solve_pool(camera_args, entry, packed, batch, pool, refined, col_count, row_count, square_len, camera_matrix, dist_coeffs, out):
    import torch
    from . import _lib
    dev = packed.device
    ptrs = _pool_ptrs(packed, batch, pool, refined)
    st, pose = (None, None) if out is None else out
    msg = f"out must be (int32 [{batch}], float64 [{batch}, 8]) contiguous tensors on {dev}"
    st = _dev.tensor(st, dev, torch.int32, (batch,), msg, "numel")
    pose = _dev.tensor(pose, dev, torch.float64, (batch, POSE_WORDS), msg, "numel")
    cam = camera_args(camera_matrix, dist_coeffs)
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), entry)(*ptrs, int(batch), int(pool), int(col_count), int(row_count), float(square_len), *cam,
                                              st.data_ptr(), pose.data_ptr(), _lib.current_stream()), entry)
    return st, pose


def solve_pnp_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, camera_matrix, dist_coeffs,
                   out=None):
    """PnP of every frame of an ``infer_batch_device`` result, read in place from the corner pool: enqueued on the current
    stream, no host sync, nothing allocated when ``out`` is given (capture-safe).  ``refined``: the pool carries RefineNet's xy
    (else the integer rows' x, y are the image points).  Returns device tensors ``(status int32 [B], pose float64 [B, 8])``
    (``out`` = that pair, preallocated); ``unpack_poses`` turns them into per-frame ``(ret, rvec, tvec)``."""
    return _solve_pool(_camera_args, "dcx_solve_pnp_pool", packed, batch, pool, refined, col_count, row_count, square_len,
                       camera_matrix, dist_coeffs, out)


def unpack_poses(status, pose) -> List[tuple]:
    """(status [B], pose [B, 8]) (device tensors or host arrays) -> per-frame ``(ret, rvec (3,1), tvec (3,1))`` like cv2's;
    ``(False, None, None)`` for every status but OK."""
    if hasattr(status, "cpu"):
        status, pose = status.cpu().numpy(), pose.cpu().numpy()
    status = np.asarray(status)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, POSE_WORDS)
    return [_as_cv2(int(s), p) for s, p in zip(status.tolist(), pose)]


def _solve_batch_device(camera_args, pool_call, keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs, device):
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    camera_args(camera_matrix, dist_coeffs)                   # ValueError before anything is uploaded
    if len(keypoints_list) == 0:
        return []
    packed, b, pool = pack_keypoints(keypoints_list, dev)
    with torch.cuda.device(dev):
        st, pose = pool_call(packed, b, pool, True, col_count, row_count, square_len, camera_matrix, dist_coeffs)
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
    if (st_h == PNP_BAD_ID).any():
        raise _bad_id_error(col_count, row_count)
    return unpack_poses(st_h, pose_h)


def solve_pnp_batch_device(keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs, device="cuda"):
    """``solve_pnp`` of every frame of a list of keypoint arrays in one kernel launch -> list of ``(ret, rvec, tvec)`` like
    ``solve_pnp_batch``'s (without OpenCV).  IndexError if any frame with >= 4 points carries an id outside the board."""
    return _solve_batch_device(_camera_args, solve_pnp_pool, keypoints_list, col_count, row_count, square_len, camera_matrix,
                               dist_coeffs, device)


def _solve_device(camera_args, batch_call, keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, device):
    kp = np.asarray(keypoints)
    if kp.ndim != 2 or kp.shape[0] < 4:
        camera_args(camera_matrix, dist_coeffs)
        return False, None, None
    return batch_call([kp], col_count, row_count, square_len, camera_matrix, dist_coeffs, device)[0]


def solve_pnp_device(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, device="cuda"):
    """``solve_pnp`` (inference.py:15-29) on the GPU, without OpenCV: same signature, returns ``(ret, rvec, tvec)`` shaped like
    cv2's (bool, (3,1) float64, (3,1) float64); ``(False, None, None)`` for fewer than 4 points or a refused input."""
    return _solve_device(_camera_args, solve_pnp_batch_device, keypoints, col_count, row_count, square_len, camera_matrix,
                         dist_coeffs, device)


# ------------------------------------------------------------------------------------------------ RANSAC on the device

def ransac_workspace_bytes(batch: int, pool: int, iterations: int = 100) -> int:
    """Bytes of device workspace ``solve_pnp_ransac_pool`` needs (every hypothesis' pose and score, the inlier index list)."""
    from . import _lib
    n = int(_lib.lib().dcx_solve_pnp_ransac_workspace_bytes(int(batch), int(pool), int(iterations)))
    if n == 0:
        raise ValueError(f"batch >= 1, pool >= 0 and iterations in [1, {RANSAC_MAX_ITERATIONS}] are required")
    return n


def _ransac_pool(camera_args, entry, packed, batch, pool, refined, col_count, row_count, square_len, camera_matrix, dist_coeffs,
                 iterations, reproj_error, min_inliers, seed, out, workspace):
    import torch
    from . import _lib
    dev = packed.device
    iterations, reproj_error, min_inliers = _ransac_args(iterations, reproj_error, min_inliers)
    ptrs = _pool_ptrs(packed, batch, pool, refined)
    need = ransac_workspace_bytes(batch, pool, iterations)
    workspace = _dev.workspace(workspace, dev, need, f"workspace must be a contiguous tensor of at least {need} bytes on {dev}")
    msg = f"out must be (int32 [{batch}], float64 [{batch}, 8], int32 [{batch}, 2], uint8 [{pool}]) contiguous tensors on {dev}"
    want = ((torch.int32, (batch,)), (torch.float64, (batch, POSE_WORDS)), (torch.int32, (batch, 2)), (torch.uint8, (pool,)))
    if out is not None and len(out) != 4:
        raise ValueError(msg)
    st, pose, info, inl = (_dev.tensor(t, dev, dt, shape, msg, "min", zeros=dt is torch.uint8)
                           for t, (dt, shape) in zip(out or (None,) * 4, want))
    cam = camera_args(camera_matrix, dist_coeffs)
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), entry)(
            *ptrs, int(batch), int(pool), int(col_count), int(row_count), float(square_len), *cam, iterations,
            reproj_error, min_inliers, int(seed) & _M32, workspace.data_ptr(), workspace.numel() * workspace.element_size(),
            st.data_ptr(), pose.data_ptr(), info.data_ptr(), inl.data_ptr(), _lib.current_stream()), entry)
    return st, pose, info, inl


def solve_pnp_ransac_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, camera_matrix,
                          dist_coeffs, iterations=100, reproj_error=8.0, min_inliers=4, seed=0, out=None, workspace=None):
    """``solve_pnp_pool`` behind a consensus search (``solve_pnp_ransac_host_full`` is the definition): two kernel launches on the
    current stream, no host sync, nothing allocated when ``out`` and ``workspace`` are given (capture-safe).  Returns device
    tensors ``(status int32 [B], pose float64 [B, 8], info int32 [B, 2] = inlier count and winning hypothesis (-1: none),
    inliers uint8 [pool] in slot order)``; ``out`` = that tuple, ``workspace`` = a contiguous device tensor of at least
    ``ransac_workspace_bytes(batch, pool, iterations)`` bytes.  Slots of the mask that belong to no frame are not written."""
    return _ransac_pool(_camera_args, "dcx_solve_pnp_ransac_pool", packed, batch, pool, refined, col_count, row_count, square_len,
                        camera_matrix, dist_coeffs, iterations, reproj_error, min_inliers, seed, out, workspace)


def unpack_ransac(status, pose, inliers, counts, starts, ids=None) -> List[tuple]:
    """Host copies of ``solve_pnp_ransac_pool``'s outputs and of the pool's counts / starts -> per-frame
    ``(ret, rvec (3,1), tvec (3,1), inliers bool[counts[b]])``; the mask is all False without a pose.  The masks are in the
    pool's slot order, or, with ``ids`` (the pool's id column, ``rows[:, 2]``), in ``unpack_results``' row order (stable by id)."""
    status, inliers = np.asarray(status), np.asarray(inliers)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, POSE_WORDS)
    out = []
    for b, s in enumerate(status.tolist()):
        n, s0 = int(counts[b]), int(starts[b])
        mask = inliers[s0:s0 + n].astype(bool) if s == PNP_OK else np.zeros(max(n, 0), bool)
        if ids is not None and s == PNP_OK:
            mask = mask[np.argsort(np.asarray(ids[s0:s0 + n]), kind="stable")]
        out.append(_as_cv2_ransac(int(s), pose[b], mask))
    return out


def _ransac_batch_device(camera_args, pool_call, keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs,
                         iterations, reproj_error, min_inliers, seed, device, full):
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    camera_args(camera_matrix, dist_coeffs)                   # ValueError before anything is uploaded
    _ransac_args(iterations, reproj_error, min_inliers)
    if len(keypoints_list) == 0:
        return []
    packed, b, pool = pack_keypoints(keypoints_list, dev)
    with torch.cuda.device(dev):
        st, pose, info, inl = pool_call(packed, b, pool, True, col_count, row_count, square_len, camera_matrix,
                                                    dist_coeffs, iterations, reproj_error, min_inliers, seed)
        st, pose, info, inl, head = (t.cpu().numpy() for t in (st, pose, info, inl, packed[:layout(b, pool).rows]))
    if (st == PNP_BAD_ID).any():
        raise _bad_id_error(col_count, row_count)
    out = []
    for i, (ret, rvec, tvec, mask) in enumerate(unpack_ransac(st, pose, inl, *views(head, b, pool)[:2])):
        mask = mask[_caller_order(keypoints_list[i])]         # undo pack_keypoints' stable id sort
        out.append((int(st[i]), pose[i].copy(), mask, int(info[i, 1])) if full else (ret, rvec, tvec, mask))
    return out


def solve_pnp_ransac_batch_device(keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                                  reproj_error=8.0, min_inliers=4, seed=0, device="cuda", full=False):
    """``solve_pnp_ransac_host`` of every frame of a list of keypoint arrays on the GPU -> list of
    ``(ret, rvec, tvec, inliers)``, ``inliers`` a bool array in the caller's row order.  ``full=True``: list of
    ``(status, pose[8], inliers, winner)`` like ``solve_pnp_ransac_host_full``.  IndexError if any frame with >= 4 points carries
    an id outside the board."""
    return _ransac_batch_device(_camera_args, solve_pnp_ransac_pool, keypoints_list, col_count, row_count, square_len, camera_matrix,
                                dist_coeffs, iterations, reproj_error, min_inliers, seed, device, full)


def _ransac_device(camera_args, batch_call, keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations,
                   reproj_error, min_inliers, seed, device):
    kp = np.asarray(keypoints)
    if kp.ndim != 2 or kp.shape[0] < 4:
        camera_args(camera_matrix, dist_coeffs)
        _ransac_args(iterations, reproj_error, min_inliers)
        return False, None, None, np.zeros(kp.shape[0] if kp.ndim == 2 else 0, bool)
    return batch_call([kp], col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations, reproj_error, min_inliers,
                      seed, device)[0]


def solve_pnp_ransac_device(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                            reproj_error=8.0, min_inliers=4, seed=0, device="cuda"):
    """``cv2.solvePnPRansac``'s role on the GPU, without OpenCV -> ``(ret, rvec, tvec, inliers bool[N])``;
    ``(False, None, None, all False)`` for fewer than 4 points, a refused input or no consensus."""
    return _ransac_device(_camera_args, solve_pnp_ransac_batch_device, keypoints, col_count, row_count, square_len, camera_matrix,
                          dist_coeffs, iterations, reproj_error, min_inliers, seed, device)
