"""Camera calibration without OpenCV: ``cv2.calibrateCamera`` (default flags) from ChArUco corners, on the host and on the GPU.

The reference gets the camera model its poses need from ``cv2.calibrateCamera(object_points, image_points, size, None, None)``
(the reference's src/calib_intrinsics.py:44) on chessboard corners.  This project already has id-labelled sub-pixel corners of a
known planar board in the corner pool ``infer_batch_device`` leaves in HBM, which is what ``cv2.aruco.calibrateCameraCharuco``
calibrates from; this module restates the solve for a planar (z = 0) target and runs it on the device straight from the pool
(``dcx_calibrate_pool``, csrc/dcx_calib.hip).  Steps, all in float64:

1. per-view checks, with the PnP status codes: fewer than 4 points -> TOO_FEW, a homography or initial pose that fails ->
   DEGENERATE / NONFINITE (from a pool also TRUNCATED and BAD_ID).  A failed view is left out of the solve and reported;
2. intrinsics init (OpenCV's initIntrinsicParams2D): principal point at ((w-1)/2, (h-1)/2); per view the Hartley-normalised
   DLT homography of pnp (board xy -> pixels), the principal point subtracted, and two rows in (1/fx^2, 1/fy^2): the
   orthogonality of the normalised h1, h2 and the equal length of the normalised diagonals (h1 +- h2)/2; least squares, f =
   sqrt(|1/f|).  Zero skew, zero distortion.  OpenCV also refines each homography by LM; this does not;
3. extrinsics init: each view's pose is ``pnp._solve`` with K0 and zero distortion (cvFindExtrinsicCameraParams2);
4. joint Levenberg-Marquardt over theta = (fx, fy, cx, cy, k1, k2, p1, p2, k3) and every used view's (rvec, tvec): the CvLevMarq
   rules of ``pnp._solve`` (damping diag(JtJ) * (1 + 10^lg), lg from -3, +1 on a rejected step up to 16, then -1 down to -16; a
   point behind the camera is a rejection) with calibrateCamera's default criteria (at most 30 accepted steps, stop when
   |dp| / |p| < DBL_EPSILON over all 9 + 6N parameters).  Each step is solved by block elimination: every view's 6 pose
   parameters couple only to the 9 intrinsics, so the 6x6 blocks are eliminated (Schur complement) and a 9x9 system remains.

``calibrate_camera_host_full`` is the readable definition and the test pin; ``calibrate_charuco_pool`` /
``calibrate_charuco_device`` run the same steps on the GPU.  The two agree to rounding (summation order), not bit for bit.

Deviations from ``cv2.calibrateCamera``: the homographies of the init are not refined by LM; each LM step is solved by Cholesky
of the reduced system instead of an SVD of the dense one; unusable views are reported instead of raising (``calibrate_camera_host``
raises like cv2).
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import pnp
from .pnp import (PNP_BAD_ID, PNP_NONFINITE, PNP_OK, PNP_TOO_FEW, _cholesky_solve, _homography, _project, _rodrigues, _solve)

# overall status (include/deepcharuco_amd.h); per-view statuses are pnp's PNP_*
CALIB_OK, CALIB_NO_VIEWS, CALIB_DEGENERATE, CALIB_NONFINITE = range(4)
CALIB_MAX_ITER = 30
CALIB_EPS = float(np.finfo(np.float64).eps)
N_INTR = 9                     # fx, fy, cx, cy, k1, k2, p1, p2, k3
RESULT_WORDS = 16              # h_result of dcx_calibrate_pool

__all__ = ["CalibResult", "calibrate_camera_host", "calibrate_camera_host_full", "calibrate_charuco_pool",
           "calibrate_charuco_device", "CALIB_OK", "CALIB_NO_VIEWS", "CALIB_DEGENERATE", "CALIB_NONFINITE"]


class CalibResult(NamedTuple):
    status: int                  # CALIB_*
    rms: float                   # sqrt(sum |r|^2 / points used): cv2.calibrateCamera's return value
    camera_matrix: np.ndarray    # 3x3
    dist_coeffs: np.ndarray      # 1x5: k1 k2 p1 p2 k3
    view_status: np.ndarray      # int32 [B], pnp.PNP_*
    rvecs: np.ndarray            # [B, 3]; zeros unless the view was used
    tvecs: np.ndarray            # [B, 3]
    view_rms: np.ndarray         # [B] rms reprojection error of the view at the solution (px)
    view_points: np.ndarray      # int64 [B]
    iterations: int              # accepted LM steps
    attempts: int                # LM trial steps (accepted + rejected)
    views_used: int
    points_used: int


# ------------------------------------------------------------------------------------------------ the fp64 steps

def _camera_of(theta: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """theta (9) -> (K 3x3, pnp's 8 distortion coefficients k1 k2 p1 p2 k3 0 0 0)."""
    K = np.array([[theta[0], 0.0, theta[2]], [0.0, theta[1], theta[3]], [0.0, 0.0, 1.0]])
    k = np.zeros(8)
    k[:5] = theta[4:9]
    return K, k


def _project_full(obj: np.ndarray, img: np.ndarray, theta: np.ndarray, p: np.ndarray, jac: bool):
    """Residuals (projected - observed, px), cost and with ``jac`` the 2N x 15 Jacobian [d/dtheta (9) | d/d(rvec, tvec) (6)].
    The residuals and the pose columns are ``pnp._project``'s; cost = inf when a point is not in front of the camera."""
    K, k = _camera_of(theta)
    res, cost, Je = _project(obj, img, p, K, k, jac)
    if not jac or res is None:
        return res, cost, None
    R = _rodrigues(p[:3])
    X = obj @ R.T + p[3:]
    iz = 1.0 / X[:, 2]
    x, y = X[:, 0] * iz, X[:, 1] * iz
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    g = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    fx, fy = theta[0], theta[1]
    n = obj.shape[0]
    Ji = np.zeros((n, 2, N_INTR))
    Ji[:, 0, 0] = xd                              # u = fx xd + cx, v = fy yd + cy
    Ji[:, 1, 1] = yd
    Ji[:, 0, 2] = 1.0
    Ji[:, 1, 3] = 1.0
    Ji[:, 0, 4], Ji[:, 1, 4] = fx * (x * r2), fy * (y * r2)                       # k1
    Ji[:, 0, 5], Ji[:, 1, 5] = fx * (x * r4), fy * (y * r4)                       # k2
    Ji[:, 0, 6], Ji[:, 1, 6] = fx * (2 * x * y), fy * (r2 + 2 * y * y)            # p1
    Ji[:, 0, 7], Ji[:, 1, 7] = fx * (r2 + 2 * x * x), fy * (2 * x * y)            # p2
    Ji[:, 0, 8], Ji[:, 1, 8] = fx * (x * r6), fy * (y * r6)                       # k3
    return res, cost, np.concatenate([Ji.reshape(2 * n, N_INTR), Je], 1)


def _init_rows(obj: np.ndarray, img: np.ndarray, cx: float, cy: float) -> Tuple[int, Optional[np.ndarray]]:
    """One view's two rows [a0, a1, b] of initIntrinsicParams2D in the unknowns (1/fx^2, 1/fy^2) -> (status, rows (2, 3))."""
    st, H, _ = _homography(obj, img)
    if st != PNP_OK:
        return st, None
    H = H.copy()
    H[0] -= H[2] * cx                              # the principal point subtracted
    H[1] -= H[2] * cy
    h, v = H[:, 0].copy(), H[:, 1].copy()
    d1, d2 = (h + v) * 0.5, (h - v) * 0.5
    h *= 1.0 / math.sqrt(float(h @ h))
    v *= 1.0 / math.sqrt(float(v @ v))
    d1 *= 1.0 / math.sqrt(float(d1 @ d1))
    d2 *= 1.0 / math.sqrt(float(d2 @ d2))
    rows = np.array([[h[0] * v[0], h[1] * v[1], -h[2] * v[2]], [d1[0] * d2[0], d1[1] * d2[1], -d1[2] * d2[2]]])
    if not np.isfinite(rows).all():
        return PNP_NONFINITE, None
    return PNP_OK, rows


def _init_focal(rows: np.ndarray) -> Optional[Tuple[float, float]]:
    """Least squares of the stacked rows (2N, 3) by the 2x2 normal equations -> (fx, fy), or None if singular."""
    A, b = rows[:, :2], rows[:, 2]
    a00, a01, a11 = float(A[:, 0] @ A[:, 0]), float(A[:, 0] @ A[:, 1]), float(A[:, 1] @ A[:, 1])
    b0, b1 = float(A[:, 0] @ b), float(A[:, 1] @ b)
    det = a00 * a11 - a01 * a01
    if not det > 1e-12 * a00 * a11:
        return None
    f0, f1 = (a11 * b0 - a01 * b1) / det, (a00 * b1 - a01 * b0) / det
    fx, fy = math.sqrt(abs(1.0 / f0)) if f0 != 0 else math.inf, math.sqrt(abs(1.0 / f1)) if f1 != 0 else math.inf
    if not (math.isfinite(fx) and math.isfinite(fy) and fx > 0 and fy > 0):
        return None
    return fx, fy


def _initialise(views, image_size):
    """-> (view status [B], theta0 (9) or None, initial poses [B, 6]).  Statuses as the module docstring; theta0 None when no
    view is left (status NO_VIEWS) or the init's 2x2 system is singular."""
    w, h = image_size
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    B = len(views)
    status = np.full(B, PNP_OK, np.int32)
    poses = np.zeros((B, 6))
    rows = []
    for i, (obj, img) in enumerate(views):
        if obj.shape[0] < 4:
            status[i] = PNP_TOO_FEW
            continue
        st, r = _init_rows(obj, img, cx, cy)
        status[i] = st
        if st == PNP_OK:
            rows.append(r)
    if not rows:
        return status, None, poses
    f = _init_focal(np.concatenate(rows, 0))
    if f is None:
        return status, None, poses
    theta = np.array([f[0], f[1], cx, cy, 0, 0, 0, 0, 0], np.float64)
    K0, k0 = _camera_of(theta)
    for i, (obj, img) in enumerate(views):
        if status[i] == PNP_OK:
            st, pose = _solve(obj, img, K0, k0)
            status[i] = st
            poses[i] = pose[:6]
    return status, theta, poses


def _normal_blocks(views, theta: np.ndarray, poses: np.ndarray):
    """The blocks of JtJ and Jtr over the used views: U [N, 6, 6] (pose-pose), W [N, 9, 6] (intrinsics-pose), V [9, 9]
    (intrinsics-intrinsics, summed), ga [9], gb [N, 6], the per-view costs [N].  None if a point is behind the camera."""
    n = len(views)
    U, W, gb, costs = np.zeros((n, 6, 6)), np.zeros((n, N_INTR, 6)), np.zeros((n, 6)), np.zeros(n)
    V, ga = np.zeros((N_INTR, N_INTR)), np.zeros(N_INTR)
    for i, (obj, img) in enumerate(views):
        res, cost, J = _project_full(obj, img, theta, poses[i], True)
        if res is None:
            return None
        r = res.ravel()
        A, Bm = J[:, :N_INTR], J[:, N_INTR:]
        U[i], W[i], gb[i], costs[i] = Bm.T @ Bm, A.T @ Bm, Bm.T @ r, cost
        V += A.T @ A
        ga += A.T @ r
    return U, W, V, ga, gb, costs


def _schur_step(U, W, V, ga, gb, lg: int):
    """Solve [V* W; W^T U*] [dtheta; dpose] = [ga; gb] with the diagonals of V and of every U_i scaled by 1 + 10^lg (Marquardt),
    by eliminating the pose blocks: S = V* - sum W_i U_i*^-1 W_i^T, dtheta = S^-1 (ga - sum W_i U_i*^-1 gb_i),
    dpose_i = U_i*^-1 (gb_i - W_i^T dtheta).  -> (dtheta [9], dpose [N, 6]), or None if a block is not positive definite."""
    s = 1.0 + 10.0 ** lg
    Us = U.copy()
    d6 = np.arange(6)
    Us[:, d6, d6] *= s
    try:
        np.linalg.cholesky(Us)
    except np.linalg.LinAlgError:
        return None
    Y = np.linalg.solve(Us, W.transpose(0, 2, 1))                  # U_i*^-1 W_i^T  [N, 6, 9]
    z = np.linalg.solve(Us, gb[:, :, None])[:, :, 0]              # U_i*^-1 gb_i   [N, 6]
    S = V.copy()
    S[np.diag_indices(N_INTR)] *= s
    S -= np.einsum("nij,njk->ik", W, Y)
    rhs = ga - np.einsum("nij,nj->i", W, z)
    dt = _cholesky_solve(S, rhs)
    if dt is None:
        return None
    return dt, z - np.einsum("nij,j->ni", Y, dt)


def _view_costs(views, theta, poses) -> np.ndarray:
    return np.array([_project_full(obj, img, theta, poses[i], False)[1] for i, (obj, img) in enumerate(views)])


def _total(costs: np.ndarray) -> float:
    c = 0.0
    for v in costs.tolist():
        c += v
    return c


def _refine(views, theta: np.ndarray, poses: np.ndarray):
    """Joint LM (module docstring, step 4) -> (status, theta, poses, per-view costs, accepted steps, attempts)."""
    blocks = _normal_blocks(views, theta, poses)
    if blocks is None or not math.isfinite(_total(blocks[5])):
        return CALIB_DEGENERATE, theta, poses, None, 0, 0
    vc = blocks[5]
    prev_cost, lg, iters, attempts = _total(vc), -3, 0, 0
    while True:
        U, W, V, ga, gb, _ = blocks
        prev_t, prev_p = theta, poses
        while True:
            step = _schur_step(U, W, V, ga, gb, lg)
            if step is None:
                return CALIB_DEGENERATE, theta, poses, None, iters, attempts
            theta, poses = prev_t - step[0], prev_p - step[1]
            vc = _view_costs(views, theta, poses)
            cost = _total(vc)
            attempts += 1
            if not cost <= prev_cost:              # (a point behind the camera: cost = inf, rejected like an increase)
                lg += 1
                if lg <= 16:
                    continue
            break
        lg = max(lg - 1, -16)
        iters += 1
        d = np.r_[theta - prev_t, (poses - prev_p).ravel()]
        pv = np.r_[prev_t, prev_p.ravel()]
        if iters >= CALIB_MAX_ITER or math.sqrt(float(d @ d)) < CALIB_EPS * math.sqrt(float(pv @ pv)):
            break
        prev_cost = cost
        blocks = _normal_blocks(views, theta, poses)
    if not (np.isfinite(theta).all() and np.isfinite(poses).all()) or math.isnan(cost):
        return CALIB_NONFINITE, theta, poses, None, iters, attempts
    if not math.isfinite(cost):
        return CALIB_DEGENERATE, theta, poses, None, iters, attempts
    return CALIB_OK, theta, poses, vc, iters, attempts


def _views(object_points, image_points):
    if len(object_points) != len(image_points):
        raise ValueError(f"{len(object_points)} object point sets but {len(image_points)} image point sets")
    views = []
    for obj, img in zip(object_points, image_points):
        obj = np.asarray(obj, dtype=np.float64).reshape(-1, 3)
        img = np.asarray(img, dtype=np.float64).reshape(-1, 2)
        if obj.shape[0] != img.shape[0]:
            raise ValueError(f"a view has {obj.shape[0]} object points but {img.shape[0]} image points")
        if obj.size and np.any(obj[:, 2] != 0):
            raise ValueError("non-planar object points: only a planar (z = 0) target is supported")
        if not (np.isfinite(obj).all() and np.isfinite(img).all()):
            raise ValueError("object and image points must be finite")
        views.append((obj, img))
    return views


def _image_size(image_size) -> Tuple[int, int]:
    w, h = (int(v) for v in image_size)
    if w <= 0 or h <= 0:
        raise ValueError(f"image_size {tuple(image_size)} must be positive (width, height)")
    return w, h


def _result(status, theta, view_status, poses, vc, counts, iters, attempts) -> CalibResult:
    B = len(view_status)
    used = np.flatnonzero(view_status == PNP_OK)
    K, dist = np.zeros((3, 3)), np.zeros((1, 5))
    rv, tv, vr = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B)
    rms = 0.0
    if status == CALIB_OK:
        K, _ = _camera_of(theta)
        dist = theta[4:9].reshape(1, 5).copy()
        rv[used], tv[used] = poses[:, :3], poses[:, 3:]
        vr[used] = np.sqrt(vc / counts[used])
        rms = math.sqrt(_total(vc) / int(counts[used].sum()))
    return CalibResult(int(status), float(rms), K, dist, view_status.astype(np.int32), rv, tv, vr, counts.astype(np.int64),
                       int(iters), int(attempts), int(used.size), int(counts[used].sum()))


def calibrate_camera_host_full(object_points, image_points, image_size) -> CalibResult:
    """``cv2.calibrateCamera(object_points, image_points, image_size, None, None)`` for a planar (z = 0) target, in float64 on the
    host, with every output of ``dcx_calibrate_pool`` (``CalibResult``).  Views that fail their checks are left out and reported
    in ``view_status``; ValueError for non-planar or mismatched input or a non-positive image size."""
    w, h = _image_size(image_size)
    views = _views(object_points, image_points)
    counts = np.array([obj.shape[0] for obj, _ in views], np.int64)
    view_status, theta, poses0 = _initialise(views, (w, h))
    used = np.flatnonzero(view_status == PNP_OK)
    if theta is None or not used.size:
        st = CALIB_NO_VIEWS if not used.size else CALIB_DEGENERATE
        return _result(st, theta, view_status, None, None, counts, 0, 0)
    st, theta, poses, vc, iters, attempts = _refine([views[i] for i in used], theta, poses0[used])
    return _result(st, theta, view_status, poses, vc, counts, iters, attempts)


def calibrate_camera_host(object_points, image_points, image_size):
    """cv2's 5-tuple ``(rms, K 3x3, dist 1x5, rvecs, tvecs)`` (rvecs / tvecs: one (3, 1) array per view).  ValueError, as cv2
    errors out, on non-planar objects, a view that cannot be used (fewer than 4 points, degenerate) or a failed calibration."""
    r = calibrate_camera_host_full(object_points, image_points, image_size)
    bad = np.flatnonzero(r.view_status != PNP_OK)
    if bad.size:
        raise ValueError(f"view {int(bad[0])} cannot be used (status {int(r.view_status[bad[0]])})")
    if r.status != CALIB_OK:
        raise ValueError(f"calibration failed (status {r.status})")
    return (r.rms, r.camera_matrix, r.dist_coeffs, tuple(v.reshape(3, 1).copy() for v in r.rvecs),
            tuple(v.reshape(3, 1).copy() for v in r.tvecs))


# ------------------------------------------------------------------------------------------------ the device solver

def workspace_bytes(batch: int) -> int:
    from . import _lib
    return int(_lib.lib().dcx_calibrate_workspace_bytes(int(batch)))


def calibrate_charuco_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len,
                           image_size) -> CalibResult:
    """Calibrate from every frame of an ``infer_batch_device`` result, read in place from the corner pool (the conventions of
    ``pnp.solve_pnp_pool``: ``refined`` = the pool carries RefineNet's xy, else the integer rows are the image points).  Object
    points are ``pnp.object_points``' float32 board corners.  ``image_size`` = (width, height) as in cv2.  The call synchronises
    the current stream (the LM loop reads one state word per step) and cannot be captured in a graph."""
    import torch
    from . import _lib
    w, h = _image_size(image_size)
    dev = packed.device
    if packed.dtype != torch.int32 or not packed.is_contiguous() or packed.numel() < 2 * batch + (6 if refined else 4) * pool:
        raise ValueError("packed must be a contiguous int32 corner pool of at least packed_len(batch, pool) words")
    st = torch.empty((batch,), dtype=torch.int32, device=dev)
    pose = torch.empty((batch, pnp.POSE_WORDS), dtype=torch.float64, device=dev)
    nbytes = workspace_bytes(batch)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    res = (_ctypes.c_double * RESULT_WORDS)()
    base = packed.data_ptr()
    rows_p = base + 8 * batch
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_calibrate_pool(base, base + 4 * batch, rows_p, rows_p + 16 * pool if refined else None,
                                                 int(batch), int(pool), int(col_count), int(row_count), float(square_len), w, h,
                                                 ws.data_ptr(), nbytes, st.data_ptr(), pose.data_ptr(), res,
                                                 _lib.current_stream()), "dcx_calibrate_pool")
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
    r = np.array(res[:], np.float64)
    status = int(r[14])
    K = np.array([[r[0], 0.0, r[2]], [0.0, r[1], r[3]], [0.0, 0.0, 1.0]]) if status == CALIB_OK else np.zeros((3, 3))
    return CalibResult(status, float(r[9]), K, r[4:9].reshape(1, 5).copy(), st_h.astype(np.int32), pose_h[:, 0:3].copy(),
                       pose_h[:, 3:6].copy(), pose_h[:, 6].copy(), pose_h[:, 7].astype(np.int64), int(r[10]), int(r[11]),
                       int(r[12]), int(r[13]))


def calibrate_charuco_device(keypoints_list: Sequence, col_count, row_count, square_len, image_size,
                             device="cuda") -> CalibResult:
    """Calibrate from ``infer_image``-format keypoint arrays ([x, y, id] rows, any number of frames and of corners each) on the
    GPU -> ``CalibResult``.  IndexError if a frame with >= 4 points carries an id outside the board."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    _image_size(image_size)
    if len(keypoints_list) == 0:
        raise ValueError("no views")
    packed, b, pool = pnp._pack(keypoints_list, dev)
    with torch.cuda.device(dev):
        r = calibrate_charuco_pool(packed, b, pool, True, col_count, row_count, square_len, image_size)
    if (r.view_status == PNP_BAD_ID).any():
        n = (col_count - 1) * (row_count - 1)
        raise IndexError(f"corner id outside [0, {n}) for a {col_count}x{row_count} board")
    return r
