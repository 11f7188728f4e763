"""The fisheye camera model without OpenCV: what a cv2 user calls ``cv2.fisheye.projectPoints`` / ``undistortPoints`` / ``calibrate``
/ ``initUndistortRectifyMap`` and ``solvePnP`` on a fisheye camera, on the host and on the GPU (csrc/dcx_fisheye.hip on
csrc/dcx_fisheye_dev.h).  The pinhole with rational and tangential distortion (``pnp``, ``calib``, ``rectify``) is a polynomial in
tan(theta) and cannot fit a lens past about 100 degrees of field; this model is a polynomial in theta.

The model (OpenCV's documented ``cv2.fisheye``, skew 0).  For a camera-frame point (X, Y, Z):

    a = X / Z, b = Y / Z, r = sqrt(a^2 + b^2), theta = atan r,
    theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
    x' = (theta_d / r) a, y' = (theta_d / r) b, u = fx x' + cx, v = fy y' + cy.

Eight intrinsics: fx, fy, cx, cy, k1..k4.  As everywhere in this package a point must have Z > 0, so the field of view is under 180
degrees (theta in [0, pi/2)).  s = theta_d / r and w = (ds/dr) / r are taken by their series in r^2 below r = ``SMALL_R`` (no
division by r): a point exactly on the optical axis is a valid input.

The inverse (pixel -> theta) is Newton on theta (1 + k1 theta^2 + ...) - theta_d from theta = theta_d, run to convergence as
``rectify.undistort_points_newton`` does (``NEWTON_MAX_ITER``, ``NEWTON_EPS``).  A pixel is OUTSIDE (NaN for points,
``MAP_SENTINEL`` in a map) if Newton does not converge or theta is not in [0, pi/2).

* pose: ``pnp``'s solver (planar DLT on the undistorted points, OpenCV's decomposition, Levenberg-Marquardt with CvLevMarq's
  rules: 20 accepted steps, |dp| / |p| < FLT_EPSILON) through this model; a frame with a pixel outside the model is DEGENERATE;
* calibration: joint Levenberg-Marquardt over the 8 intrinsics and every used view's pose with ``calib``'s rules and Schur
  elimination (``_lm.refine``).  This model has no closed-form start: the principal point starts at ((w-1)/2, (h-1)/2),
  fx = fy = ``focal0`` or, if that is not > 0, max(w, h) / 2 (at which every in-frame pixel undistorts: sqrt(2) < pi / 2), k = 0,
  and every view's pose is the fisheye pose solve at that camera.  The start being cruder than Zhang's, the cap is 100 accepted
  steps, not 30.  On noise-free 640 x 480 scenes of 12 views and 28 corners that start reached the truth for true focal lengths of
  150, 230 and 400 px in 8 - 35 accepted steps (with max(w, h) / pi the 400 px lens is refused at the init); it rests on those
  few scenes and nothing more;
* the undistort + rectify map and the rectified points: ``rectify``'s steps 2 and 3 with the ray through this model; the map has
  ``rectify``'s fixed-point format, so ``rectify.remap_device`` warps through it unchanged.

The ``*_host`` functions are the readable fp64 definitions and the pins of the kernels; host and device agree to rounding
(summation order, libm), not bit for bit.  A fisheye camera inside a rig is ``rig``'s ``models`` keyword, which takes this
module's ``_solve`` and ``_project_q``, and so does ``stereo``'s for a pair; the consensus pose (``solve_pnp_fisheye_ransac_*``)
is ``pnp``'s search run through this model.  Not here: fisheye inside ``calib.calibrate_charuco_ransac_*`` (its raw-pixel
homography consensus does not hold through a fisheye lens), skew, cv2's CALIB_* flags, fields of 180 degrees and more; bit parity
with cv2 is not claimed.
"""
from __future__ import annotations

import ctypes as _ctypes
import functools
import math
from typing import Sequence, Tuple

import numpy as np

from . import _dev, pnp
from .calib import (CALIB_NO_VIEWS, CAMERA_FISHEYE, RESULT_WORDS, CalibResult, CalibUncertainty, _camera_matrix, _common_fields, _cv2_tuple,
                    _image_size, _no_bad_id, _refine, _result, _uncertainty_device, _uncertainty_host, _uncertainty_pool, _upload,
                    _view_outputs, _views)
from .pnp import PNP_OK, PNP_TOO_FEW, POSE_WORDS, _as_cv2, _camera, _pool_ptrs, _rodrigues, object_points
from .rectify import (NEWTON_EPS, NEWTON_MAX_ITER, Rectification, _map_device, _points_pool, _projections, _rectify_map,
                      _rectify_points, _rectifying_rotations)

SMALL_R = 1e-4                 # below it theta_d / r and its derivative come from their series
SMALL_THETA_D = 1e-8           # below it tan(theta) / theta_d = 1 to the last bit
N_INTR = 8                     # fx, fy, cx, cy, k1, k2, k3, k4
N_DIST = 4                     # k1, k2, k3, k4
CALIB_MAX_ITER = 100           # accepted steps of the joint LM

__all__ = ["project_points_host", "undistort_points_host", "solve_pnp_fisheye_host", "solve_pnp_fisheye_host_full",
           "calibrate_fisheye_host", "calibrate_fisheye_host_full", "undistort_rectify_map_fisheye_host",
           "rectify_points_fisheye_host", "stereo_rectify_fisheye_host", "solve_pnp_fisheye_pool",
           "solve_pnp_fisheye_batch_device", "solve_pnp_fisheye_device", "solve_pnp_fisheye_ransac_host_full",
           "solve_pnp_fisheye_ransac_host", "solve_pnp_fisheye_ransac_pool", "solve_pnp_fisheye_ransac_batch_device",
           "solve_pnp_fisheye_ransac_device",
           "calibrate_fisheye_pool", "calibrate_fisheye_device", "workspace_bytes", "undistort_rectify_map_fisheye_device",
           "rectify_points_fisheye_pool", "SMALL_R", "CALIB_MAX_ITER", "calibration_uncertainty_fisheye_host",
           "calibration_uncertainty_fisheye_pool", "calibration_uncertainty_fisheye_device"]


# ------------------------------------------------------------------------------------------------ arguments

def _dist4(dist_coeffs) -> np.ndarray:
    """-> (k1, k2, k3, k4); None is four zeros."""
    d = np.zeros(4) if dist_coeffs is None else np.asarray(dist_coeffs, dtype=np.float64).ravel()
    if d.size != 4:
        raise ValueError(f"{d.size} distortion coefficients: the fisheye model has 4 (k1, k2, k3, k4)")
    if not np.isfinite(d).all():
        raise ValueError("distortion coefficients must be finite")
    return d.copy()


def _camera_args(camera_matrix, dist_coeffs):
    K, k = _camera(camera_matrix), _dist4(dist_coeffs)
    return (_ctypes.c_double * 9)(*K.ravel().tolist()), (_ctypes.c_double * 4)(*k.tolist())


# ------------------------------------------------------------------------------------------------ the model

def _distort(a, b, k, jac: bool):
    """Normalised (a, b) (arrays) -> (x', y', tt = theta / r, t2 = theta^2) and with ``jac`` also (dx'/da, dx'/db = dy'/da,
    dy'/db).  dx'/dk_j = a tt theta^(2j)."""
    r2 = a * a + b * b
    r = np.sqrt(r2)
    th = np.arctan(r)
    small = r < SMALL_R
    with np.errstate(all="ignore"):
        tt = np.where(small, 1.0 + r2 * (-1.0 / 3.0 + r2 * (1.0 / 5.0)), th / r)
    t2 = th * th
    s = tt * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    xd, yd = s * a, s * b
    if not jac:
        return xd, yd, tt, t2
    dthd = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
    # w = (ds/dr) / r; s = 1 + (k1 - 1/3) r^2 + (1/5 - k1 + k2) r^4 + ...
    with np.errstate(all="ignore"):
        w = np.where(small, 2.0 * (k[0] - 1.0 / 3.0) + 4.0 * (1.0 / 5.0 - k[0] + k[1]) * r2, (dthd / (1.0 + r2) - s) / r2)
    return xd, yd, tt, t2, s + a * a * w, a * b * w, s + b * b * w


def _undistort(img: np.ndarray, K: np.ndarray, k: np.ndarray) -> np.ndarray:
    """Pixels (N, 2) -> the pinhole-normalised points (tan(theta) along the pixel's direction); NaN rows for pixels outside."""
    xp = (img[:, 0] - K[0, 2]) / K[0, 0]
    yp = (img[:, 1] - K[1, 2]) / K[1, 1]
    thd = np.sqrt(xp * xp + yp * yp)
    th = thd.copy()
    done = np.zeros(th.shape[0], bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_MAX_ITER):
            t2 = th * th
            f = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - thd
            df = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
            s = f / df
            live = ~done
            th = np.where(live, th - s, th)
            done |= live & (np.abs(s) < NEWTON_EPS)
            if done.all():
                break
        inside = done & (th >= 0.0) & (th < math.pi / 2)
        sc = np.where(thd < SMALL_THETA_D, 1.0, np.tan(th) / thd)
    out = np.stack([xp * sc, yp * sc], 1)
    out[~inside] = np.nan
    return out


def undistort_points_host(pix, camera_matrix, dist_coeffs) -> np.ndarray:
    """Pixels (N, 2) -> normalised undistorted coordinates (N, 2) (``cv2.fisheye.undistortPoints`` without R and P): the
    point tan(theta) from the axis along the pixel's direction.  NaN rows for pixels outside the model."""
    return _undistort(np.asarray(pix, np.float64).reshape(-1, 2), _camera(camera_matrix), _dist4(dist_coeffs))


def _project(obj: np.ndarray, img: np.ndarray, p: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool, intr: bool = False):
    """``pnp._project`` through this model: residuals (projected - observed, px) at pose p, their cost, and with ``jac`` the
    2N x 6 Jacobian (with ``intr`` 2N x 14: the 8 intrinsic columns first).  cost = inf when a point is not in front of the camera."""
    res, cost, J, m = pnp._project_through(_distort, obj, img, p, K, k, jac)
    if J is None or not intr:
        return res, cost, J
    a, b, xd, yd, tt, t2 = m[:6]
    fx, fy = K[0, 0], K[1, 1]
    n = obj.shape[0]
    Ji = np.zeros((n, 2, N_INTR))
    Ji[:, 0, 0] = xd
    Ji[:, 1, 1] = yd
    Ji[:, 0, 2] = 1.0
    Ji[:, 1, 3] = 1.0
    pw = tt
    for j in range(4):
        pw = pw * t2
        Ji[:, 0, 4 + j], Ji[:, 1, 4 + j] = fx * (a * pw), fy * (b * pw)
    return res, cost, np.concatenate([Ji.reshape(2 * n, N_INTR), J], 1)


def _project_q(Q: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool):
    """``stereo._project_q`` through this model: points Q (n, 3) in the camera's frame -> residuals (projected - observed, px)
    and, with ``jac``, d(u, v)/dQ (n, 2, 3): ``_project``'s model and derivatives with the pose taken out, which is what a camera
    behind a rig transform needs.  Every Z must be positive (the caller checks)."""
    return pnp._project_q_through(_distort, Q, img, K, k, jac)


def project_points_host(object_points_, rvec, tvec, camera_matrix, dist_coeffs, jacobian: bool = False):
    """``cv2.fisheye.projectPoints``: object points (N, 3) at the pose (rvec, tvec) -> pixels (N, 2); NaN rows for points that
    are not in front of the camera.  With ``jacobian`` (every point must be in front): ``(pixels, J)`` with J (2N, 14) =
    d(u, v)/d(fx, fy, cx, cy, k1, k2, k3, k4, rvec, tvec)."""
    K, k = _camera(camera_matrix), _dist4(dist_coeffs)
    obj = np.asarray(object_points_, np.float64).reshape(-1, 3)
    p = np.r_[np.asarray(rvec, np.float64).ravel(), np.asarray(tvec, np.float64).ravel()]
    X = obj @ _rodrigues(p[:3]).T + p[3:]
    front = X[:, 2] > 0
    out = np.full((obj.shape[0], 2), np.nan)
    if jacobian:
        if not front.all():
            raise ValueError("a point is not in front of the camera")
        res, _, J = _project(obj, np.zeros((obj.shape[0], 2)), p, K, k, True, True)
        return res, J
    if front.any():
        out[front] = _project(obj[front], np.zeros((int(front.sum()), 2)), p, K, k, False)[0]
    return out


# ------------------------------------------------------------------------------------------------ pose

def _solve(obj: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray) -> Tuple[int, np.ndarray]:
    """``pnp._solve`` through this model: obj (N, 3) board points, img (N, 2) pixels -> (status, pose[8])."""
    return pnp._solve_through(_undistort, _project, obj, img, K, k)


def solve_pnp_fisheye_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs):
    """``pnp.solve_pnp_host_full`` on a fisheye camera: (status, pose[8] = rvec, tvec, rms px, accepted LM steps)."""
    K, k = _camera(camera_matrix), _dist4(dist_coeffs)
    kp = np.asarray(keypoints)
    if kp.ndim != 2 or kp.shape[0] < 4:
        return PNP_TOO_FEW, np.zeros(POSE_WORDS)
    obj = object_points(kp[:, 2], col_count, row_count, square_len)
    return _solve(obj, kp[:, :2].astype(np.float32), K, k)


def solve_pnp_fisheye_host(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs):
    """``pnp.solve_pnp_host`` on a fisheye camera -> (ret, rvec (3,1), tvec (3,1)); (False, None, None) for fewer than 4 points,
    a pixel outside the model or input the solver refuses."""
    return _as_cv2(*solve_pnp_fisheye_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs))


def solve_pnp_fisheye_ransac_host_full(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                                       reproj_error=8.0, min_inliers=4, seed=0, with_margin=False, pool_order=False):
    """``pnp.solve_pnp_ransac_host_full`` on a fisheye camera, and the definition of ``dcx_fisheye_solve_pnp_ransac_pool`` ->
    (status, pose[8], inliers bool[N] in the caller's row order, winning hypothesis or -1[, margin]).  The sampler, the four-point
    pose, the scoring and the selection are ``pnp._ransac_host_full``'s, run through this model: the sample's pixels through
    ``_undistort`` (a sample with a pixel outside the model has no hypothesis), the rows scored by ``_project``, the winner's
    inliers solved by ``_solve`` (DEGENERATE if one of them lies outside the model)."""
    return pnp._ransac_host_full(keypoints, col_count, row_count, square_len, _camera(camera_matrix), _dist4(dist_coeffs),
                                 (_undistort, _project, _solve), iterations, reproj_error, min_inliers, seed, with_margin, pool_order)


def solve_pnp_fisheye_ransac_host(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                                  reproj_error=8.0, min_inliers=4, seed=0):
    """``pnp.solve_pnp_ransac_host`` on a fisheye camera -> (ret, rvec (3,1), tvec (3,1), inliers bool[N])."""
    return pnp._as_cv2_ransac(*solve_pnp_fisheye_ransac_host_full(keypoints, col_count, row_count, square_len, camera_matrix,
                                                                  dist_coeffs, iterations, reproj_error, min_inliers, seed)[:3])


# ------------------------------------------------------------------------------------------------ calibration

def _camera_of(theta: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    return _camera_matrix(theta), np.array(theta[4:8], np.float64)


def _project_full(obj, img, theta, p, jac: bool):
    K, k = _camera_of(theta)
    return _project(obj, img, p, K, k, jac, True)


def _theta0(w: int, h: int, focal0) -> np.ndarray:
    f = float(focal0) if focal0 is not None and float(focal0) > 0 else max(w, h) / 2.0
    if not math.isfinite(f):
        raise ValueError("focal0 must be finite")
    return np.array([f, f, (w - 1) * 0.5, (h - 1) * 0.5, 0, 0, 0, 0], np.float64)


def calibrate_fisheye_host_full(object_points_, image_points, image_size, focal0=None) -> CalibResult:
    """``cv2.fisheye.calibrate``'s role for a planar (z = 0) target, in float64 on the host (module docstring), with every output
    of ``dcx_fisheye_calibrate_pool``: ``calib.CalibResult`` with ``dist_coeffs`` 1x4 = k1 k2 k3 k4.  A view with fewer than 4
    points (TOO_FEW) or whose pose solve at the start camera fails (DEGENERATE: also a pixel beyond theta = pi/2 there) is left
    out and reported in ``view_status``."""
    w, h = _image_size(image_size)
    views = _views(object_points_, image_points)
    counts = np.array([obj.shape[0] for obj, _ in views], np.int64)
    theta = _theta0(w, h, focal0)
    K0, k0 = _camera_of(theta)
    view_status = np.full(len(views), PNP_OK, np.int32)
    poses0 = np.zeros((len(views), 6))
    for i, (obj, img) in enumerate(views):
        if obj.shape[0] < 4:
            view_status[i] = PNP_TOO_FEW
            continue
        view_status[i], pose = _solve(obj, img, K0, k0)
        poses0[i] = pose[:6]
    used = np.flatnonzero(view_status == PNP_OK)
    if not used.size:
        return _result(CALIB_NO_VIEWS, theta, view_status, None, None, counts, 0, 0, N_DIST)
    st, theta, poses, vc, iters, attempts = _refine([views[i] for i in used], theta, poses0[used], _project_full, CALIB_MAX_ITER)
    return _result(st, theta, view_status, poses, vc, counts, iters, attempts, N_DIST)


def calibrate_fisheye_host(object_points_, image_points, image_size, focal0=None):
    """cv2's 5-tuple ``(rms, K 3x3, D 1x4, rvecs, tvecs)``.  ValueError, as cv2 errors out, on a view that cannot be used or a
    failed calibration."""
    return _cv2_tuple(calibrate_fisheye_host_full(object_points_, image_points, image_size, focal0))


# ------------------------------------------------------------------------------------------------ map and points

def undistort_rectify_map_fisheye_host(camera_matrix, dist_coeffs, R, P, width: int, height: int, quantised: bool = True) -> np.ndarray:
    """``rectify.undistort_rectify_map_host`` with the ray through this model (``cv2.fisheye.initUndistortRectifyMap``) -> int32
    [height, width, 2] (x, y in 1/32 px, MAP_SENTINEL outside: q_z <= 0, a non-finite position or one beyond +-2^15 px); with
    ``quantised=False`` float64 source pixels, NaN outside."""
    return _rectify_map(_distort, _camera(camera_matrix), _dist4(dist_coeffs), R, P, width, height, quantised)


def rectify_points_fisheye_host(pix, camera_matrix, dist_coeffs, R=None, P=None) -> np.ndarray:
    """``rectify.rectify_points_host`` through this model (``cv2.fisheye.undistortPoints`` with R and P): pixels (N, 2) ->
    rectified pixels (N, 2), NaN rows for pixels outside the model or with a rotated z <= 0."""
    return _rectify_points(undistort_points_host, pix, camera_matrix, dist_coeffs, R, P)


def stereo_rectify_fisheye_host(camera0, dist0, camera1, dist1, image_size, R, T, focal=None) -> Rectification:
    """``rectify.stereo_rectify_host`` for a pair of fisheye cameras (``cv2.fisheye.stereoRectify``'s role): the rig (R, T) with
    q1 = R q0 + T -> ``rectify.Rectification``.  R1, R2, axis and Tn are ``stereo_rectify_host``'s (no camera enters them).  The
    rectified cameras are pinholes with f = ``focal`` or, by default, min(fy0, fy1), and the principal point ((W - 1) / 2,
    (H - 1) / 2): a wide lens's image corners need not undistort, so the corner-balancing principal point of the pinhole call is
    not available, and neither is ``alpha``.  P1, P2 and Q take ``stereo_rectify_host``'s forms, so
    ``undistort_rectify_map_fisheye_device``, ``rectify.remap_device``, ``rectify_points_fisheye_pool``,
    ``rectify.reproject_to_3d`` and the matcher follow unchanged.  With a small f more of the field fits the rectified frame.
    ValueError for refused cameras, a zero T or a focal length that is not positive and finite."""
    K0, K1 = _camera(camera0), _camera(camera1)
    _dist4(dist0), _dist4(dist1)
    W, H = int(image_size[0]), int(image_size[1])
    if W < 2 or H < 2:
        raise ValueError("image_size must be (W, H) with both >= 2")
    R1, R2, axis, Tn = _rectifying_rotations(R, T)
    f = min(K0[1, 1], K1[1, 1]) if focal is None else float(focal)
    if not (math.isfinite(f) and f > 0):
        raise ValueError("the rectified focal length must be positive and finite")
    P1, P2, Q = _projections(f, (W - 1) / 2, (H - 1) / 2, axis, Tn)
    return Rectification(R1, R2, P1, P2, Q, axis, Tn)


# ------------------------------------------------------------------------------------------------ the device entry points

def solve_pnp_fisheye_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, camera_matrix,
                           dist_coeffs, out=None):
    """``pnp.solve_pnp_pool`` on a fisheye camera (``dcx_fisheye_solve_pnp_pool``): one launch on the current stream, no host sync,
    nothing allocated when ``out`` is given (capture-safe).  Returns device tensors ``(status int32 [B], pose float64 [B, 8])``."""
    return pnp._solve_pool(_camera_args, "dcx_fisheye_solve_pnp_pool", packed, batch, pool, refined, col_count, row_count, square_len,
                           camera_matrix, dist_coeffs, out)


def solve_pnp_fisheye_batch_device(keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs, device="cuda"):
    """``solve_pnp_fisheye_host`` of every frame of a list of keypoint arrays in one launch -> list of ``(ret, rvec, tvec)``.
    IndexError if any frame with >= 4 points carries an id outside the board."""
    return pnp._solve_batch_device(_camera_args, solve_pnp_fisheye_pool, keypoints_list, col_count, row_count, square_len,
                                   camera_matrix, dist_coeffs, device)


def solve_pnp_fisheye_device(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, device="cuda"):
    """``solve_pnp_fisheye_host`` on the GPU -> ``(ret, rvec, tvec)``."""
    return pnp._solve_device(_camera_args, solve_pnp_fisheye_batch_device, keypoints, col_count, row_count, square_len,
                             camera_matrix, dist_coeffs, device)


def solve_pnp_fisheye_ransac_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, camera_matrix,
                                  dist_coeffs, iterations=100, reproj_error=8.0, min_inliers=4, seed=0, out=None, workspace=None):
    """``pnp.solve_pnp_ransac_pool`` on a fisheye camera (``dcx_fisheye_solve_pnp_ransac_pool``): the same two launches, outputs
    ``(status, pose, info, inliers)``, ``out`` / ``workspace`` conventions (``pnp.ransac_workspace_bytes``) and capture safety."""
    return pnp._ransac_pool(_camera_args, "dcx_fisheye_solve_pnp_ransac_pool", packed, batch, pool, refined, col_count, row_count,
                            square_len, camera_matrix, dist_coeffs, iterations, reproj_error, min_inliers, seed, out, workspace)


def solve_pnp_fisheye_ransac_batch_device(keypoints_list, col_count, row_count, square_len, camera_matrix, dist_coeffs,
                                          iterations=100, reproj_error=8.0, min_inliers=4, seed=0, device="cuda", full=False):
    """``pnp.solve_pnp_ransac_batch_device`` on a fisheye camera -> list of ``(ret, rvec, tvec, inliers)`` (``full=True``: of
    ``(status, pose[8], inliers, winner)``), the masks in the caller's row order."""
    return pnp._ransac_batch_device(_camera_args, solve_pnp_fisheye_ransac_pool, keypoints_list, col_count, row_count, square_len,
                                    camera_matrix, dist_coeffs, iterations, reproj_error, min_inliers, seed, device, full)


def solve_pnp_fisheye_ransac_device(keypoints, col_count, row_count, square_len, camera_matrix, dist_coeffs, iterations=100,
                                    reproj_error=8.0, min_inliers=4, seed=0, device="cuda"):
    """``pnp.solve_pnp_ransac_device`` on a fisheye camera -> ``(ret, rvec, tvec, inliers bool[N])``."""
    return pnp._ransac_device(_camera_args, solve_pnp_fisheye_ransac_batch_device, keypoints, col_count, row_count, square_len,
                              camera_matrix, dist_coeffs, iterations, reproj_error, min_inliers, seed, device)


def workspace_bytes(batch: int) -> int:
    """Bytes of device workspace ``calibrate_fisheye_pool`` needs."""
    from . import _lib
    return int(_lib.lib().dcx_fisheye_calibrate_workspace_bytes(int(batch)))


_calib_fields = functools.partial(_common_fields, n_dist=N_DIST)     # ``dcx_fisheye_calibrate_pool``'s 16 doubles -> ``CalibResult``'s fields


def calibrate_fisheye_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, image_size,
                           focal0=None, workspace=None) -> CalibResult:
    """``calibrate_fisheye_host_full`` from every frame of a corner pool, read in place (``calib.calibrate_charuco_pool``'s
    conventions).  ``workspace``: a contiguous device tensor of at least ``workspace_bytes(batch)`` bytes (else one is made).
    Like ``calibrate_charuco_pool`` the call synchronises the current stream and cannot be captured in a graph."""
    import torch
    from . import _lib
    w, h = _image_size(image_size)
    f0 = 0.0 if focal0 is None else float(focal0)             # not > 0: the entry takes max(w, h) / 2
    _theta0(w, h, focal0)                                     # ValueError for an infinite one
    dev = packed.device
    ptrs = _pool_ptrs(packed, batch, pool, refined)
    st, pose = _view_outputs(batch, dev)
    nbytes = workspace_bytes(batch)
    ws = _dev.workspace(workspace, dev, nbytes, f"workspace must be a contiguous tensor of at least {nbytes} bytes on {dev}")
    res = (_ctypes.c_double * RESULT_WORDS)()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_fisheye_calibrate_pool(*ptrs, int(batch), int(pool), int(col_count), int(row_count),
                                                         float(square_len), w, h, f0, ws.data_ptr(),
                                                         ws.numel() * ws.element_size(), st.data_ptr(), pose.data_ptr(), res,
                                                         _lib.current_stream()), "dcx_fisheye_calibrate_pool")
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
    return CalibResult(*_calib_fields(res, st_h, pose_h))


def calibrate_fisheye_device(keypoints_list: Sequence, col_count, row_count, square_len, image_size, focal0=None,
                             device="cuda") -> CalibResult:
    """Calibrate a fisheye camera from ``infer_image``-format keypoint arrays ([x, y, id] rows) on the GPU -> ``CalibResult``.
    IndexError if a frame with >= 4 points carries an id outside the board."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    _image_size(image_size)
    packed, b, pool = _upload(keypoints_list, dev)
    with torch.cuda.device(dev):
        r = calibrate_fisheye_pool(packed, b, pool, True, col_count, row_count, square_len, image_size, focal0)
    return _no_bad_id(r, col_count, row_count)


# ------------------------------------------------------------------------------------------------ how well the model is determined

def calibration_uncertainty_fisheye_host(object_points_, image_points, camera_matrix, dist_coeffs=None, rvecs=None, tvecs=None,
                                         view_status=None, inliers=None) -> CalibUncertainty:
    """``calib.calibration_uncertainty_host`` for the fisheye model: theta = (fx, fy, cx, cy, k1, k2, k3, k4), exactly 4
    coefficients (ValueError otherwise), dof = 2 points - 8 - 6 views; everything else (arguments, the ``CalibResult`` in
    ``camera_matrix``'s place, statuses, the dof convention) as said there."""
    return _uncertainty_host(object_points_, image_points, camera_matrix, dist_coeffs, rvecs, tvecs, view_status, inliers, N_DIST,
                             _project_full)


def calibration_uncertainty_fisheye_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len,
                                         result_or_model, inliers=None, workspace=None, out=None):
    """``calib.calibration_uncertainty_pool`` for the fisheye model -> the same two device tensors;
    ``calib.unpack_uncertainty(global_, pose_cov, N_INTR)`` unpacks them."""
    return _uncertainty_pool(CAMERA_FISHEYE, N_DIST, packed, batch, pool, refined, col_count, row_count, square_len, result_or_model,
                             inliers, workspace, out)


def calibration_uncertainty_fisheye_device(keypoints_list: Sequence, col_count, row_count, square_len, result_or_model, inliers=None,
                                           device="cuda") -> CalibUncertainty:
    """``calib.calibration_uncertainty_device`` for the fisheye model."""
    return _uncertainty_device(CAMERA_FISHEYE, N_DIST, keypoints_list, col_count, row_count, square_len, result_or_model, inliers,
                               device)


def undistort_rectify_map_fisheye_device(camera_matrix, dist_coeffs, R, P, width: int, height: int, device="cuda", out=None):
    """``undistort_rectify_map_fisheye_host`` on the GPU -> int32 device tensor [height, width, 2] (``out``: that tensor,
    preallocated and contiguous); ``rectify.remap_device`` warps through it.  Enqueued on the current stream; nothing is allocated
    when ``out`` is given.  Equal to the host map except where 32 m is within rounding of a half-integer, and there by 1."""
    return _map_device(_camera_args, "dcx_fisheye_undistort_rectify_map", camera_matrix, dist_coeffs, R, P, width, height, device, out)


def rectify_points_fisheye_pool(packed, batch: int, pool: int, refined: bool, camera_matrix, dist_coeffs, R=None, P=None, out=None):
    """``rectify.rectify_points_pool`` through this model: every slot of a corner pool in rectified coordinates -> float64 device
    tensor [pool, 2] by slot; NaN where ``rectify_points_fisheye_host`` gives NaN.  Capture-safe when ``out`` is given."""
    return _points_pool(_camera_args, "dcx_fisheye_rectify_points_pool", packed, batch, pool, refined, camera_matrix, dist_coeffs, R, P,
                        out)
