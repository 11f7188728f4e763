"""Camera calibration without OpenCV: ``cv2.calibrateCamera`` (default flags, or the ``CALIB_*`` flags below and the rational
model) from ChArUco corners, on the host and on the GPU.

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

``flags`` (cv2's numeric values, ``CALIB_USE_INTRINSIC_GUESS`` ... ``CALIB_RATIONAL_MODEL``; any other bit is a ValueError) with the
optional guess ``camera_matrix`` / ``dist_coeffs`` select what is solved for.  The parameter vector is then always theta12 = (fx, fy,
cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) with a mask of free entries (``_flag_model``):
- start: without ``USE_INTRINSIC_GUESS`` steps 2 and 3 above; with ``FIX_ASPECT_RATIO`` OpenCV's rule is applied to K0 before step 3
  (a = camera_matrix[0, 0] / camera_matrix[1, 1], tf = (fx + fy) / (a + 1), fx = a tf, fy = tf).  With the guess, theta is the given
  model (missing coefficients 0) and every view that passes step 1's checks gets its pose by ``pnp._solve`` through that model,
  distortion included;
- ``FIX_PRINCIPAL_POINT`` fixes cx cy, ``FIX_FOCAL_LENGTH`` fx fy, ``ZERO_TANGENT_DIST`` sets p1 = p2 = 0 and fixes them, ``FIX_Ki`` fixes
  ki at its start value; without ``RATIONAL_MODEL`` k4 k5 k6 stay at their start values (0 unless an 8-coefficient guess was given).  A
  fixed parameter has a zero Jacobian column, a 1 on its diagonal of V and a zero gradient entry, hence a zero step: it comes back
  with the bits it started with;
- ``FIX_ASPECT_RATIO``: fx = a fy.  The fy column is d/dfy + a d/dfx, fx is not a free parameter, and every trial step writes
  fx = a * fy, one multiplication (``_lm.refine``'s ``constrain``; the device's reduce_solve does the same);
- the stop rule, the caps and the damping are step 4's, |dp| / |p| over all 12 + 6N entries.
``flags = 0`` is the call without the keyword: the same code path and bits.  Rational models are compared by where they project,
never coefficient by coefficient (numerator and denominator trade against each other).  The flags are not offered by the robust
calibration (its step C stays the default solve), the fisheye, stereo and rig solvers; thin-prism and tilted terms are refused.

``calibrate_camera_ransac_*`` / ``calibrate_charuco_ransac_*`` put a consensus search in front of that solve and a re-check behind
it: a corner with a wrong id sits a board square away from its label, the joint least squares has no defence, and every pose
computed later inherits the wrong model.  ``calibrate_camera_ransac_host_full`` is the definition and carries the steps;
``calibrate_charuco_ransac_pool`` / ``_device`` run them in csrc/dcx_calib_ransac.hip.  The discrete results (winners, masks,
number of solves) are equal on host and device wherever no row stands within rounding of a threshold.

``calibration_uncertainty_*`` say how well a solved model is determined: the covariances of the intrinsics and of every used view's
pose (cv2.calibrateCameraExtended's standard deviations).  ``calibration_uncertainty_host`` is the definition;
``calibration_uncertainty_pool`` / ``_device`` run it in csrc/dcx_calib_cov.hip, without a host loop or a synchronisation.
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _dev, _lm, pnp
from .corner_pool import _caller_order, _pool_rows, layout, pack_keypoints, views
from .pnp import PNP_BAD_ID, PNP_DEGENERATE, PNP_NO_CONSENSUS, PNP_NONFINITE, PNP_OK, PNP_TOO_FEW, _bad_id_error, _homography, _solve

# overall status (include/deepcharuco_amd.h); per-view statuses are pnp's PNP_*
CALIB_OK, CALIB_NO_VIEWS, CALIB_DEGENERATE, CALIB_NONFINITE = _lm.LM_OK, _lm.LM_NO_UNITS, _lm.LM_DEGENERATE, _lm.LM_NONFINITE
CALIB_MAX_ITER = 30
CALIB_EPS = float(np.finfo(np.float64).eps)
N_INTR = 9                     # fx, fy, cx, cy, k1, k2, p1, p2, k3
RESULT_WORDS = 16              # h_result of dcx_calibrate_pool
N_FULL = 12                    # theta12: N_INTR, then k4, k5, k6
FLAGS_RESULT_WORDS = 20        # h_result of dcx_calibrate_flags_pool

# cv2's values.  Any other bit (thin prism, tilted, FIX_S*, FIX_TANGENT_DIST, USE_LU / USE_QR) is refused
CALIB_USE_INTRINSIC_GUESS, CALIB_FIX_ASPECT_RATIO, CALIB_FIX_PRINCIPAL_POINT, CALIB_ZERO_TANGENT_DIST = 1, 2, 4, 8
CALIB_FIX_FOCAL_LENGTH, CALIB_FIX_K1, CALIB_FIX_K2, CALIB_FIX_K3 = 16, 32, 64, 128
CALIB_FIX_K4, CALIB_FIX_K5, CALIB_FIX_K6, CALIB_RATIONAL_MODEL = 0x800, 0x1000, 0x2000, 0x4000
CALIB_FLAGS_KNOWN = 0x1 | 0x2 | 0x4 | 0x8 | 0x10 | 0x20 | 0x40 | 0x80 | 0x800 | 0x1000 | 0x2000 | 0x4000
_FIX_K = ((CALIB_FIX_K1, 4), (CALIB_FIX_K2, 5), (CALIB_FIX_K3, 8), (CALIB_FIX_K4, 9), (CALIB_FIX_K5, 10), (CALIB_FIX_K6, 11))

RANSAC_MAX_ROUNDS = 8          # re-mask rounds of the robust calibration

__all__ = ["CalibResult", "calibrate_camera_host", "calibrate_camera_host_full", "calibrate_charuco_pool",
           "calibrate_charuco_device", "CALIB_OK", "CALIB_NO_VIEWS", "CALIB_DEGENERATE", "CALIB_NONFINITE",
           "CALIB_USE_INTRINSIC_GUESS", "CALIB_FIX_ASPECT_RATIO", "CALIB_FIX_PRINCIPAL_POINT", "CALIB_ZERO_TANGENT_DIST",
           "CALIB_FIX_FOCAL_LENGTH", "CALIB_FIX_K1", "CALIB_FIX_K2", "CALIB_FIX_K3", "CALIB_FIX_K4", "CALIB_FIX_K5", "CALIB_FIX_K6",
           "CALIB_RATIONAL_MODEL", "flags_workspace_bytes",
           "RobustCalibResult", "calibrate_camera_ransac_host", "calibrate_camera_ransac_host_full",
           "calibrate_charuco_ransac_pool", "calibrate_charuco_ransac_device", "ransac_workspace_bytes",
           "CalibUncertainty", "calibration_uncertainty_host", "calibration_uncertainty_pool", "calibration_uncertainty_device",
           "unpack_uncertainty", "uncertainty_workspace_bytes", "COV_OK", "COV_NO_VIEWS", "COV_NO_DOF", "COV_SINGULAR"]


class _CalibFields(NamedTuple):
    status: int                  # CALIB_*
    rms: float                   # sqrt(sum |r|^2 / points used): cv2.calibrateCamera's return value
    camera_matrix: np.ndarray    # 3x3
    dist_coeffs: np.ndarray      # 1x5: k1 k2 p1 p2 k3; 1x8 (k4 k5 k6) with CALIB_RATIONAL_MODEL or an 8-coefficient guess
    view_status: np.ndarray      # int32 [B], pnp.PNP_*
    rvecs: np.ndarray            # [B, 3]; zeros unless the view was used
    tvecs: np.ndarray            # [B, 3]
    view_rms: np.ndarray         # [B] rms reprojection error of the view at the solution (px)
    view_points: np.ndarray      # int64 [B]
    iterations: int              # accepted LM steps
    attempts: int                # LM trial steps (accepted + rejected)
    views_used: int
    points_used: int


class CalibResult(_CalibFields):
    """The 13 fields above, which ``RobustCalibResult`` begins with in the same order, and beside them the attribute ``flags``: the
    CALIB_* flags the model was solved with (0: the default model).  ``flags`` is a keyword of the constructor and of ``_replace``
    and no member of the tuple, whose length and layout other code relies on."""
    flags = 0

    def __new__(cls, *args, flags: int = 0, **kw):
        self = super().__new__(cls, *args, **kw)
        self.flags = int(flags)
        return self

    def _replace(self, **kw):
        flags = kw.pop("flags", self.flags)
        r = super()._replace(**kw)
        r.flags = int(flags)
        return r


# ------------------------------------------------------------------------------------------------ the fp64 steps

def _camera_matrix(theta: np.ndarray) -> np.ndarray:
    """theta = (fx, fy, cx, cy, ...) -> K 3x3."""
    return np.array([[theta[0], 0.0, theta[2]], [0.0, theta[1], theta[3]], [0.0, 0.0, 1.0]])


def _camera_of(theta: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """theta (9) -> (K 3x3, pnp's 8 distortion coefficients k1 k2 p1 p2 k3 0 0 0)."""
    k = np.zeros(8)
    k[:5] = theta[4:9]
    return _camera_matrix(theta), k


def _project_full(obj: np.ndarray, img: np.ndarray, theta: np.ndarray, p: np.ndarray, jac: bool):
    """Residuals (projected - observed, px), cost and with ``jac`` the 2N x 15 Jacobian [d/dtheta (9) | d/d(rvec, tvec) (6)].
    The residuals and the pose columns are ``pnp._project``'s; cost = inf when a point is not in front of the camera."""
    K, k = _camera_of(theta)
    res, cost, Je, m = pnp._project_through(pnp._distort, obj, img, p, K, k, jac)
    if Je is None:
        return res, cost, None
    x, y, xd, yd, r2 = m[:5]
    r4, r6 = r2 * r2, r2 * r2 * r2
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


def _initialise(views, image_size, adjust=None):
    """-> (view status [B], theta0 (9) or None, initial poses [B, 6]).  Statuses as the module docstring; theta0 None when no
    view is left (status NO_VIEWS) or the init's 2x2 system is singular.  ``adjust(theta0)`` -> the theta0 the poses are solved
    with and the solve starts from (FIX_ASPECT_RATIO's rule); None: Zhang's as it is."""
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
    if adjust is not None:
        theta = adjust(theta)
    K0, k0 = _camera_of(theta)
    for i, (obj, img) in enumerate(views):
        if status[i] == PNP_OK:
            st, pose = _solve(obj, img, K0, k0)
            status[i] = st
            poses[i] = pose[:6]
    return status, theta, poses


def _normal_blocks(views, theta: np.ndarray, poses: np.ndarray, project_full=_project_full):
    """The blocks of JtJ and Jtr over the used views, for a camera model given by its ``project_full`` (this module's, or
    ``fisheye._project_full``) with n = theta.size intrinsics: U [N, 6, 6] (pose-pose), W [N, n, 6] (intrinsics-pose), V [n, n]
    (intrinsics-intrinsics, summed), ga [n], gb [N, 6], the per-view costs [N].  None if a point is behind the camera."""
    N, n = len(views), theta.size
    U, W, gb, costs = np.zeros((N, 6, 6)), np.zeros((N, n, 6)), np.zeros((N, 6)), np.zeros(N)
    V, ga = np.zeros((n, n)), np.zeros(n)
    for i, (obj, img) in enumerate(views):
        res, cost, J = project_full(obj, img, theta, poses[i], True)
        if res is None:
            return None
        r = res.ravel()
        A, Bm = J[:, :n], J[:, n:]
        U[i], W[i], gb[i], costs[i] = Bm.T @ Bm, A.T @ Bm, Bm.T @ r, cost
        V += A.T @ A
        ga += A.T @ r
    return U, W, V, ga, gb, costs


_schur_step = _lm.schur_step     # one copy, generic in the global block's size


def _view_costs(views, theta, poses, project_full=_project_full) -> np.ndarray:
    return np.array([project_full(obj, img, theta, poses[i], False)[1] for i, (obj, img) in enumerate(views)])


def _total(costs: np.ndarray) -> float:
    c = 0.0
    for v in costs.tolist():
        c += v
    return c


def _refine(views, theta: np.ndarray, poses: np.ndarray, project_full=_project_full, max_iter=CALIB_MAX_ITER):
    """Joint LM (module docstring, step 4) -> (status, theta, poses, per-view costs, accepted steps, attempts)."""
    return _lm.refine(theta, poses, lambda t, p: _normal_blocks(views, t, p, project_full),
                      lambda t, p: _view_costs(views, t, p, project_full), _total, False, max_iter, CALIB_EPS)


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


def _result(status, theta, view_status, poses, vc, counts, iters, attempts, n_dist=5) -> CalibResult:
    """``n_dist``: the model's distortion coefficients, theta[4:4 + n_dist] (5 here, the fisheye model's 4)."""
    B = len(view_status)
    used = np.flatnonzero(view_status == PNP_OK)
    K, dist = np.zeros((3, 3)), np.zeros((1, n_dist))
    rv, tv, vr = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B)
    rms = 0.0
    if status == CALIB_OK:
        K = _camera_matrix(theta)
        dist = theta[4:4 + n_dist].reshape(1, n_dist).copy()
        rv[used], tv[used] = poses[:, :3], poses[:, 3:]
        vr[used] = np.sqrt(vc / counts[used])
        rms = math.sqrt(_total(vc) / int(counts[used].sum()))
    return CalibResult(int(status), float(rms), K, dist, view_status.astype(np.int32), rv, tv, vr, counts.astype(np.int64),
                       int(iters), int(attempts), int(used.size), int(counts[used].sum()))


# ------------------------------------------------------------------------------------------------ the flags

class _FlagModel(NamedTuple):
    flags: int
    free: np.ndarray             # bool [12]: the entries of theta12 the solve moves (fx is not free under the aspect tie)
    aspect: Optional[float]      # a of fx = a fy while fy is free, else None
    ratio: Optional[float]       # a of FIX_ASPECT_RATIO's rule on Zhang's K0 (the start without a guess), else None
    guess: Optional[np.ndarray]  # theta12 of USE_INTRINSIC_GUESS, else None
    n_dist: int                  # coefficients reported: 8 with RATIONAL_MODEL or an 8-coefficient guess, else 5
    rational: bool               # k4 k5 k6 are live: the device runs its 12-parameter model


def _flag_model(flags, camera_matrix, dist_coeffs) -> Optional[_FlagModel]:
    """The checked arguments of a flagged call (module docstring), or None for ``flags == 0``: today's call, in which a
    ``camera_matrix`` has no role.  ValueError for an unknown bit, a missing or unusable ``camera_matrix``, a number of coefficients
    other than 0, 4, 5 or 8, values that are not finite, or ``dist_coeffs`` without ``CALIB_USE_INTRINSIC_GUESS``."""
    if int(flags) != flags:
        raise ValueError(f"flags must be an integer, not {flags!r}")
    flags = int(flags)
    if flags & ~CALIB_FLAGS_KNOWN:
        raise ValueError(f"flags {flags:#x}: the bits {flags & ~CALIB_FLAGS_KNOWN:#x} are not supported (known: {CALIB_FLAGS_KNOWN:#x})")
    use_guess = bool(flags & CALIB_USE_INTRINSIC_GUESS)
    if dist_coeffs is not None and not use_guess:
        raise ValueError("dist_coeffs is part of the guess: it needs CALIB_USE_INTRINSIC_GUESS")
    if flags == 0:
        return None
    K = None if camera_matrix is None else pnp._camera(camera_matrix)
    if K is None and flags & (CALIB_USE_INTRINSIC_GUESS | CALIB_FIX_ASPECT_RATIO):
        raise ValueError("CALIB_USE_INTRINSIC_GUESS and CALIB_FIX_ASPECT_RATIO need a camera_matrix")
    d = np.zeros(0) if dist_coeffs is None else np.asarray(dist_coeffs, dtype=np.float64).ravel()
    k8 = pnp._dist(dist_coeffs)
    free = np.ones(N_FULL, bool)
    if not flags & CALIB_RATIONAL_MODEL:
        free[9:] = False
    if flags & CALIB_FIX_PRINCIPAL_POINT:
        free[2:4] = False
    if flags & CALIB_FIX_FOCAL_LENGTH:
        free[0:2] = False
    if flags & CALIB_ZERO_TANGENT_DIST:
        free[6:8] = False
    for bit, j in _FIX_K:
        if flags & bit:
            free[j] = False
    guess = None
    if use_guess:
        guess = np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], k8]
        if flags & CALIB_ZERO_TANGENT_DIST:
            guess[6:8] = 0.0
    ratio = float(K[0, 0] / K[1, 1]) if flags & CALIB_FIX_ASPECT_RATIO else None
    if ratio is not None and not (math.isfinite(ratio) and ratio > 0):
        raise ValueError(f"CALIB_FIX_ASPECT_RATIO: camera_matrix gives the ratio {ratio}, which must be finite and positive")
    aspect = ratio if free[1] else None
    if aspect is not None:
        free[0] = False
    rational = bool(flags & CALIB_RATIONAL_MODEL) or bool(guess is not None and guess[9:].any())
    return _FlagModel(flags, free, aspect, ratio if guess is None else None, guess,
                      8 if flags & CALIB_RATIONAL_MODEL or d.size == 8 else 5, rational)


def _camera_of12(theta: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """theta12 -> (K 3x3, pnp's 8 distortion coefficients)."""
    return _camera_matrix(theta), theta[4:12].copy()


def _project_full12(obj: np.ndarray, img: np.ndarray, theta: np.ndarray, p: np.ndarray, jac: bool):
    """``_project_full`` over theta12 with the denominator live: the 2N x 18 Jacobian [d/dtheta12 | d/d(rvec, tvec)].  The k1 k2 k3
    columns are ``_project_full``'s divided by den = 1 + k4 r^2 + k5 r^4 + k6 r^6, the k4 k5 k6 columns -f (x, y) r^2j num / den^2."""
    K, k = _camera_of12(theta)
    res, cost, Je, m = pnp._project_through(pnp._distort, obj, img, p, K, k, jac)
    if Je is None:
        return res, cost, None
    x, y, xd, yd, r2 = m[:5]
    r4, r6 = r2 * r2, r2 * r2 * r2
    num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]))
    iden = 1.0 / den
    gq = -(num * iden) * iden                     # d(num / den) / d den
    fx, fy = theta[0], theta[1]
    n = obj.shape[0]
    Ji = np.zeros((n, 2, N_FULL))
    Ji[:, 0, 0] = xd
    Ji[:, 1, 1] = yd
    Ji[:, 0, 2] = 1.0
    Ji[:, 1, 3] = 1.0
    for j, pw in ((4, r2), (5, r4), (8, r6)):                                       # k1 k2 k3
        Ji[:, 0, j], Ji[:, 1, j] = fx * (x * pw * iden), fy * (y * pw * iden)
    Ji[:, 0, 6], Ji[:, 1, 6] = fx * (2 * x * y), fy * (r2 + 2 * y * y)              # p1
    Ji[:, 0, 7], Ji[:, 1, 7] = fx * (r2 + 2 * x * x), fy * (2 * x * y)              # p2
    for j, pw in ((9, r2), (10, r4), (11, r6)):                                     # k4 k5 k6
        Ji[:, 0, j], Ji[:, 1, j] = fx * (x * pw * gq), fy * (y * pw * gq)
    return res, cost, np.concatenate([Ji.reshape(2 * n, N_FULL), Je], 1)


def _masked_project(free: np.ndarray, aspect: Optional[float], project_full=_project_full12):
    """``project_full`` with the flags' linear map on its intrinsic columns: a times the fx column added to the fy column under the
    aspect tie, then every column that is not free zeroed."""
    fixed = np.flatnonzero(~free)

    def project(obj, img, theta, p, jac):
        res, cost, J = project_full(obj, img, theta, p, jac)
        if J is not None:
            if aspect is not None:
                J[:, 1] += aspect * J[:, 0]
            J[:, fixed] = 0.0
        return res, cost, J
    return project


def _masked_blocks(views, theta, poses, free, aspect):
    """``_normal_blocks`` of the masked model; a fixed parameter gets a 1 on its diagonal of V (its row, column and gradient entry
    are zero), so the reduced system stays positive definite and its step is zero."""
    nb = _normal_blocks(views, theta, poses, _masked_project(free, aspect))
    if nb is not None:
        fixed = np.flatnonzero(~free)
        nb[2][fixed, fixed] = 1.0
    return nb


def _refine_flags(views, theta: np.ndarray, poses: np.ndarray, fm: _FlagModel, max_iter=CALIB_MAX_ITER):
    """``_refine`` over theta12 with ``fm``'s mask and aspect tie."""
    a = fm.aspect

    def constrain(g):
        g = g.copy()
        g[0] = a * g[1]
        return g
    return _lm.refine(theta, poses, lambda t, p: _masked_blocks(views, t, p, fm.free, a),
                      lambda t, p: _view_costs(views, t, p, _project_full12), _total, False, max_iter, CALIB_EPS,
                      constrain if a is not None else None)


def _aspect_rule(theta: np.ndarray, a: float) -> np.ndarray:
    """OpenCV's rule on Zhang's focal lengths: tf = (fx + fy) / (a + 1), fx = a tf, fy = tf."""
    theta = theta.copy()
    tf = (theta[0] + theta[1]) / (a + 1.0)
    theta[0], theta[1] = a * tf, tf
    return theta


def _initialise_flags(views, image_size, fm: _FlagModel):
    """``_initialise`` for a flagged call -> (view status [B], theta12 or None, initial poses [B, 6])."""
    if fm.guess is None:
        status, theta, poses = _initialise(views, image_size, None if fm.ratio is None else lambda t: _aspect_rule(t, fm.ratio))
        return status, None if theta is None else np.r_[theta, 0.0, 0.0, 0.0], poses
    B = len(views)
    status = np.full(B, PNP_OK, np.int32)
    poses = np.zeros((B, 6))
    K, k = _camera_of12(fm.guess)
    for i, (obj, img) in enumerate(views):
        if obj.shape[0] < 4:
            status[i] = PNP_TOO_FEW
            continue
        status[i] = _homography(obj, img)[0]          # the check of the default start, on the pixels as they are
        if status[i] == PNP_OK:
            st, pose = _solve(obj, img, K, k)
            status[i] = st
            if st == PNP_OK:
                poses[i] = pose[:6]
    return status, fm.guess.copy(), poses


def _calibrate_flags_host(object_points, image_points, image_size, fm: _FlagModel) -> CalibResult:
    w, h = _image_size(image_size)
    views = _views(object_points, image_points)
    counts = np.array([obj.shape[0] for obj, _ in views], np.int64)
    view_status, theta, poses0 = _initialise_flags(views, (w, h), fm)
    used = np.flatnonzero(view_status == PNP_OK)
    if theta is None or not used.size:
        st = CALIB_NO_VIEWS if not used.size else CALIB_DEGENERATE
        return _result(st, theta, view_status, None, None, counts, 0, 0, fm.n_dist)._replace(flags=fm.flags)
    st, theta, poses, vc, iters, attempts = _refine_flags([views[i] for i in used], theta, poses0[used], fm)
    return _result(st, theta, view_status, poses, vc, counts, iters, attempts, fm.n_dist)._replace(flags=fm.flags)


def calibrate_camera_host_full(object_points, image_points, image_size, flags: int = 0, camera_matrix=None,
                               dist_coeffs=None) -> CalibResult:
    """``cv2.calibrateCamera(object_points, image_points, image_size, camera_matrix, dist_coeffs, flags=flags)`` for a planar
    (z = 0) target, in float64 on the host, with every output of ``dcx_calibrate_pool`` / ``dcx_calibrate_flags_pool``
    (``CalibResult``).  ``flags``, ``camera_matrix``, ``dist_coeffs``: the module docstring; ``flags = 0`` is cv2's call with None,
    None.  Views that fail their checks are left out and reported in ``view_status``; ValueError for non-planar or mismatched
    input, a non-positive image size or refused flags."""
    fm = _flag_model(flags, camera_matrix, dist_coeffs)
    if fm is not None:
        return _calibrate_flags_host(object_points, image_points, image_size, fm)
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


def _cv2_tuple(r):
    """A ``CalibResult`` or ``RobustCalibResult`` -> cv2's 5-tuple, or the ValueError cv2 would end with."""
    bad = np.flatnonzero(r.view_status != PNP_OK)
    if bad.size:
        raise ValueError(f"view {int(bad[0])} cannot be used (status {int(r.view_status[bad[0]])})")
    if r.status != CALIB_OK:
        raise ValueError(f"calibration failed (status {r.status})")
    return (r.rms, r.camera_matrix, r.dist_coeffs, tuple(v.reshape(3, 1).copy() for v in r.rvecs),
            tuple(v.reshape(3, 1).copy() for v in r.tvecs))


def _no_bad_id(r, col_count, row_count):
    """``r``, or IndexError if one of its views carries an id outside the board."""
    if (r.view_status == PNP_BAD_ID).any():
        raise _bad_id_error(col_count, row_count)
    return r


def calibrate_camera_host(object_points, image_points, image_size, flags: int = 0, camera_matrix=None, dist_coeffs=None):
    """cv2's 5-tuple ``(rms, K 3x3, dist 1x5 or 1x8, rvecs, tvecs)`` (rvecs / tvecs: one (3, 1) array per view); ``flags``,
    ``camera_matrix``, ``dist_coeffs`` as for ``calibrate_camera_host_full``.  ValueError, as cv2 errors out, on non-planar objects,
    a view that cannot be used (fewer than 4 points, degenerate) or a failed calibration."""
    return _cv2_tuple(calibrate_camera_host_full(object_points, image_points, image_size, flags, camera_matrix, dist_coeffs))


# ------------------------------------------------------------------------------------------------ consensus: the definition

class RobustCalibResult(NamedTuple):
    status: int                  # CALIB_* of the last solve
    rms: float                   # over the inlier rows of the views used
    camera_matrix: np.ndarray
    dist_coeffs: np.ndarray
    view_status: np.ndarray      # int32 [B], pnp.PNP_* (incl. NO_CONSENSUS, and DEGENERATE for a view without a hypothesis)
    rvecs: np.ndarray
    tvecs: np.ndarray
    view_rms: np.ndarray         # [B], over the view's inlier rows
    view_points: np.ndarray      # int64 [B]: the rows OFFERED by the view
    iterations: int
    attempts: int
    views_used: int
    points_used: int             # inlier rows of the views used
    inliers: list                # per view a bool array: the mask the last solve was given (all False for a view left out)
    view_inliers: np.ndarray     # int64 [B]
    winners: np.ndarray          # int32 [B]: the winning hypothesis, -1 where there is none
    solves: int                  # joint solves run (1 .. 1 + rounds)
    stable: bool                 # the last re-mask changed nothing (False when none ran after the last solve)


def _calib_ransac_args(iterations, consensus_error, reproj_error, min_inliers, rounds):
    iterations, reproj_error, min_inliers = pnp._ransac_args(iterations, reproj_error, min_inliers)
    if not (math.isfinite(float(consensus_error)) and float(consensus_error) > 0):
        raise ValueError("consensus_error must be finite and positive")
    if not 0 <= int(rounds) <= RANSAC_MAX_ROUNDS:
        raise ValueError(f"rounds must be in [0, {RANSAC_MAX_ROUNDS}]")
    return iterations, float(consensus_error), reproj_error, min_inliers, int(rounds)


def _transfer_errors2(H: np.ndarray, mc: np.ndarray, obj: np.ndarray, img: np.ndarray) -> np.ndarray:
    """Squared distance (px^2) of every row's image point from H (board xy - mc); inf where q_z <= 0."""
    X, Y = obj[:, 0] - mc[0], obj[:, 1] - mc[1]
    qx = H[0, 0] * X + H[0, 1] * Y + H[0, 2]
    qy = H[1, 0] * X + H[1, 1] * Y + H[1, 2]
    qz = H[2, 0] * X + H[2, 1] * Y + H[2, 2]
    e2 = np.full(obj.shape[0], math.inf)
    f = qz > 0
    du, dv = qx[f] / qz[f] - img[f, 0], qy[f] / qz[f] - img[f, 1]
    e2[f] = du * du + dv * dv
    return e2


def _margin(e2: np.ndarray, thr: float) -> float:
    e2 = e2[np.isfinite(e2)]
    return float(np.abs(np.sqrt(e2) - thr).min()) / thr if e2.size else math.inf


def _view_consensus(obj, img, ids, row_count, iterations, thr, min_inliers, seed):
    """Step B for one view (rows in pool order, float64) -> (status, mask, winner, score, margin).  Only the view's own rows
    and (seed, n, h) enter: the outcome does not depend on the view's place in a batch."""
    n = obj.shape[0]
    best, winner, best_e2, records = -1, -1, None, []
    for h in range(iterations):
        s = pnp._ransac_sample(seed, n, h, ids, row_count - 1)
        if s is None:
            continue
        st, H, mc = pnp._homography4(obj[s], img[s])        # board xy - centroid -> RAW pixels: there is no model to undistort by
        if st != PNP_OK:
            continue
        e2 = _transfer_errors2(H, mc, obj, img)
        score = int((e2 <= thr * thr).sum())
        records.append((score, e2))
        if score > best:
            best, winner, best_e2 = score, h, e2
    if winner < 0:
        return PNP_DEGENERATE, np.zeros(n, bool), -1, 0, math.inf
    margin = min(_margin(e2, thr) for sc, e2 in records if sc >= best - 1)
    if best < max(min_inliers, 4):
        return PNP_NO_CONSENSUS, np.zeros(n, bool), winner, best, margin
    return PNP_OK, best_e2 <= thr * thr, winner, best, margin


def calibrate_camera_ransac_host_full(keypoints_list, col_count, row_count, square_len, image_size, iterations=100,
                                      consensus_error=8.0, reproj_error=3.0, min_inliers=6, rounds=2, seed=0, with_margin=False,
                                      pool_order=False):
    """The definition of the robust calibration -> ``RobustCalibResult`` (with ``with_margin``: ``(result, margin)``).

    ``keypoints_list``: per view an array of [x, y, id] rows.  Rows are taken in the order the corner pool holds them, as in
    ``pnp.solve_pnp_ransac_host_full``: id-sorted stably, or as they stand with ``pool_order=True``.  Object points are
    ``pnp.object_points`` (float32 -> float64), image points float32 -> float64.

    A. per-view checks, with ``calibrate_charuco_pool``'s codes: fewer than 4 rows TOO_FEW, an id outside the board BAD_ID.
    B. consensus per view, without a camera: hypothesis h draws four rows with ``pnp._ransac_sample`` and takes
       ``pnp._homography4`` through them, board xy minus the sample's centroid -> RAW pixels (a pose hypothesis would need the
       model this call is about to estimate; a homography has to absorb the lens, which is what ``consensus_error`` allows for).
       Its score is the rows with |H(X) - x|^2 <= consensus_error^2 (q_z <= 0: an outlier).  All hypotheses are scored; the
       winner is the highest score, the lowest h among equals.  No hypothesis: DEGENERATE; a score below max(min_inliers, 4):
       NO_CONSENSUS; else the view's mask is the winner's.
    C. ``calibrate_camera_host_full`` on the masked rows of the views that still stand (so a batch whose masks are all true gives
       the plain result bit for bit).  A view that fails the solve's checks gets that status.  An overall status other than
       CALIB_OK is returned as it is, with the masks that were used.
    D. at most ``rounds`` times: ALL rows of every view the last solve used are projected through the solved (K, dist, rvec, tvec)
       (``pnp._row_errors2``); the new mask is e^2 <= reproj_error^2; a view left with fewer than max(min_inliers, 4) rows
       becomes NO_CONSENSUS with an all-false mask; views left out earlier never come back.  If no mask changed: ``stable``, stop.
       Else solve again FROM SCRATCH on the new masks.  The result is always the last solve with the masks it was given, so
       ``stable`` is False when the rounds ran out (or ``rounds=0``) before a re-mask could confirm the last solve.

    The defaults are parameters, not measured claims: 8 px for the homography (solvePnPRansac's default), 3 px for the model;
    min_inliers 6 because four rows always agree with the homography through themselves.

    ``with_margin``: the smallest relative distance of any decision to its threshold: in B the rows of every hypothesis that
    scores within one of its view's winner against ``consensus_error``, in D every row at every re-mask against ``reproj_error``."""
    w, h = _image_size(image_size)
    iterations, cthr, rthr, min_inliers, rounds = _calib_ransac_args(iterations, consensus_error, reproj_error, min_inliers, rounds)
    need = max(min_inliers, 4)
    B, n_ids = len(keypoints_list), (col_count - 1) * (row_count - 1)
    vstat = np.full(B, PNP_OK, np.int32)                     # steps A, B, D: OK = the view still stands
    winners = np.full(B, -1, np.int32)
    offered = np.zeros(B, np.int64)
    orders, obj32, img32, masks = [None] * B, [None] * B, [None] * B, [None] * B
    margin = math.inf
    for b, kp in enumerate(keypoints_list):
        kp, orders[b] = _pool_rows(kp, pool_order)
        n = offered[b] = kp.shape[0]
        masks[b] = np.zeros(n, bool)
        if n < 4:
            vstat[b] = PNP_TOO_FEW
            continue
        kp = kp[orders[b]]
        ids = kp[:, 2].astype(np.int64)
        if ids.min() < 0 or ids.max() >= n_ids:
            vstat[b] = PNP_BAD_ID
            continue
        obj32[b], img32[b] = pnp.object_points(ids, col_count, row_count, square_len), kp[:, :2].astype(np.float32)
        vstat[b], masks[b], winners[b], _, mg = _view_consensus(obj32[b].astype(np.float64), img32[b].astype(np.float64), ids,
                                                                row_count, iterations, cthr, min_inliers, seed)
        margin = min(margin, mg)

    solves, stable = 0, False
    while True:
        standing = np.flatnonzero(vstat == PNP_OK)
        r = calibrate_camera_host_full([obj32[b][masks[b]] for b in standing], [img32[b][masks[b]] for b in standing], (w, h))
        solves += 1
        if r.status != CALIB_OK or solves > rounds:
            break
        k8 = np.zeros(8)
        k8[:5] = r.dist_coeffs.ravel()
        changed = False
        for j, b in enumerate(standing):
            if r.view_status[j] != PNP_OK:                   # not used by the solve: nothing to project it through
                continue
            e2 = pnp._row_errors2(obj32[b].astype(np.float64), img32[b].astype(np.float64), np.r_[r.rvecs[j], r.tvecs[j]],
                                  r.camera_matrix, k8)
            margin = min(margin, _margin(e2, rthr))
            m = e2 <= rthr * rthr
            if int(m.sum()) < need:
                vstat[b], m = PNP_NO_CONSENSUS, np.zeros(m.size, bool)
            changed |= not np.array_equal(m, masks[b])
            masks[b] = m
        if not changed:
            stable = True
            break

    view_status = vstat.copy()
    view_status[standing] = r.view_status
    rv, tv, vr = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B)
    rv[standing], tv[standing], vr[standing] = r.rvecs, r.tvecs, r.view_rms
    inliers = []
    for b in range(B):
        m = np.empty(masks[b].size, bool)
        m[orders[b]] = masks[b]                               # back to the caller's row order
        inliers.append(m)
    out = RobustCalibResult(r.status, r.rms, r.camera_matrix, r.dist_coeffs, view_status, rv, tv, vr, offered, r.iterations,
                            r.attempts, r.views_used, r.points_used, inliers, np.array([int(m.sum()) for m in inliers], np.int64),
                            winners, solves, stable)
    return (out, margin) if with_margin else out


def calibrate_camera_ransac_host(keypoints_list, col_count, row_count, square_len, image_size, iterations=100, consensus_error=8.0,
                                 reproj_error=3.0, min_inliers=6, rounds=2, seed=0):
    """cv2's 5-tuple plus the masks: ``(rms, K 3x3, dist 1x5, rvecs, tvecs, inliers)``.  Raises like ``calibrate_camera_host``:
    ValueError for a view that cannot be used (too few rows, no consensus, degenerate) or a failed calibration; IndexError for an
    id outside the board."""
    r = calibrate_camera_ransac_host_full(keypoints_list, col_count, row_count, square_len, image_size, iterations,
                                          consensus_error, reproj_error, min_inliers, rounds, seed)
    return _cv2_tuple(_no_bad_id(r, col_count, row_count)) + (r.inliers,)


# ------------------------------------------------------------------------------------------------ the device solver

def workspace_bytes(batch: int) -> int:
    from . import _lib
    return int(_lib.lib().dcx_calibrate_workspace_bytes(int(batch)))


def _common_fields(res, view_status, pose, n_dist=5) -> tuple:
    """The 16-double result of a device calibration (``n_dist`` distortion coefficients from word 4: 5, the fisheye model's 4) and
    the host copies of its per-view outputs -> the fields that ``CalibResult`` and ``RobustCalibResult`` share, in their order."""
    r = np.array(res[:], np.float64)
    status = int(r[14])
    K = _camera_matrix(r) if status == CALIB_OK else np.zeros((3, 3))
    return (status, float(r[9]), K, r[4:4 + n_dist].reshape(1, n_dist).copy(), view_status.astype(np.int32), pose[:, 0:3].copy(),
            pose[:, 3:6].copy(), pose[:, 6].copy(), pose[:, 7].astype(np.int64), int(r[10]), int(r[11]), int(r[12]), int(r[13]))


def _view_outputs(batch, dev):
    """-> what a calibration writes per view on the device: status int32 [B], pose float64 [B, POSE_WORDS]."""
    import torch
    return torch.empty((batch,), dtype=torch.int32, device=dev), torch.empty((batch, pnp.POSE_WORDS), dtype=torch.float64, device=dev)


def _upload(keypoints_list, dev):
    """The ``calibrate_*_device`` calls' views -> ``pack_keypoints``' (packed, batch, pool).  ValueError for no views."""
    if len(keypoints_list) == 0:
        raise ValueError("no views")
    return pack_keypoints(keypoints_list, dev)


def flags_workspace_bytes(batch: int, flags: int) -> int:
    """Bytes of device workspace ``dcx_calibrate_flags_pool`` needs; a guess whose k4 k5 k6 are not all zero needs the size of
    ``flags | CALIB_RATIONAL_MODEL``."""
    from . import _lib
    n = int(_lib.lib().dcx_calibrate_flags_workspace_bytes(int(batch), int(flags)))
    if n == 0:
        raise ValueError("batch >= 1 and known flags are required")
    return n


def _flags_result(res, view_status, pose, fm: _FlagModel) -> CalibResult:
    """``dcx_calibrate_flags_pool``'s 20 doubles (theta12, then rms .. status) -> ``CalibResult``."""
    r = np.array(res[:], np.float64)
    r16 = np.r_[r[:9], r[12:18], 0.0]                     # dcx_calibrate_pool's places
    f = list(_common_fields(r16, view_status, pose))
    f[3] = r[4:4 + fm.n_dist].reshape(1, fm.n_dist).copy()
    return CalibResult(*f, flags=fm.flags)


def _calibrate_flags_pool(packed, batch, pool, refined, col_count, row_count, square_len, image_size, fm: _FlagModel) -> CalibResult:
    import torch
    from . import _lib
    w, h = _image_size(image_size)
    dev = packed.device
    ptrs = pnp._pool_ptrs(packed, batch, pool, refined)
    st, pose = _view_outputs(batch, dev)
    nbytes = flags_workspace_bytes(batch, fm.flags | (CALIB_RATIONAL_MODEL if fm.rational else 0))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    res = (_ctypes.c_double * FLAGS_RESULT_WORDS)()
    cam, dist, n_dist = None, None, 0
    if fm.guess is not None:
        cam = (_ctypes.c_double * 9)(*_camera_matrix(fm.guess).ravel().tolist())
        dist, n_dist = (_ctypes.c_double * 8)(*fm.guess[4:].tolist()), 8
    elif fm.ratio is not None:
        cam = (_ctypes.c_double * 9)(fm.ratio, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)      # only the ratio fx / fy is read
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_calibrate_flags_pool(*ptrs, int(batch), int(pool), int(col_count), int(row_count), float(square_len),
                                                       w, h, fm.flags, cam, dist, n_dist, ws.data_ptr(), nbytes, st.data_ptr(),
                                                       pose.data_ptr(), res, _lib.current_stream()), "dcx_calibrate_flags_pool")
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
    return _flags_result(res, st_h, pose_h, fm)


def calibrate_charuco_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len,
                           image_size, flags: int = 0, camera_matrix=None, dist_coeffs=None) -> CalibResult:
    """Calibrate from every frame of an ``infer_batch_device`` result, read in place from the corner pool (the conventions of
    ``pnp.solve_pnp_pool``: ``refined`` = the pool carries RefineNet's xy, else the integer rows are the image points).  Object
    points are ``pnp.object_points``' float32 board corners.  ``image_size`` = (width, height) as in cv2.  ``flags``,
    ``camera_matrix``, ``dist_coeffs`` as for ``calibrate_camera_host_full``: ``flags = 0`` is ``dcx_calibrate_pool``, anything else
    ``dcx_calibrate_flags_pool``.  The call synchronises the current stream (the LM loop reads one state word per step) and cannot
    be captured in a graph."""
    import torch
    from . import _lib
    fm = _flag_model(flags, camera_matrix, dist_coeffs)
    if fm is not None:
        return _calibrate_flags_pool(packed, batch, pool, refined, col_count, row_count, square_len, image_size, fm)
    w, h = _image_size(image_size)
    dev = packed.device
    ptrs = pnp._pool_ptrs(packed, batch, pool, refined)
    st, pose = _view_outputs(batch, dev)
    nbytes = workspace_bytes(batch)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    res = (_ctypes.c_double * RESULT_WORDS)()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_calibrate_pool(*ptrs, int(batch), int(pool), int(col_count), int(row_count), float(square_len),
                                                 w, h, ws.data_ptr(), nbytes, st.data_ptr(), pose.data_ptr(), res,
                                                 _lib.current_stream()), "dcx_calibrate_pool")
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
    return CalibResult(*_common_fields(res, st_h, pose_h))


def calibrate_charuco_device(keypoints_list: Sequence, col_count, row_count, square_len, image_size,
                             device="cuda", flags: int = 0, camera_matrix=None, dist_coeffs=None) -> CalibResult:
    """Calibrate from ``infer_image``-format keypoint arrays ([x, y, id] rows, any number of frames and of corners each) on the
    GPU -> ``CalibResult``; ``flags``, ``camera_matrix``, ``dist_coeffs`` as for ``calibrate_camera_host_full``.  IndexError if a
    frame with >= 4 points carries an id outside the board."""
    import torch
    from .models._handles import require_cuda
    _flag_model(flags, camera_matrix, dist_coeffs)
    dev = require_cuda(device)
    _image_size(image_size)
    packed, b, pool = _upload(keypoints_list, dev)
    with torch.cuda.device(dev):
        r = calibrate_charuco_pool(packed, b, pool, True, col_count, row_count, square_len, image_size, flags, camera_matrix,
                                   dist_coeffs)
    return _no_bad_id(r, col_count, row_count)


# ------------------------------------------------------------------------------------------------ consensus on the device

def ransac_workspace_bytes(batch: int, pool: int, iterations: int = 100) -> int:
    """Bytes of device workspace ``calibrate_charuco_ransac_pool`` needs (the scores, the filtered pool, the masks and the inner
    solve's workspace)."""
    from . import _lib
    n = int(_lib.lib().dcx_calibrate_ransac_workspace_bytes(int(batch), int(pool), int(iterations)))
    if n == 0:
        raise ValueError(f"batch >= 1, pool >= 0 and iterations in [1, {pnp.RANSAC_MAX_ITERATIONS}] are required")
    return n


def calibrate_charuco_ransac_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, image_size,
                                  iterations=100, consensus_error=8.0, reproj_error=3.0, min_inliers=6, rounds=2, seed=0,
                                  out_inliers=None) -> RobustCalibResult:
    """``calibrate_charuco_pool`` behind the consensus search and re-check of ``calibrate_camera_ransac_host_full`` (the
    definition), read in place from the corner pool.  The views' slot ranges must not overlap (DcxError).  ``inliers`` holds each
    view's mask in SLOT order (``counts[b]`` values; all False for a view cut by the pool).  ``out_inliers``: a contiguous uint8
    device tensor of at least ``pool`` values that receives the mask by slot; slots of no view are not written.  Like
    ``calibrate_charuco_pool`` the call synchronises the current stream and cannot be captured in a graph."""
    import torch
    from . import _lib
    w, h = _image_size(image_size)
    iterations, cthr, rthr, min_inliers, rounds = _calib_ransac_args(iterations, consensus_error, reproj_error, min_inliers, rounds)
    dev = packed.device
    ptrs = pnp._pool_ptrs(packed, batch, pool, refined)
    out_inliers = _dev.tensor(out_inliers, dev, torch.uint8, (pool,),
                              f"out_inliers must be a contiguous uint8 tensor of at least {pool} values on {dev}", "min", zeros=True)
    st, pose = _view_outputs(batch, dev)
    info = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    nbytes = ransac_workspace_bytes(batch, pool, iterations)
    ws = _dev.workspace(None, dev, nbytes)
    res = (_ctypes.c_double * RESULT_WORDS)()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_calibrate_ransac_pool(
            *ptrs, int(batch), int(pool), int(col_count), int(row_count), float(square_len), w, h, iterations, cthr, rthr,
            min_inliers, rounds, int(seed) & 0xFFFFFFFF,
            ws.data_ptr(), nbytes, st.data_ptr(), pose.data_ptr(), info.data_ptr(), out_inliers.data_ptr(), res,
            _lib.current_stream()), "dcx_calibrate_ransac_pool")
        st_h, pose_h, info_h, inl_h, head = (t.cpu().numpy() for t in (st, pose, info, out_inliers, packed[:layout(batch, pool).rows]))
    inl_b, solves = inl_h.astype(bool), int(res[15])
    counts, starts = views(head, batch, pool)[:2]
    inliers = [inl_b[s0:s0 + n] if n > 0 and s0 >= 0 and s0 + n <= pool else np.zeros(max(n, 0), bool)
               for n, s0 in zip(counts.tolist(), starts.tolist())]
    return RobustCalibResult(*_common_fields(res, st_h, pose_h), inliers, info_h[:, 0].astype(np.int64),
                             info_h[:, 1].astype(np.int32), solves % 16, solves >= 16)


def calibrate_charuco_ransac_device(keypoints_list: Sequence, col_count, row_count, square_len, image_size, iterations=100,
                                    consensus_error=8.0, reproj_error=3.0, min_inliers=6, rounds=2, seed=0,
                                    device="cuda") -> RobustCalibResult:
    """The robust calibration from ``infer_image``-format keypoint arrays on the GPU -> ``RobustCalibResult``, the masks in the
    caller's row order.  IndexError if a view with >= 4 points carries an id outside the board."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    _image_size(image_size)
    _calib_ransac_args(iterations, consensus_error, reproj_error, min_inliers, rounds)
    packed, b, pool = _upload(keypoints_list, dev)
    with torch.cuda.device(dev):
        r = calibrate_charuco_ransac_pool(packed, b, pool, True, col_count, row_count, square_len, image_size, iterations,
                                          consensus_error, reproj_error, min_inliers, rounds, seed)
    _no_bad_id(r, col_count, row_count)
    # undo pack_keypoints' stable id sort
    return r._replace(inliers=[mask[_caller_order(kp)] for kp, mask in zip(keypoints_list, r.inliers)])


# ------------------------------------------------------------------------------------------------ how well the model is determined

COV_OK, COV_NO_VIEWS, COV_NO_DOF, COV_SINGULAR = range(4)       # DCX_COV_* of include/deepcharuco_amd.h
COV_GLOBAL_WORDS, COV_POSE_WORDS = 96, 42                       # d_global, a view of d_pose_cov (DCX_COV_GLOBAL_WORDS, DCX_COV_POSE_WORDS)
_COV_STD, _COV_SIGMA2 = 81, 90                                  # DCX_COV_STD; DCX_COV_SIGMA2, then dof, points, views, status
CAMERA_PINHOLE, CAMERA_FISHEYE = 0, 1                           # DCX_CAMERA_*


class CalibUncertainty(NamedTuple):
    status: int                  # COV_*
    sigma2: float                # sum |r|^2 / dof (px^2): the variance of one image coordinate the residuals imply
    dof: int                     # 2 * points - intrinsics - 6 * views
    points: int                  # kept rows of the views used
    views: int                   # views used
    std_intrinsics: np.ndarray   # [NG]: fx fy cx cy, then the model's distortion coefficients (cv2's stdDeviationsIntrinsics)
    cov_intrinsics: np.ndarray   # [NG, NG]
    std_extrinsics: np.ndarray   # [B, 6]: rvec then tvec (cv2's order); zeros unless the view was used
    cov_extrinsics: np.ndarray   # [B, 6, 6]


def _uncertainty(views, view_status, theta: np.ndarray, poses: np.ndarray, project_full) -> CalibUncertainty:
    """The definition (``calibration_uncertainty_host``) on checked arguments: ``views`` with their masks applied, ``poses``
    [B, 6], ``project_full`` the camera model's."""
    B, n = len(views), theta.size
    used = np.flatnonzero(view_status == PNP_OK)
    points = int(sum(views[i][0].shape[0] for i in used))
    dof = 2 * points - n - 6 * int(used.size)

    def out(status, sigma2=0.0, cov=None, blocks=None):
        ci, ce = np.zeros((n, n)), np.zeros((B, 6, 6))
        if status == COV_OK:
            ci, ce[used] = cov, blocks
        return CalibUncertainty(status, float(sigma2), dof, points, int(used.size), np.sqrt(np.diag(ci)), ci,
                                np.sqrt(np.diagonal(ce, axis1=1, axis2=2)), ce)

    if not used.size:
        return out(COV_NO_VIEWS)
    if dof <= 0:
        return out(COV_NO_DOF)
    if not (np.isfinite(theta).all() and np.isfinite(poses[used]).all()):
        return out(COV_SINGULAR)
    nb = _normal_blocks([views[i] for i in used], theta, poses[used], project_full)
    if nb is None:
        return out(COV_SINGULAR)
    U, W, V, _, _, costs = nb
    inv = _lm.schur_covariance(U, W, V, costs)
    if inv is None:
        return out(COV_SINGULAR)
    sigma2 = _total(costs) / dof
    cov, blocks = sigma2 * inv[0], sigma2 * inv[1]
    if not (math.isfinite(sigma2) and np.isfinite(cov).all() and np.isfinite(blocks).all()):
        return out(COV_SINGULAR)
    return out(COV_OK, sigma2, cov, blocks)


def _is_result(x) -> bool:
    return hasattr(x, "camera_matrix") and hasattr(x, "view_status")


def _free_model(camera_matrix, dist_coeffs, n_dist: int) -> np.ndarray:
    """(K, the model's ``n_dist`` free distortion coefficients) -> theta.  ValueError for any other number of coefficients: one
    that the solver held fixed has no variance to report."""
    K = pnp._camera(camera_matrix)
    d = np.zeros(0) if dist_coeffs is None else np.asarray(dist_coeffs, dtype=np.float64).ravel()
    if d.size != n_dist:
        raise ValueError(f"{d.size} distortion coefficients: the uncertainty is that of the solvers' free parameters, fx fy cx cy and "
                         f"{n_dist} coefficients; a coefficient held fixed has no variance to report")
    if not np.isfinite(d).all():
        raise ValueError("distortion coefficients must be finite")
    return np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], d]


def _poses(rvecs, tvecs, B: int) -> np.ndarray:
    r = np.asarray(rvecs, dtype=np.float64).reshape(-1, 3) if B else np.zeros((0, 3))
    t = np.asarray(tvecs, dtype=np.float64).reshape(-1, 3) if B else np.zeros((0, 3))
    if r.shape[0] != B or t.shape[0] != B:
        raise ValueError(f"{B} views but {r.shape[0]} rvecs and {t.shape[0]} tvecs")
    return np.concatenate([r, t], 1)


def _view_status(view_status, B: int) -> np.ndarray:
    st = np.full(B, PNP_OK, np.int32) if view_status is None else np.asarray(view_status).astype(np.int32).ravel()
    if st.size != B:
        raise ValueError(f"{B} views but {st.size} view statuses")
    return st


def _model_args(camera_matrix, dist_coeffs, rvecs, tvecs, view_status, inliers):
    """The explicit arguments, or those of the ``CalibResult`` / ``RobustCalibResult`` given in ``camera_matrix``'s place (its
    ``inliers`` where it has them and none are given).  ValueError for a result whose calibration failed."""
    if not _is_result(camera_matrix):
        if rvecs is None or tvecs is None:
            raise ValueError("rvecs and tvecs are required with an explicit camera model")
        return camera_matrix, dist_coeffs, rvecs, tvecs, view_status, inliers
    r = camera_matrix
    if r.status != CALIB_OK:
        raise ValueError(f"the calibration failed (status {r.status}): there is no solution to take an uncertainty at")
    if getattr(r, "flags", 0) & ~CALIB_USE_INTRINSIC_GUESS:
        raise ValueError(f"a result solved with flags {r.flags:#x}: the uncertainty is that of the solvers' free parameters, and a "
                         f"parameter held fixed has no variance to report (covariances of flagged models are not computed)")
    return r.camera_matrix, r.dist_coeffs, r.rvecs, r.tvecs, r.view_status, inliers if inliers is not None else getattr(r, "inliers", None)


def _uncertainty_host(object_points, image_points, camera_matrix, dist_coeffs, rvecs, tvecs, view_status, inliers, n_dist,
                      project_full) -> CalibUncertainty:
    camera_matrix, dist_coeffs, rvecs, tvecs, view_status, inliers = _model_args(camera_matrix, dist_coeffs, rvecs, tvecs,
                                                                                 view_status, inliers)
    theta = _free_model(camera_matrix, dist_coeffs, n_dist)
    views = _views(object_points, image_points)
    B = len(views)
    if inliers is not None:
        if len(inliers) != B:
            raise ValueError(f"{B} views but {len(inliers)} inlier masks")
        for i, m in enumerate(inliers):
            m = np.asarray(m).astype(bool).ravel()
            if m.size != views[i][0].shape[0]:
                raise ValueError(f"view {i} has {views[i][0].shape[0]} rows but its mask {m.size}")
            views[i] = (views[i][0][m], views[i][1][m])            # a dropped row is a row that is not there
    return _uncertainty(views, _view_status(view_status, B), theta, _poses(rvecs, tvecs, B), project_full)


def calibration_uncertainty_host(object_points, image_points, camera_matrix, dist_coeffs=None, rvecs=None, tvecs=None,
                                 view_status=None, inliers=None) -> CalibUncertainty:
    """How well a solved pinhole calibration is determined: the covariance of theta = (fx, fy, cx, cy, k1, k2, p1, p2, k3) and of
    every used view's (rvec, tvec), cv2.calibrateCameraExtended's ``stdDeviationsIntrinsics`` / ``stdDeviationsExtrinsics``.  In
    float64 on the host; the definition and the pin of ``dcx_calibrate_uncertainty_pool``.

    ``camera_matrix``, ``dist_coeffs`` (exactly the solver's 5: ValueError otherwise, a coefficient held fixed has no variance),
    ``rvecs``, ``tvecs`` [B, 3]: the solution; ``view_status`` [B]: a view takes part where it is ``PNP_OK`` (None: every view);
    ``inliers``: per view a mask over its rows (None: every row).  In ``camera_matrix``'s place a ``CalibResult`` or a
    ``RobustCalibResult`` stands for all of them (its ``inliers`` included, in the row order of the points given here).

    With the undamped normal blocks of ``_normal_blocks`` at the solution, over the used views' kept rows:
    S = V - sum W_i U_i^-1 W_i^T, Y_i = U_i^-1 W_i^T, dof = 2 points - 9 - 6 views, sigma^2 = sum |r|^2 / dof,
    cov_intrinsics = sigma^2 S^-1, cov_pose_i = sigma^2 (U_i^-1 + Y_i S^-1 Y_i^T) (``_lm.schur_covariance``: the corner and the
    diagonal blocks of the inverse of the full normal matrix); the standard deviations are the roots of the diagonals.

    The dof convention: sigma^2 is the textbook estimator, residuals (two per point) minus parameters.  cv2 is believed to divide
    by (points - parameters) instead; that could not be checked against cv2 here, so ``sigma2``, ``dof``, ``points`` and ``views``
    are returned for a caller who wants another convention: covariances scale with sigma^2, standard deviations with its root.

    Statuses, in this order: ``COV_NO_VIEWS`` (no used view), ``COV_NO_DOF`` (dof <= 0), ``COV_SINGULAR`` (a U_i or S not positive
    definite, a point not in front of the camera, a value not finite).  Everything but the status and the counts is zero unless
    ``COV_OK``; views that were not used get zeros.  Not reported: the intrinsics-pose cross-covariances."""
    return _uncertainty_host(object_points, image_points, camera_matrix, dist_coeffs, rvecs, tvecs, view_status, inliers, 5,
                             _project_full)


# ---- on the device

def uncertainty_workspace_bytes(batch: int) -> int:
    """Bytes of device workspace ``calibration_uncertainty_pool`` needs (one size for both camera models)."""
    from . import _lib
    return int(_lib.lib().dcx_calibrate_uncertainty_workspace_bytes(int(batch)))


def _device_or_upload(x, dev, dtype, shape, what):
    """A device tensor is taken as it is (checked); anything else is an array to upload."""
    import torch
    if isinstance(x, torch.Tensor):
        if x.device != dev or x.dtype != dtype or tuple(x.shape) != tuple(shape) or not x.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
        return x
    a = np.ascontiguousarray(np.asarray(x), dtype={torch.int32: np.int32, torch.float64: np.float64}[dtype])
    if a.shape != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, not {a.shape}")
    return torch.from_numpy(a).to(dev)


def _slot_mask(inliers, packed, batch, pool, dev):
    """``inliers`` -> the mask by pool slot the entry takes (uint8 [>= pool]) or None: a device tensor in the format of
    ``calibrate_charuco_ransac_pool``'s ``out_inliers`` is taken as it is; per-view masks in SLOT order (``RobustCalibResult.inliers``
    of that call) are laid at their views' slots (this reads the pool's head: a copy to the host)."""
    import torch
    if inliers is None:
        return None
    if isinstance(inliers, torch.Tensor):
        if inliers.device != dev or inliers.dtype != torch.uint8 or inliers.numel() < pool or not inliers.is_contiguous():
            raise ValueError(f"inliers must be a contiguous uint8 tensor of at least {pool} values on {dev}")
        return inliers
    if len(inliers) != batch:
        raise ValueError(f"{batch} views but {len(inliers)} inlier masks")
    counts, starts = views(packed[:layout(batch, pool).rows].cpu().numpy(), batch, pool)[:2]
    mask = np.zeros(max(pool, 1), np.uint8)
    for m, n, s0 in zip(inliers, counts.tolist(), starts.tolist()):
        m = np.asarray(m).astype(np.uint8).ravel()
        if n > 0 and s0 >= 0 and s0 + n <= pool:
            if m.size != n:
                raise ValueError(f"a view has {n} rows but its mask {m.size}")
            mask[s0:s0 + n] = m
    return torch.from_numpy(mask).to(dev)


def _uncertainty_pool(model, n_dist, packed, batch, pool, refined, col_count, row_count, square_len, result_or_model, inliers,
                      workspace, out):
    import torch
    from . import _lib
    dev = packed.device
    ptrs = pnp._pool_ptrs(packed, batch, pool, refined)
    if _is_result(result_or_model):
        K, dist, rv, tv, st, inliers = _model_args(result_or_model, None, None, None, None, inliers)
        pose = np.zeros((batch, pnp.POSE_WORDS))
        pose[:, :6] = _poses(rv, tv, batch)
    else:
        try:
            K, dist, st, pose = result_or_model
        except (TypeError, ValueError):
            raise ValueError("result_or_model must be a CalibResult, a RobustCalibResult or (camera_matrix, dist_coeffs, view_status "
                             "[B], pose [B, 8])") from None
    theta = _free_model(K, dist, n_dist)
    st_d = _device_or_upload(st, dev, torch.int32, (batch,), "view_status")
    pose_d = _device_or_upload(pose, dev, torch.float64, (batch, pnp.POSE_WORDS), "pose")
    mask = _slot_mask(inliers, packed, batch, pool, dev)
    nbytes = uncertainty_workspace_bytes(batch)
    ws = _dev.workspace(workspace, dev, nbytes, f"workspace must be a contiguous tensor of at least {nbytes} bytes on {dev}")
    if out is None:
        out = (torch.empty((COV_GLOBAL_WORDS,), dtype=torch.float64, device=dev),
               torch.empty((batch, COV_POSE_WORDS), dtype=torch.float64, device=dev))
    glob = _dev.tensor(out[0], dev, torch.float64, (COV_GLOBAL_WORDS,), f"out[0] must be a contiguous float64 tensor of "
                       f"{COV_GLOBAL_WORDS} values on {dev}")
    pcov = _dev.tensor(out[1], dev, torch.float64, (batch, COV_POSE_WORDS), f"out[1] must be a contiguous float64 tensor "
                       f"[{batch}, {COV_POSE_WORDS}] on {dev}")
    th = (_ctypes.c_double * 9)(*theta.tolist())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_calibrate_uncertainty_pool(
            *ptrs, int(batch), int(pool), int(col_count), int(row_count), float(square_len), model, th, st_d.data_ptr(),
            pose_d.data_ptr(), None if mask is None else mask.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
            glob.data_ptr(), pcov.data_ptr(), _lib.current_stream()), "dcx_calibrate_uncertainty_pool")
    return glob, pcov


def calibration_uncertainty_pool(packed, batch: int, pool: int, refined: bool, col_count, row_count, square_len, result_or_model,
                                 inliers=None, workspace=None, out=None):
    """``calibration_uncertainty_host`` on the GPU, read in place from the corner pool the calibration read (the conventions of
    ``calibrate_charuco_pool``) -> device tensors ``(global_ float64 [COV_GLOBAL_WORDS], pose_cov float64 [B, COV_POSE_WORDS])``,
    which ``unpack_uncertainty`` turns into a ``CalibUncertainty``.

    ``result_or_model``: the ``CalibResult`` / ``RobustCalibResult`` of a calibration of this pool, or ``(camera_matrix,
    dist_coeffs, view_status [B] int32, pose [B, 8] float64)`` with the last two as arrays or as the device tensors the calibration
    wrote.  ``inliers``: a uint8 device tensor by slot (``calibrate_charuco_ransac_pool``'s ``out_inliers``), or per-view masks in
    slot order; None takes a ``RobustCalibResult``'s own.  ``workspace``: at least ``uncertainty_workspace_bytes(batch)`` bytes;
    ``out``: the two output tensors.  Four launches on the current stream.  Given device tensors throughout the call neither
    allocates nor synchronises and can be captured in a graph (a result tuple or per-view masks are uploaded first)."""
    return _uncertainty_pool(CAMERA_PINHOLE, 5, packed, batch, pool, refined, col_count, row_count, square_len, result_or_model,
                             inliers, workspace, out)


def unpack_uncertainty(global_, pose_cov, n_intr: int = N_INTR) -> CalibUncertainty:
    """The two tensors of ``calibration_uncertainty_pool`` (``n_intr`` = 9) or ``fisheye.calibration_uncertainty_fisheye_pool``
    (8) -> ``CalibUncertainty`` on the host."""
    g, p = global_.cpu().numpy(), pose_cov.cpu().numpy()
    s2, dof, points, nviews, status = g[_COV_SIGMA2:_COV_SIGMA2 + 5]
    return CalibUncertainty(int(status), float(s2), int(dof), int(points), int(nviews), g[_COV_STD:_COV_STD + n_intr].copy(),
                            g[:n_intr * n_intr].reshape(n_intr, n_intr).copy(), p[:, 36:42].copy(), p[:, :36].reshape(-1, 6, 6).copy())


def _uncertainty_device(model, n_dist, keypoints_list, col_count, row_count, square_len, result_or_model, inliers, device):
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    packed, b, pool = _upload(keypoints_list, dev)
    if inliers is None and _is_result(result_or_model):
        inliers = getattr(result_or_model, "inliers", None)
    if inliers is not None:                                    # the caller's row order -> the pool's (pack_keypoints' id sort)
        if len(inliers) != b:
            raise ValueError(f"{b} views but {len(inliers)} inlier masks")
        by_slot = []
        for kp, m in zip(keypoints_list, inliers):
            m, order = np.asarray(m).astype(bool).ravel(), _pool_rows(kp)[1]
            if m.size != order.size:
                raise ValueError(f"a view has {order.size} rows but its mask {m.size}")
            by_slot.append(m[order])
        inliers = by_slot
    with torch.cuda.device(dev):
        g, p = _uncertainty_pool(model, n_dist, packed, b, pool, True, col_count, row_count, square_len, result_or_model, inliers,
                                 None, None)
        return unpack_uncertainty(g, p, 4 + n_dist)


def calibration_uncertainty_device(keypoints_list: Sequence, col_count, row_count, square_len, result_or_model, inliers=None,
                                   device="cuda") -> CalibUncertainty:
    """``calibration_uncertainty_host`` on the GPU from ``infer_image``-format keypoint arrays ([x, y, id] rows), the views the
    calibration was given -> ``CalibUncertainty``.  ``result_or_model`` as for ``calibration_uncertainty_pool``; ``inliers``: per
    view a mask in the caller's row order (None takes a ``RobustCalibResult``'s own, as ``calibrate_charuco_ransac_device`` returns
    them)."""
    return _uncertainty_device(CAMERA_PINHOLE, 5, keypoints_list, col_count, row_count, square_len, result_or_model, inliers, device)
