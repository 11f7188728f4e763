"""Stereo extrinsic calibration without OpenCV: ``cv2.stereoCalibrate`` with CALIB_FIX_INTRINSIC (its default) from the ChArUco
corners of two rigidly mounted cameras, on the host and on the GPU.

Two cameras 0 and 1 with known ``(camera_matrix, dist_coeffs)`` (none, 4, 5 or 8 coefficients each, as the PnP entry points take
them; the two models may differ) see the same board at the same instants: view t of camera 0 and view t of camera 1 belong
together.  Every corner carries its id, so the two views of a timestamp need NOT share a single id (``cv2.stereoCalibrate`` needs
the same points in both images).  Unknowns: the rig transform X = (R, T) in cv2's convention, q1 = R q0 + T for a point q0 in
camera 0's frame, and the board's pose P_t in camera 0's frame for every timestamp that is used.  Cost: the squared pixel distance
of pi0(P_t o) to the rows of view (0, t) and of pi1(X P_t o) to the rows of view (1, t).  Steps, all in float64:

1. per-view checks with the PnP status codes.  An optional mask per view drops rows first (the format of the inlier masks the
   consensus calls emit; that is how they compose with this one); then fewer than 4 rows -> TOO_FEW, an id outside the board ->
   BAD_ID (from a pool also TRUNCATED);
2. per-view pose: ``pnp._solve`` with that camera's model, unchanged (a failure: DEGENERATE / NONFINITE).  A timestamp is a PAIR,
   and is used, only if both of its views are PNP_OK; the others are left out and reported per camera;
3. rig init: per pair R_t = R1_t R0_t^T, T_t = t1_t - R_t t0_t; X0 = the element-wise LOWER median over the pairs of the 9 entries
   of R_t and the 3 of T_t (element (n - 1) // 2 of the sorted values: no two values are averaged), the median matrix
   orthonormalised by the polar factor of ``pnp._pose_of_homography`` and passed through ``pnp._rvec_of``.  P_t starts at camera
   0's own pose;
4. joint Levenberg-Marquardt over X (6 parameters) and every used P_t (6 each), analytic Jacobians through SO(3)'s right Jacobian
   as in ``pnp._project``, the CvLevMarq rules of ``calib.py`` exactly (damping diag * (1 + 10^lg), lg from -3, +1 on a rejected
   step up to 16, then -1 down to -16; a point behind either camera is a rejection), at most 30 accepted steps, stop at
   |dp| / |p| < DBL_EPSILON over all 6 + 6N parameters.  Each step by block elimination: P_t couples only to X, so the 6x6 blocks
   U_t are eliminated (Schur complement) and one 6x6 system remains, solved by Cholesky;
5. outputs: rvec(R), T, rms = sqrt(sum |r|^2 / points used) over both cameras (cv2's return value), per timestamp P_t, both
   views' status, rms and row count; in Python from those E = [T]x R and F = K1^-T E K0^-1, scaled so that F[2, 2] = 1 where that
   entry is not zero (as cv2 does).

``stereo_calibrate_host_full`` is the readable definition and the test pin; ``stereo_calibrate_pool`` /
``stereo_calibrate_device`` run the same steps on the GPU (csrc/dcx_stereo.hip).  The two agree to rounding (summation order), not
bit for bit.  ``stereo_uncertainty_host`` / ``_pool`` / ``_device`` (end of the module) say how well the solved pair is determined:
``rig.rig_uncertainty_*`` with two cameras.

Deviations from ``cv2.stereoCalibrate``:
* the rig initialisation takes the median over MATRIX entries (then the polar factor) where cv2 takes it over rotation VECTORS: a
  rig whose relative rotation is near pi does not wrap (the vectors r and r (1 - 2 pi / |r|) are one rotation and far apart);
* the stop test uses DBL_EPSILON where cv2's default criteria for stereoCalibrate use 1e-6, for the reason ``calib.py`` gives: a
  stop decided well above rounding makes host and device stop a whole step apart;
* the two views of a timestamp need no common id, and their poses are initialised separately;
* each step is solved by Cholesky of the reduced system; unusable views are reported instead of raising
  (``stereo_calibrate_host`` raises like cv2).
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _dev, _lm, fisheye, pnp
from .calib import _no_bad_id
from .corner_pool import _pool_rows, pack_keypoints
from .pnp import (PNP_BAD_ID, PNP_OK, PNP_TOO_FEW, _bad_id_error, _camera, _dist, _jacobi, _pool_ptrs, _right_jacobian, _rodrigues,
                  _rvec_of, _skew, _solve)

# overall status (include/deepcharuco_amd.h); per-view statuses are pnp's PNP_*
STEREO_OK, STEREO_NO_PAIRS, STEREO_DEGENERATE, STEREO_NONFINITE = _lm.LM_OK, _lm.LM_NO_UNITS, _lm.LM_DEGENERATE, _lm.LM_NONFINITE
STEREO_MAX_ITER = 30
STEREO_EPS = float(np.finfo(np.float64).eps)
RESULT_WORDS = 16              # h_result of dcx_stereo_calibrate_pool
REDUCE_CHUNK, REDUCE_SLICES = 16, 16   # csrc/dcx_stereo.hip's kChunk, kSlices: the two fan-ins of the per-attempt reduction

__all__ = ["StereoResult", "stereo_calibrate_host", "stereo_calibrate_host_full", "stereo_calibrate_pool",
           "stereo_calibrate_device", "workspace_bytes", "essential_fundamental", "STEREO_OK", "STEREO_NO_PAIRS",
           "STEREO_DEGENERATE", "STEREO_NONFINITE", "stereo_uncertainty_host", "stereo_uncertainty_pool", "stereo_uncertainty_device"]


class StereoResult(NamedTuple):
    status: int                  # STEREO_*
    rms: float                   # sqrt(sum |r|^2 / points used) over both cameras: cv2.stereoCalibrate's return value
    R: np.ndarray                # 3x3: q1 = R q0 + T
    T: np.ndarray                # [3]
    rvec: np.ndarray             # [3] Rodrigues vector of R
    E: np.ndarray                # 3x3 [T]x R
    F: Optional[np.ndarray]      # 3x3 K1^-T E K0^-1, F[2, 2] = 1 where it is not zero; None for a pair with a fisheye camera
    view_status: np.ndarray      # int32 [T, 2], pnp.PNP_* per camera
    rvecs: np.ndarray            # [T, 3] the board's pose P_t in camera 0's frame; zeros unless the pair was used
    tvecs: np.ndarray            # [T, 3]
    pair_rms: np.ndarray         # [T] rms over both views of the pair at the solution (px)
    pair_points: np.ndarray      # int64 [T] rows of both views of a used pair; zeros unless STEREO_OK
    view_rms: np.ndarray         # [T, 2]
    view_points: np.ndarray      # int64 [T, 2] rows the view brings (after its mask), used or not
    iterations: int              # accepted LM steps
    attempts: int                # LM trial steps (accepted + rejected)
    pairs_used: int              # the pairs found and their rows, whatever the status
    points_used: int


# ------------------------------------------------------------------------------------------------ the fp64 steps
# Every step that does not depend on the number of cameras is written for C of them and kept here once; ``rig.py`` runs these same
# functions, and a pair is a rig of two cameras whose timestamps all have both views (``_rows_of`` through ``_rig_rows``, ``_pair_segments``).

def _project_q(Q: np.ndarray, img: np.ndarray, K: np.ndarray, k: np.ndarray, jac: bool):
    """Points Q (n, 3) in a camera's frame -> residuals (projected - observed, px) and, with ``jac``, d(u, v)/dQ (n, 2, 3):
    ``pnp._project``'s model and derivatives with the pose taken out.  Every Z must be positive (the caller checks)."""
    return pnp._project_q_through(pnp._distort, Q, img, K, k, jac)


MODELS = ("pinhole", "fisheye")      # DCX_CAMERA_PINHOLE, DCX_CAMERA_FISHEYE of include/deepcharuco_amd.h, in that order
# what the steps need of a camera model: its pose solve and its projection of camera-frame points
_MODEL = {"pinhole": (_solve, _project_q), "fisheye": (fisheye._solve, fisheye._project_q)}


def _model_of(cam):
    """A camera of the steps is (K, k), a pinhole, or (K, k, model) -> (solve, project_q) of its model."""
    return _MODEL[cam[2] if len(cam) > 2 else "pinhole"]


def _models(models, n_cams):
    """``models`` of the entry points -> None, or the model names, one per camera."""
    if models is None:
        return None
    models = list(models)
    if len(models) != n_cams or any(m not in MODELS for m in models):
        raise ValueError(f"models must be None or one of {MODELS} per camera")
    return models


def _model_cameras(cameras, dists, models):
    """-> the cameras of the steps: (K, k) for a pinhole (and for every camera without ``models``), (K, k1..k4, model) else."""
    if models is None:
        return [(_camera(K), _dist(d)) for K, d in zip(cameras, dists)]
    return [(_camera(K), _dist(d)) if m == "pinhole" else (_camera(K), fisheye._dist4(d), m) for K, d, m in zip(cameras, dists, models)]


def _model_args(camera, dist, model):
    """One camera's (camera9, dist, n_dist) of the C entries that take a model: a fisheye camera's k1..k4 ride in dist[0..3]."""
    if model != "fisheye":
        return pnp._camera_args(camera, dist)
    cam9, d4 = fisheye._camera_args(camera, dist)
    return cam9, (_ctypes.c_double * 8)(*d4), 0 if dist is None else 4


class _Rows(NamedTuple):
    """Every row of every used timestamp: timestamp by timestamp, its usable cameras ascending, each view's rows in pool order."""
    obj: np.ndarray              # (M, 3) board points
    img: np.ndarray              # (M, 2)
    cam: np.ndarray              # (M,) the row's camera
    stamp: np.ndarray            # (M,) index of the row's timestamp among the used ones
    starts: np.ndarray           # (N,) first row of every timestamp
    vstarts: np.ndarray          # (NV,) first row of every view
    vstamp: np.ndarray           # (NV,) the view's timestamp (index among the used ones) ...
    vcam: np.ndarray             # (NV,) ... and camera
    n_cams: int

    @property
    def pair(self) -> np.ndarray:
        """``stamp`` under the name it has for two cameras."""
        return self.stamp


def _rig_rows(stamps, n_cams: int) -> _Rows:
    """Per used timestamp a list of (camera, obj, img) of its usable views, cameras ascending -> the rows, in float64."""
    obj, img, cam, stamp, counts, vstamp, vcam, per_stamp = [], [], [], [], [], [], [], []
    for i, views in enumerate(stamps):
        per_stamp.append(sum(o.shape[0] for _, o, _ in views))
        for c, o, m in views:
            n = o.shape[0]
            obj.append(np.asarray(o, np.float64))
            img.append(np.asarray(m, np.float64))
            cam.append(np.full(n, c))
            stamp.append(np.full(n, i))
            counts.append(n)
            vstamp.append(i)
            vcam.append(c)
    vstarts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(per_stamp)[:-1]]).astype(np.int64)
    return _Rows(np.concatenate(obj), np.concatenate(img), np.concatenate(cam), np.concatenate(stamp), starts, vstarts,
                 np.array(vstamp), np.array(vcam), n_cams)


def _rows_of(pairs) -> _Rows:
    """Per pair (obj0, img0, obj1, img1) -> the rows of a rig of two cameras whose timestamps all have both views."""
    return _rig_rows([[(0, v[0], v[1]), (1, v[2], v[3])] for v in pairs], 2)


def _view_segments(rows: _Rows):
    """``_normal_blocks``' segments with one per view: the rig's."""
    return rows.vstarts, rows.vstamp.tolist(), rows.vcam.tolist()


def _pair_segments(rows: _Rows):
    """``_normal_blocks``' segments with one per pair, camera 0's rows (whose J_X is zero) before camera 1's: the stereo solve's."""
    return rows.starts, list(range(rows.starts.size)), [1] * rows.starts.size


def _skews(v: np.ndarray) -> np.ndarray:
    S = np.zeros((v.shape[0], 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -v[:, 2], v[:, 1]
    S[:, 1, 0], S[:, 1, 2] = v[:, 2], -v[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -v[:, 1], v[:, 0]
    return S


def _points(rows: _Rows, X: np.ndarray, P: np.ndarray):
    """-> (q_0 (M, 3): the rows' board points in camera 0's frame, q (M, 3): in their own camera's, R(X_c) [C - 1, 3, 3], R(P_t))."""
    RP = np.stack([_rodrigues(p[:3]) for p in P])
    RX = np.stack([_rodrigues(x[:3]) for x in X])
    Q0 = np.einsum("mij,mj->mi", RP[rows.stamp], rows.obj) + P[rows.stamp, 3:]
    Q = Q0.copy()
    for c in range(1, rows.n_cams):
        sel = rows.cam == c
        Q[sel] = Q0[sel] @ RX[c - 1].T + X[c - 1, 3:]
    return Q0, Q, RX, RP


def _evaluate(rows: _Rows, cams, X: np.ndarray, P: np.ndarray, jac: bool):
    """Residuals (M, 2) at the rig X [C - 1, 6] (or, for two cameras, [6]) of (rvec, T) and the board poses P [N, 6], and with
    ``jac`` the rows' Jacobians J_X (M, 2, 6) with respect to the row's OWN camera's X_c (zero for camera 0's rows) and J_P
    (M, 2, 6) with respect to the row's own P_t.  None if a point is not in front of its camera."""
    X = X.reshape(-1, 6)
    Q0, Q, RX, RP = _points(rows, X, P)
    if not (Q[:, 2] > 0).all():
        return None
    M = rows.obj.shape[0]
    res, D = np.empty((M, 2)), (np.empty((M, 2, 3)) if jac else None)
    for c, cam in enumerate(cams):
        sel = rows.cam == c
        if not sel.any():
            continue
        r, d = _model_of(cam)[1](Q[sel], rows.img[sel], cam[0], cam[1], jac)
        res[sel] = r
        if jac:
            D[sel] = d
    if not jac:
        return res, None, None
    JrP = np.stack([_right_jacobian(p[:3]) for p in P])
    dQ0_dr = -np.einsum("mij,mjk,mkl->mil", RP[rows.stamp], _skews(rows.obj), JrP[rows.stamp])    # -R_P [o]x Jr(r_P)
    Dp = D.copy()
    JX = np.zeros((M, 2, 6))
    for c in range(1, rows.n_cams):
        sel = rows.cam == c
        if not sel.any():
            continue
        Dp[sel] = D[sel] @ RX[c - 1]                           # camera c sees q_0 through R_c: d(u, v)/dq_0 = d(u, v)/dq R_c
        dQ_drx = -np.einsum("ij,mjk,kl->mil", RX[c - 1], _skews(Q0[sel]), _right_jacobian(X[c - 1, :3]))   # -R_c [q_0]x Jr(r_c)
        JX[sel, :, :3] = D[sel] @ dQ_drx
        JX[sel, :, 3:] = D[sel]
    JP = np.concatenate([Dp @ dQ0_dr, Dp], 2)
    return res, JX, JP


def _view_costs(rows: _Rows, res: np.ndarray) -> np.ndarray:
    """-> [N, C]: the cost of every usable view, zero elsewhere."""
    out = np.zeros((rows.starts.size, rows.n_cams))
    out[rows.vstamp, rows.vcam] = np.add.reduceat((res * res).sum(1), rows.vstarts)
    return out


def _total(costs: np.ndarray) -> float:
    """Per timestamp over the cameras ascending, then over the timestamps in order."""
    per = np.zeros(costs.shape[0])
    for c in range(costs.shape[1]):
        per = per + costs[:, c]
    s = 0.0
    for v in per.tolist():
        s += v
    return s


def _normal_blocks(rows: _Rows, cams, X, P, segments):
    """The blocks of JtJ and Jtr as ``_lm.schur_step`` takes them with n = 6 (C - 1): U [N, 6, 6] (P_t - P_t), W [N, n, 6]
    (X - P_t), V [n, n] (X - X, block diagonal, summed over the timestamps in order), ga [n], gb [N, 6], the per-view costs
    [N, C].  ``segments`` = (first row, timestamp, camera) of every run of rows whose J_X products are summed by one reduction,
    ``_view_segments`` or ``_pair_segments``: numpy does not add a longer run in the same order, so a pair's sum and its two
    views' differ by rounding, and each definition keeps the bits it has.  None if a point is behind a camera."""
    ev = _evaluate(rows, cams, X, P, True)
    if ev is None:
        return None
    res, JX, JP = ev
    N, n = rows.starts.size, 6 * (rows.n_cams - 1)
    first, stamp, cam = segments
    U = np.add.reduceat(np.einsum("mai,maj->mij", JP, JP), rows.starts, 0)
    gb = np.add.reduceat(np.einsum("mai,ma->mi", JP, res), rows.starts, 0)
    Ws = np.add.reduceat(np.einsum("mai,maj->mij", JX, JP), first, 0)
    Vs = np.add.reduceat(np.einsum("mai,maj->mij", JX, JX), first, 0)
    gs = np.add.reduceat(np.einsum("mai,ma->mi", JX, res), first, 0)
    W, V, ga = np.zeros((N, n, 6)), np.zeros((n, n)), np.zeros(n)
    for i, (t, c) in enumerate(zip(stamp, cam)):               # timestamps in order
        if c == 0:
            continue
        s = slice(6 * (c - 1), 6 * c)
        W[t, s] = Ws[i]
        V[s, s] += Vs[i]
        ga[s] += gs[i]
    return U, W, V, ga, gb, _view_costs(rows, res)


def _refine(rows: _Rows, cams, X: np.ndarray, P: np.ndarray, segments):
    """Joint LM (module docstring, step 4) -> (status, X in the shape it came in, P, per-view costs [N, C], accepted steps,
    attempts)."""
    def trial_costs(g, p):
        ev = _evaluate(rows, cams, g, p, False)
        return _view_costs(rows, ev[0]) if ev is not None else None

    st, g, P, vc, iters, attempts = _lm.refine(X.ravel().copy(), P, lambda g, p: _normal_blocks(rows, cams, g, p, segments),
                                               trial_costs, _total, True, STEREO_MAX_ITER, STEREO_EPS)
    return st, g.reshape(X.shape), P, vc, iters, attempts


def _depth_margin(rows: _Rows, X: np.ndarray, P: np.ndarray) -> float:
    """The smallest depth of a row at (X, P), relative to its distance from its camera's centre."""
    Q = _points(rows, X.reshape(-1, 6), P)[1]
    return float((Q[:, 2] / np.linalg.norm(Q, axis=1)).min())


def _view_poses(keypoints_lists, masks, cams, board, pool_order):
    """Steps 1 and 2 for C cameras: ``keypoints_lists[c][t]`` and ``masks[c]`` (None, or per timestamp None or a bool array in the
    caller's row order) -> (view_status [T, C], view_points [T, C], poses [T, C, 6], and per [t][c] the object and the image
    points of a view that passed its checks, else None)."""
    C, B = len(cams), len(keypoints_lists[0])
    col_count, row_count, square_len = board
    n_ids = (col_count - 1) * (row_count - 1)
    view_status = np.full((B, C), PNP_OK, np.int32)
    view_points = np.zeros((B, C), np.int64)
    poses = np.zeros((B, C, 6))
    obj_l, img_l = [[None] * C for _ in range(B)], [[None] * C for _ in range(B)]
    for t in range(B):
        for c in range(C):
            kp, order = _pool_rows(keypoints_lists[c][t], pool_order)
            keep = np.ones(kp.shape[0], bool)
            if masks[c] is not None and masks[c][t] is not None:
                keep = np.asarray(masks[c][t]).astype(bool).ravel()
                if keep.size != kp.shape[0]:
                    raise ValueError(f"view ({c}, {t}) has {kp.shape[0]} rows but its mask {keep.size}")
            kp = kp[order][keep[order]]
            view_points[t, c] = kp.shape[0]
            if kp.shape[0] < 4:
                view_status[t, c] = PNP_TOO_FEW
                continue
            ids = kp[:, 2].astype(np.int64)
            if ids.min() < 0 or ids.max() >= n_ids:
                view_status[t, c] = PNP_BAD_ID
                continue
            obj_l[t][c] = pnp.object_points(ids, col_count, row_count, square_len)
            img_l[t][c] = kp[:, :2].astype(np.float32)
            st, pose = _model_of(cams[c])[0](obj_l[t][c], img_l[t][c], cams[c][0], cams[c][1])
            view_status[t, c] = st
            poses[t, c] = pose[:6]
    return view_status, view_points, poses, obj_l, img_l


def lower_median(values) -> float:
    """Element (n - 1) // 2 of the sorted values."""
    v = np.sort(np.asarray(values, np.float64))
    return float(v[(v.size - 1) // 2])


def _sine(R: np.ndarray) -> float:
    """The sine term of ``pnp._rvec_of`` at R: its branch switches at 1e-5."""
    return 0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)


def _rig_init(poses0: np.ndarray, poses1: np.ndarray):
    """Step 3 -> (status, X0 (6) or None, the sine term of ``_rvec_of`` at the orthonormalised median: its branch switches at
    1e-5)."""
    n = poses0.shape[0]
    Rt, Tt = np.empty((n, 3, 3)), np.empty((n, 3))
    for i in range(n):
        Rt[i] = _rodrigues(poses1[i, :3]) @ _rodrigues(poses0[i, :3]).T
        Tt[i] = poses1[i, 3:] - Rt[i] @ poses0[i, 3:]
    M = np.array([[lower_median(Rt[:, a, b]) for b in range(3)] for a in range(3)])
    T = np.array([lower_median(Tt[:, a]) for a in range(3)])
    ws, W = _jacobi(M.T @ M)                     # polar factor M (M^T M)^-1/2, as pnp._pose_of_homography
    if not ws.min() > 0:
        return STEREO_DEGENERATE, None, math.inf
    Q = M @ (W @ np.diag(1.0 / np.sqrt(ws)) @ W.T)
    X0 = np.r_[_rvec_of(Q), T]
    sine = _sine(Q)
    if not np.isfinite(X0).all():
        return STEREO_NONFINITE, None, sine
    return STEREO_OK, X0, sine


def essential_fundamental(R, T, camera0, camera1):
    """E = [T]x R and F = K1^-T E K0^-1, F scaled so that F[2, 2] = 1 where that entry is not zero (as cv2.stereoCalibrate)."""
    E = _skew(np.asarray(T, np.float64)) @ np.asarray(R, np.float64)
    F = np.linalg.inv(np.asarray(camera1, np.float64)).T @ E @ np.linalg.inv(np.asarray(camera0, np.float64))
    if F[2, 2] != 0.0:
        F = F / F[2, 2]
    return E, F


def _result(status, X, K0, K1, view_status, view_points, used, P, vc, iters, attempts, pinholes=True) -> StereoResult:
    B = view_status.shape[0]
    rv, tv, pr, vr = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B), np.zeros((B, 2))
    pp = np.zeros(B, np.int64)
    points = int(view_points[used].sum())          # the rows of the pairs found: reported whatever the status
    R, T, rvec, E, F, rms = np.zeros((3, 3)), np.zeros(3), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3)), 0.0
    if status == STEREO_OK:
        pp[used] = view_points[used].sum(1)
        rvec, T = X[:3].copy(), X[3:].copy()
        R = _rodrigues(rvec)
        E, F = essential_fundamental(R, T, K0, K1)
        rv[used], tv[used] = P[:, :3], P[:, 3:]
        vr[used] = np.sqrt(vc / view_points[used])
        pr[used] = np.sqrt(vc.sum(1) / pp[used])
        rms = math.sqrt(_total(vc) / points)
    return StereoResult(int(status), float(rms), R, T, rvec, E, F if pinholes else None, view_status.astype(np.int32), rv, tv, pr, pp, vr,
                        view_points.astype(np.int64), int(iters), int(attempts), int(used.size), points)


def _mask_pair(masks):
    if masks is None:
        return None, None
    if len(masks) != 2:
        raise ValueError("masks must be None or a pair (masks of camera 0, masks of camera 1), either of which may be None")
    return masks[0], masks[1]


def stereo_calibrate_host_full(keypoints_list0, keypoints_list1, col_count, row_count, square_len, camera0, dist0, camera1, dist1,
                               masks=None, pool_order=False, with_margin=False, models=None):
    """The definition (module docstring) -> ``StereoResult`` (with ``with_margin``: ``(result, margin)``).

    ``keypoints_list0`` / ``keypoints_list1``: per timestamp an array of [x, y, id] rows of camera 0 / 1 (an empty array for a
    timestamp the camera did not see).  Rows are taken in the order the corner pool holds them, as in
    ``pnp.solve_pnp_ransac_host_full``: id-sorted stably, or as they stand with ``pool_order=True``.  Object points are
    ``pnp.object_points`` (float32 -> float64), image points float32 -> float64.  ``masks``: None, or a pair (camera 0's,
    camera 1's) of None or per-timestamp bool arrays in the caller's row order (None: keep every row) that drop rows before the
    checks.  ``models``: None, or ("pinhole" | "fisheye", "pinhole" | "fisheye"): a fisheye camera is ``fisheye.py``'s model with
    k1..k4 (or None) as its ``dist``, its views are solved by ``fisheye._solve`` (a pixel outside the model: PNP_DEGENERATE) and
    its rows enter the joint solve through ``fisheye._project_q``; F, which relates pixels of two pinholes, is then None.  With
    None or two pinholes the result is what it has always been, bit for bit.  Nothing raises for unusable views; ValueError for
    a refused camera or lists of different lengths.

    ``with_margin``: the smallest relative distance of a discrete decision of steps 3 - 5 from its threshold: the sine term of
    the rig init's matrix -> vector conversion from its switch at 1e-5, and the depth of every used row at the solution from 0
    (relative to its distance from the camera centre)."""
    models = _models(models, 2)
    cams = _model_cameras((camera0, camera1), (dist0, dist1), models)
    pinholes = models is None or "fisheye" not in models
    lists = (keypoints_list0, keypoints_list1)
    if len(lists[0]) != len(lists[1]):
        raise ValueError(f"{len(lists[0])} views of camera 0 but {len(lists[1])} of camera 1")
    view_status, view_points, poses, obj_l, img_l = _view_poses(lists, _mask_pair(masks), cams, (col_count, row_count, square_len),
                                                                pool_order)
    used = np.flatnonzero((view_status == PNP_OK).all(1))

    def done(status, X=None, P=None, vc=None, iters=0, attempts=0, margin=math.inf):
        r = _result(status, X, cams[0][0], cams[1][0], view_status, view_points, used, P, vc, iters, attempts, pinholes)
        return (r, margin) if with_margin else r

    if not used.size:
        return done(STEREO_NO_PAIRS)
    st, X0, sine = _rig_init(poses[used, 0], poses[used, 1])
    margin = abs(sine - 1e-5) / 1e-5
    if st != STEREO_OK:
        return done(st, margin=margin)
    rows = _rows_of([(obj_l[t][0], img_l[t][0], obj_l[t][1], img_l[t][1]) for t in used])
    st, X, P, vc, iters, attempts = _refine(rows, cams, X0, poses[used, 0].copy(), _pair_segments(rows))
    if st == STEREO_OK and with_margin:
        margin = min(margin, _depth_margin(rows, X, P))
    return done(st, X, P, vc, iters, attempts, margin)


def _raise_like_cv2(r, col_count, row_count, what="stereo", empty_ok=False):
    """Raise where cv2's calibrations would, for a ``StereoResult`` or a ``RigResult``.  ``empty_ok``: a view without rows is a
    camera that did not see the board, not an error (the rig's rule)."""
    if (r.view_status == PNP_BAD_ID).any():
        raise _bad_id_error(col_count, row_count)
    unusable = r.view_status != PNP_OK
    if empty_ok:
        unusable &= r.view_points > 0
    bad = np.argwhere(unusable)
    if bad.size:
        t, c = (int(v) for v in bad[0])
        raise ValueError(f"view {t} of camera {c} cannot be used (status {int(r.view_status[t, c])})")
    if r.status != _lm.LM_OK:
        raise ValueError(f"{what} calibration failed (status {r.status})")


def stereo_calibrate_host(keypoints_list0, keypoints_list1, col_count, row_count, square_len, camera0, dist0, camera1, dist1,
                          masks=None, models=None):
    """cv2.stereoCalibrate's 9-tuple ``(rms, K0, d0, K1, d1, R, T (3, 1), E, F)`` with the intrinsics as they were given
    (CALIB_FIX_INTRINSIC).  Raises where cv2 would: ValueError for a view that cannot be used (too few rows, degenerate) or a failed
    calibration, IndexError for an id outside the board.  ``models`` as for the definition (F is then None)."""
    r = stereo_calibrate_host_full(keypoints_list0, keypoints_list1, col_count, row_count, square_len, camera0, dist0, camera1,
                                   dist1, masks, models=models)
    _raise_like_cv2(r, col_count, row_count)
    d0 = np.zeros((1, 0)) if dist0 is None else np.asarray(dist0, np.float64).reshape(1, -1).copy()
    d1 = np.zeros((1, 0)) if dist1 is None else np.asarray(dist1, np.float64).reshape(1, -1).copy()
    return (r.rms, _camera(camera0).copy(), d0, _camera(camera1).copy(), d1, r.R, r.T.reshape(3, 1).copy(), r.E, r.F)


# ------------------------------------------------------------------------------------------------ the device solver

def workspace_bytes(batch: int, pool0: int, pool1: int) -> int:
    """Bytes of device workspace ``stereo_calibrate_pool`` needs."""
    from . import _lib
    n = int(_lib.lib().dcx_stereo_calibrate_workspace_bytes(int(batch), int(pool0), int(pool1)))
    if n == 0:
        raise ValueError("batch >= 1 and pool0, pool1 >= 0 are required")
    return n


def _device_masks(masks, pools, dev):
    """Every mask that is given must be a contiguous uint8 tensor on ``dev`` of at least its pool's size (ValueError)."""
    import torch
    for c, (m, pool) in enumerate(zip(masks, pools)):
        if m is not None:
            _dev.tensor(m, dev, torch.uint8, (pool,), f"mask {c} must be a contiguous uint8 tensor of at least {pool} values on {dev}",
                        "min")


def _outputs(batch, n_cams, dev):
    """-> what a joint solve writes on the device: view status int32 [B, C], pose float64 [B, POSE_WORDS], info float64 [B, C, 2]."""
    import torch
    return (torch.empty((batch, n_cams), dtype=torch.int32, device=dev),
            torch.empty((batch, pnp.POSE_WORDS), dtype=torch.float64, device=dev),
            torch.empty((batch, n_cams, 2), dtype=torch.float64, device=dev))


def _call(entry, head, tags, tail):
    """``dcx_<entry>_pool(*head, *tail, stream)``, or with ``tags``, the cameras' models as the C entry takes them,
    ``dcx_<entry>_models_pool(*head, *tags, *tail, stream)``."""
    from . import _lib
    name = f"dcx_{entry}_pool" if tags is None else f"dcx_{entry}_models_pool"
    _lib.check(getattr(_lib.lib(), name)(*head, *(tags or ()), *tail, _lib.current_stream()), name)


def _unpack(st, pose, info):
    """``_outputs`` after the call -> host arrays: view status [B, C], rvecs, tvecs [B, 3], the timestamps' rms and rows [B], the
    views' rms and rows [B, C]."""
    st_h, pose_h, info_h = st.cpu().numpy(), pose.cpu().numpy(), info.cpu().numpy()
    return (st_h.astype(np.int32), pose_h[:, 0:3].copy(), pose_h[:, 3:6].copy(), pose_h[:, 6].copy(), pose_h[:, 7].astype(np.int64),
            info_h[:, :, 0].copy(), info_h[:, :, 1].astype(np.int64))


def stereo_calibrate_pool(packed0, packed1, batch: int, pool0: int, pool1: int, refined: bool, col_count, row_count, square_len,
                          camera0, dist0, camera1, dist1, masks=None, models=None) -> StereoResult:
    """The rig of two cameras from two ``infer_batch_device`` results of ``batch`` frames each, read in place from the two corner
    pools (the conventions of ``pnp.solve_pnp_pool``; frame t of ``packed0`` and frame t of ``packed1`` were taken at the same
    instant).  ``masks``: None, or a pair of None / contiguous uint8 device tensors of at least ``pool0`` / ``pool1`` values by
    SLOT, the ``inliers`` that ``pnp.solve_pnp_ransac_pool`` and ``calib.calibrate_charuco_ransac_pool`` write: rows with 0 are
    dropped before the checks.  With a mask the slot ranges of that pool's views must not overlap (DcxError).  ``models``: None
    (``dcx_stereo_calibrate_pool``) or the two cameras' models (``dcx_stereo_calibrate_models_pool``).  The call
    synchronises the current stream (the rig init's median and the LM loop's state word are read on the host) and cannot be
    captured in a graph."""
    import torch
    from . import _lib
    dev = packed0.device
    if packed1.device != dev:
        raise ValueError("the two pools must be on one device")
    p0, p1 = _pool_ptrs(packed0, batch, pool0, refined), _pool_ptrs(packed1, batch, pool1, refined)
    mk = _mask_pair(masks)
    _device_masks(mk, (pool0, pool1), dev)
    models = _models(models, 2)
    cam0, d0, n0 = _model_args(camera0, dist0, models and models[0])
    cam1, d1, n1 = _model_args(camera1, dist1, models and models[1])
    st, pose, info = _outputs(batch, 2, dev)
    nbytes = workspace_bytes(batch, pool0, pool1)
    ws = _dev.workspace(None, dev, nbytes)
    res = (_ctypes.c_double * RESULT_WORDS)()
    head = (*p0, _lib.ptr(mk[0]), *p1, _lib.ptr(mk[1]), int(batch), int(pool0), int(pool1), int(col_count), int(row_count),
            float(square_len), cam0, d0, n0, cam1, d1, n1)
    tail = (ws.data_ptr(), nbytes, st.data_ptr(), pose.data_ptr(), info.data_ptr(), res)
    with torch.cuda.device(dev):
        _call("stereo_calibrate", head, models and [MODELS.index(m) for m in models], tail)
        view_status, rvecs, tvecs, pair_rms, pair_points, view_rms, view_points = _unpack(st, pose, info)
    r = np.array(res[:], np.float64)
    status = int(r[11])
    R, E, F = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
    if status == STEREO_OK:
        R = _rodrigues(r[0:3])
        E, F = essential_fundamental(R, r[3:6], _camera(camera0), _camera(camera1))
    if models is not None and "fisheye" in models:
        F = None
    return StereoResult(status, float(r[6]), R, r[3:6].copy(), r[0:3].copy(), E, F, view_status, rvecs, tvecs, pair_rms, pair_points,
                        view_rms, view_points, int(r[7]), int(r[8]), int(r[9]), int(r[10]))


def _slot_mask(keypoints_list, masks, pool, dev):
    """Per-view masks in the caller's row order -> a uint8 device tensor by slot of the pool ``pack_keypoints`` lays (stable id sort)."""
    import torch
    out = np.ones(pool, np.uint8)
    s = 0
    for t, kp in enumerate(keypoints_list):
        kp, order = _pool_rows(kp)
        n = kp.shape[0]
        if masks[t] is not None:
            m = np.asarray(masks[t]).astype(bool).ravel()
            if m.size != n:
                raise ValueError(f"view {t} has {n} rows but its mask {m.size}")
            out[s:s + n] = m[order]
        s += n
    return torch.from_numpy(out).to(dev)


def _upload(keypoints_lists, masks, dev):
    """The ``*_device`` calls' views, one list per camera, and ``masks`` (per camera None or its per-view masks) -> (per camera
    ``pack_keypoints``' (packed, batch, pool), per camera None or its mask by slot).  ValueError for no views."""
    if len(keypoints_lists[0]) == 0:
        raise ValueError("no views")
    packs = [pack_keypoints(k, dev) for k in keypoints_lists]
    return packs, [None if m is None else _slot_mask(k, m, p[2], dev) for k, m, p in zip(keypoints_lists, masks, packs)]


def stereo_calibrate_device(keypoints_list0: Sequence, keypoints_list1: Sequence, col_count, row_count, square_len, camera0, dist0,
                            camera1, dist1, masks=None, device="cuda", models=None) -> StereoResult:
    """``stereo_calibrate_host_full`` on the GPU from ``infer_image``-format keypoint arrays ([x, y, id] rows; one list per
    camera, equally long) -> ``StereoResult``.  ``masks`` and ``models`` as for the host definition.  IndexError if a view with >= 4 rows carries
    an id outside the board."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    models = _models(models, 2)
    _model_args(camera0, dist0, models and models[0])         # ValueError before anything is uploaded
    _model_args(camera1, dist1, models and models[1])
    if len(keypoints_list0) != len(keypoints_list1):
        raise ValueError(f"{len(keypoints_list0)} views of camera 0 but {len(keypoints_list1)} of camera 1")
    ((packed0, b, pool0), (packed1, _, pool1)), dm = _upload((keypoints_list0, keypoints_list1), _mask_pair(masks), dev)
    with torch.cuda.device(dev):
        r = stereo_calibrate_pool(packed0, packed1, b, pool0, pool1, True, col_count, row_count, square_len, camera0, dist0,
                                  camera1, dist1, None if masks is None else tuple(dm), models)
    return _no_bad_id(r, col_count, row_count)


# ------------------------------------------------------------------------------------------------ how well the pair is determined
# ``rig.rig_uncertainty_*`` with two cameras: the same functions and the same entry (csrc/dcx_rig_cov.hip with n_cams = 2), so the
# results are those calls' bit for bit.  (``rig`` imports this module, so it is imported at the call.)

def stereo_uncertainty_host(keypoints_list0, keypoints_list1, col_count, row_count, square_len, camera0, dist0, camera1, dist1,
                            result_or_model, masks=None, models=None):
    """``rig.rig_uncertainty_host`` on the two lists -> its ``RigUncertainty``: the covariance of X_1 = (rvec, T) (``cov_rig``
    6 x 6) and of every used pair's board pose, given the two camera models.  ``result_or_model``: a ``StereoResult`` (ValueError
    unless ``STEREO_OK``; it stands for X_1, its P_t and its view statuses) or that function's tuple with C = 2.  ``masks`` and
    ``models`` as for ``stereo_calibrate_host_full``."""
    from . import rig
    return rig.rig_uncertainty_host((keypoints_list0, keypoints_list1), col_count, row_count, square_len, (camera0, camera1),
                                    (dist0, dist1), result_or_model, None if masks is None else list(_mask_pair(masks)), models)


def stereo_uncertainty_pool(packed0, packed1, batch: int, pool0: int, pool1: int, refined: bool, col_count, row_count, square_len,
                            camera0, dist0, camera1, dist1, result_or_model, masks=None, models=None, workspace=None, out=None):
    """``rig.rig_uncertainty_pools`` on the two pools of ``stereo_calibrate_pool`` -> its two device tensors
    (``rig.unpack_rig_uncertainty`` makes a ``RigUncertainty`` of them).  No synchronisation; capturable as that call is."""
    from . import rig
    return rig.rig_uncertainty_pools([packed0, packed1], batch, [pool0, pool1], refined, col_count, row_count, square_len,
                                     (camera0, camera1), (dist0, dist1), result_or_model,
                                     None if masks is None else list(_mask_pair(masks)), models, workspace, out)


def stereo_uncertainty_device(keypoints_list0: Sequence, keypoints_list1: Sequence, col_count, row_count, square_len, camera0, dist0,
                              camera1, dist1, result_or_model, masks=None, device="cuda", models=None):
    """``stereo_uncertainty_host`` on the GPU from ``infer_image``-format keypoint arrays -> ``RigUncertainty``."""
    from . import rig
    return rig.rig_uncertainty_device((keypoints_list0, keypoints_list1), col_count, row_count, square_len, (camera0, camera1),
                                      (dist0, dist1), result_or_model, None if masks is None else list(_mask_pair(masks)), device,
                                      models)
