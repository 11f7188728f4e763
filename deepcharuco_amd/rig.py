"""Joint extrinsic calibration of a rig of 2 to 8 rigidly mounted cameras from their ChArUco corners, on the host and on the GPU:
``stereo.py``'s solve with a 6 (C - 1) shared block in place of its 6.

C cameras, each with a known ``(camera_matrix, dist_coeffs)`` (none, 4, 5 or 8 coefficients; the models may differ), see the same
board at the same instants: view t of every camera belongs to timestamp t, and a camera that did not see the board then has an
empty view.  Every corner carries its id, so the views of a timestamp need not share a single id, and two cameras constrain each
other through any timestamp both of them saw.  Camera 0 is the reference.  Unknowns: X_c = (rvec, T) for c = 1 .. C - 1 in cv2's
convention, q_c = R_c q_0 + T_c for a point q_0 in camera 0's frame, and the board's pose P_t in camera 0's frame for every
timestamp that is used.  Cost: the squared pixel distance of pi_c(X_c P_t o) to the rows of view (c, t) (X_0 is the identity),
over every usable view of every used timestamp.  Steps, all in float64:

1. per-view checks and poses, exactly ``stereo.py``'s steps 1 - 2: an optional mask per view drops rows first; then fewer than 4
   rows -> TOO_FEW, an id outside the board -> BAD_ID (from a pool also TRUNCATED); ``pnp._solve`` with that camera's model.  A
   view is USABLE if it is PNP_OK.  A timestamp is USED if at least two of its views are usable, whichever cameras they are.  A
   usable view that is alone at its timestamp is reported with its status and row count and takes no part;
2. the camera graph and the initial rig.  Cameras a and c SHARE a timestamp if both of their views are usable there (it is then
   used).  Camera 0 is placed first.  Then, in the order they were placed, every placed camera a takes, in ascending order, each
   camera c not placed yet that shares at least one timestamp with it: c gets the parent a and is placed (breadth first).  The
   edge Z_{a -> c} is ``stereo._rig_init`` over the timestamps a and c share, in order, with a in camera 0's role: the
   element-wise LOWER median of R_c,t R_a,t^T (9) and of t_c,t - R_t t_a,t (3), the median matrix's polar factor, ``_rvec_of``.
   X_c = Z for a child of camera 0, unchanged; otherwise X_c = Z o X_a: rvec_c = ``_rvec_of``(R(Z) R(X_a)), T_c = R(Z) T_a + T_Z.
   A camera that is never placed -> RIG_DISCONNECTED; no used timestamp at all -> RIG_NO_STAMPS (tested first).  ``parents``
   holds the tree (-1 for camera 0 and for a camera that was not placed);
3. the initial board poses: with c the lowest-numbered usable camera of timestamp t, P_t = X_c^-1 o pose_{c,t}:
   rvec = ``_rvec_of``(R_c^T R(pose)), t = R_c^T (t_pose - T_c); for c = 0 the view's own pose, unchanged;
4. joint Levenberg-Marquardt over all X_c (6 (C - 1) parameters, camera 1's first) and every used P_t (6 each) by ``_lm.refine``
   with stereo's rules: a step forced with a point behind its camera ends the solve, at most 30 accepted steps, stop at
   |dp| / |p| < DBL_EPSILON over all 6 (C - 1) + 6 N parameters, a point behind its camera is a rejection.  Jacobians are analytic
   as ``stereo._evaluate`` has them: a row of camera c >= 1 touches X_c's six columns only, a row of camera 0 none.  Each step by
   block elimination (``_lm.schur_step``): the 6 x 6 blocks U_t are eliminated and one 6 (C - 1)-square system remains, solved by
   Cholesky.  The order of every sum: U_t, g_b,t and a timestamp's cost over its usable cameras ascending, each camera's rows in
   pool order; W_{t,c} over the rows of view (c, t) in pool order; V (block diagonal, one 6 x 6 per camera) and g_a over the
   timestamps in order; the total cost over the timestamps in order;
5. outputs (``RigResult``): per camera R, T, rvec (camera 0: identity, zero, zero), rms = sqrt(sum |r|^2 / points used), the
   tree, per view status, rows and rms, per timestamp P_t, rms and rows; the continuous outputs and the per-timestamp rows are
   zero unless the status is RIG_OK (P_t also unless the timestamp was used); timestamps used and points used whatever the status.

``rig_calibrate_host_full`` is the readable definition and the test pin; ``rig_calibrate_pools`` / ``rig_calibrate_device`` run the
same steps on the GPU (csrc/dcx_rig.hip).  The two agree to rounding (summation order), not bit for bit.  With C = 2 the steps
are ``stereo.py``'s, and the result its result to rounding: V and g_a are summed in the same order, the cost per timestamp is
added up camera by camera.

``models`` (the last keyword of the four entry points): None, or per camera ``"pinhole"`` or ``"fisheye"``.  A fisheye camera is
``fisheye.py``'s model with its four coefficients k1..k4 (or None) in ``dists``: its views are solved by ``fisheye._solve`` (a view
with a pixel outside the model is PNP_DEGENERATE, and then not usable) and its rows enter step 4 through ``fisheye._project_q``.
Nothing else changes: the steps above never look inside a camera.  With None, and with every camera a pinhole, the result is
what it has always been, bit for bit.

What it gives over C - 1 stereo solves: one consistent rig from one call, and cameras that never see the board together with
camera 0.  Where every camera shares views with camera 0 it is not measurably more accurate than the pairwise solves.
With the rig solved, ``rig_pose_host_full`` / ``rig_pose_pools`` / ``rig_pose_device`` (second half of this module) find the board's
pose per timestamp from every camera's rows, the rig held fixed, and ``rig_uncertainty_host`` / ``rig_uncertainty_pools`` /
``rig_uncertainty_device`` (last part) say how well the rig is determined: the covariances of the X_c and of the P_t, given the
camera models (csrc/dcx_rig_cov.hip, without a host loop or a synchronisation).
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import NamedTuple, Sequence

import numpy as np

from . import _dev, _lm
from .calib import COV_NO_DOF, COV_NO_VIEWS, COV_OK, COV_SINGULAR, COV_POSE_WORDS, _device_or_upload, _no_bad_id
from .corner_pool import _pool_rows
from .pnp import (LM_EPS, LM_MAX_ITER, LM_STATUS, PNP_DEGENERATE, PNP_OK, PNP_TOO_FEW, PNP_TRUNCATED, _bad_id_error, _camera,
                  _pool_ptrs, _rodrigues, _rvec_of, object_points)
# every step that does not depend on the number of cameras is stereo.py's, kept once
from .stereo import (MODELS, STEREO_EPS, STEREO_MAX_ITER, _call, _depth_margin, _device_masks, _evaluate, _model_args, _model_cameras,
                     _models, _normal_blocks, _outputs, _raise_like_cv2, _refine, _rig_init, _sine, _total, _unpack, _upload, _view_poses,
                     _view_segments, essential_fundamental)
from .stereo import _rig_rows as _rows_of

# overall status (include/deepcharuco_amd.h); per-view statuses are pnp's PNP_*
RIG_OK, RIG_NO_STAMPS, RIG_DEGENERATE, RIG_NONFINITE = _lm.LM_OK, _lm.LM_NO_UNITS, _lm.LM_DEGENERATE, _lm.LM_NONFINITE
RIG_DISCONNECTED = 4
RIG_MAX_CAMERAS = 8
RIG_MAX_ITER, RIG_EPS = STEREO_MAX_ITER, STEREO_EPS      # step 4's rules are stereo's: ``stereo._refine`` runs both
RESULT_HEAD = 8                # h_result of dcx_rig_calibrate_pool: 8 words, then X_1 .. X_{C-1}
REDUCE_CHUNK, REDUCE_SLICES = 16, 16   # csrc/dcx_rig.hip's kChunk, kSlices: the two fan-ins of the per-attempt reduction

__all__ = ["RigResult", "rig_calibrate_host", "rig_calibrate_host_full", "rig_calibrate_pools", "rig_calibrate_device", "rig_pair",
           "workspace_bytes", "RIG_OK", "RIG_NO_STAMPS", "RIG_DEGENERATE", "RIG_NONFINITE", "RIG_DISCONNECTED",
           "RigPoseResult", "rig_pose_host", "rig_pose_host_full", "rig_pose_pools", "unpack_rig_poses", "rig_pose_device",
           "rig_pose_workspace_bytes", "RigUncertainty", "rig_uncertainty_host", "rig_uncertainty_pools", "unpack_rig_uncertainty",
           "rig_uncertainty_device", "rig_uncertainty_workspace_bytes"]


class RigResult(NamedTuple):
    status: int                  # RIG_*
    rms: float                   # sqrt(sum |r|^2 / points used) over every used row
    R: np.ndarray                # [C, 3, 3]: q_c = R[c] q_0 + T[c]; R[0] the identity
    T: np.ndarray                # [C, 3]
    rvec: np.ndarray             # [C, 3] Rodrigues vectors of R
    parents: np.ndarray          # int32 [C] the initialisation's tree; -1 for camera 0 and for a camera that was not placed
    view_status: np.ndarray      # int32 [T, C], pnp.PNP_* per view
    view_points: np.ndarray      # int64 [T, C] rows the view brings (after its mask), used or not
    view_rms: np.ndarray         # [T, C] rms of the view at the solution; zero unless it took part
    rvecs: np.ndarray            # [T, 3] the board's pose P_t in camera 0's frame; zeros unless the timestamp was used
    tvecs: np.ndarray            # [T, 3]
    stamp_rms: np.ndarray        # [T] rms over the usable views of the timestamp at the solution (px)
    stamp_points: np.ndarray     # int64 [T] rows of the usable views of a used timestamp; zeros unless RIG_OK
    iterations: int              # accepted LM steps
    attempts: int                # LM trial steps (accepted + rejected)
    stamps_used: int             # the timestamps found and their rows, whatever the status
    points_used: int


# ------------------------------------------------------------------------------------------------ the fp64 steps

def _tree(usable: np.ndarray):
    """Step 2's graph walk over usable [T, C] (bool) -> (parents [C] with -1 for camera 0 and the cameras not placed, the placed
    cameras in placement order)."""
    C = usable.shape[1]
    share = (usable.astype(np.int64).T @ usable.astype(np.int64)) > 0
    parents, order, placed = np.full(C, -1, np.int32), [0], {0}
    i = 0
    while i < len(order):
        a = order[i]
        for c in range(C):
            if c not in placed and share[a, c]:
                parents[c] = a
                placed.add(c)
                order.append(c)
        i += 1
    return parents, order


def _seed_pose(x, pose):
    """X_c^-1 o pose, a view's own pose taken into camera 0's frame (step 3 of the calibration and of the rig pose solve) -> (P, the
    sine term of its ``_rvec_of``)."""
    Rc = _rodrigues(x[:3])
    R = Rc.T @ _rodrigues(pose[:3])
    return np.r_[_rvec_of(R), Rc.T @ (pose[3:] - x[3:])], _sine(R)


def _initial_rig(usable, poses, parents, order):
    """Steps 2 (the edges and their composition) and 3 -> (status, X [C - 1, 6], P [N, 6], the smallest relative distance of a sine
    term of ``_rvec_of`` from its switch)."""
    C = usable.shape[1]
    X, margin = np.zeros((C, 6)), math.inf
    for c in order[1:]:
        a = int(parents[c])
        ts = np.flatnonzero(usable[:, a] & usable[:, c])
        st, Z, sine = _rig_init(poses[ts, a], poses[ts, c])
        margin = min(margin, abs(sine - 1e-5) / 1e-5)
        if st != RIG_OK:
            return st, None, None, margin
        if a == 0:
            X[c] = Z
        else:
            RZ = _rodrigues(Z[:3])
            Rc = RZ @ _rodrigues(X[a, :3])
            margin = min(margin, abs(_sine(Rc) - 1e-5) / 1e-5)
            X[c] = np.r_[_rvec_of(Rc), RZ @ X[a, 3:] + Z[3:]]
        if not np.isfinite(X[c]).all():
            return RIG_NONFINITE, None, None, margin
    used = np.flatnonzero(usable.sum(1) >= 2)
    P = np.zeros((used.size, 6))
    for i, t in enumerate(used):
        c = int(np.flatnonzero(usable[t])[0])
        if c == 0:
            P[i] = poses[t, 0]
        else:
            P[i], sine = _seed_pose(X[c], poses[t, c])
            margin = min(margin, abs(sine - 1e-5) / 1e-5)
    return RIG_OK, X[1:], P, margin


def _result(status, X, parents, view_status, view_points, usable, used, P, vc, iters, attempts) -> RigResult:
    B, C = view_status.shape
    part = usable & (usable.sum(1) >= 2)[:, None]          # the views that take part
    points = int(view_points[part].sum())                   # reported whatever the status
    R, T, rvec, rms = np.zeros((C, 3, 3)), np.zeros((C, 3)), np.zeros((C, 3)), 0.0
    rv, tv, sr, vr, sp = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B), np.zeros((B, C)), np.zeros(B, np.int64)
    if status == RIG_OK:
        rvec[1:], T[1:] = X[:, :3], X[:, 3:]
        R = np.stack([_rodrigues(r) for r in rvec])
        sp[used] = (view_points * part)[used].sum(1)
        rv[used], tv[used] = P[:, :3], P[:, 3:]
        n = np.where(part[used], view_points[used], 1)
        vr[used] = np.sqrt(vc / n)
        per = np.zeros(used.size)
        for c in range(C):
            per = per + vc[:, c]
        sr[used] = np.sqrt(per / sp[used])
        rms = math.sqrt(_total(vc) / points)
    return RigResult(int(status), float(rms), R, T, rvec, np.asarray(parents, np.int32), view_status.astype(np.int32),
                     view_points.astype(np.int64), vr, rv, tv, sr, sp, int(iters), int(attempts), int(used.size), points)


def _cameras(cameras, dists, models=None):
    if dists is None:
        dists = [None] * len(cameras)
    if not 2 <= len(cameras) <= RIG_MAX_CAMERAS or len(dists) != len(cameras):
        raise ValueError(f"2 to {RIG_MAX_CAMERAS} cameras and as many distortion models are required")
    return _model_cameras(cameras, dists, _models(models, len(cameras))), list(dists)


def _mask_lists(masks, n_cams):
    if masks is None:
        return [None] * n_cams
    if len(masks) != n_cams:
        raise ValueError("masks must be None or one entry per camera, each None or that camera's masks")
    return list(masks)


def rig_calibrate_host_full(keypoints_lists, col_count, row_count, square_len, cameras, dists, masks=None, pool_order=False,
                            with_margin=False, models=None):
    """The definition (module docstring) -> ``RigResult`` (with ``with_margin``: ``(result, margin)``).

    ``keypoints_lists[c][t]``: the [x, y, id] rows of camera c at timestamp t (an empty array where the camera did not see the
    board); every camera's list is equally long.  Rows are taken in the order the corner pool holds them: id-sorted stably, or as
    they stand with ``pool_order=True``.  ``cameras`` / ``dists``: per camera its matrix and coefficients (``dists`` or an entry
    of it may be None).  ``masks``: None, or per camera None or per-timestamp bool arrays in the caller's row order (None: keep
    every row) that drop rows before the checks.  ``models``: None or per camera "pinhole" / "fisheye" (module docstring).
    Nothing raises for unusable views; ValueError for a refused camera, fewer than
    2 or more than 8 cameras, or lists of different lengths.

    ``with_margin``: the smallest relative distance of a discrete decision of steps 2 - 5 from its threshold: the sine term of
    every ``_rvec_of`` of the initialisation (every tree edge, every composition) from its switch at 1e-5, and the depth of every
    used row at the solution from 0 (relative to its distance from the camera centre)."""
    cams, _ = _cameras(cameras, dists, models)
    C = len(cams)
    if len(keypoints_lists) != C:
        raise ValueError(f"{len(keypoints_lists)} keypoint lists for {C} cameras")
    B = len(keypoints_lists[0])
    for c in range(C):
        if len(keypoints_lists[c]) != B:
            raise ValueError(f"{B} views of camera 0 but {len(keypoints_lists[c])} of camera {c}")
    view_status, view_points, poses, obj_l, img_l = _view_poses(keypoints_lists, _mask_lists(masks, C), cams,
                                                                (col_count, row_count, square_len), pool_order)
    usable = view_status == PNP_OK
    used = np.flatnonzero(usable.sum(1) >= 2)
    parents = np.full(C, -1, np.int32)

    def done(status, X=None, P=None, vc=None, iters=0, attempts=0, margin=math.inf):
        r = _result(status, X, parents, view_status, view_points, usable, used, P, vc, iters, attempts)
        return (r, margin) if with_margin else r

    if not used.size:
        return done(RIG_NO_STAMPS)
    parents, order = _tree(usable)
    if len(order) < C:
        return done(RIG_DISCONNECTED)
    st, X0, P0, margin = _initial_rig(usable, poses, parents, order)
    if st != RIG_OK:
        return done(st, margin=margin)
    rows = _rows_of([[(c, obj_l[t][c], img_l[t][c]) for c in range(C) if usable[t, c]] for t in used], C)
    st, X, P, vc, iters, attempts = _refine(rows, cams, X0, P0, _view_segments(rows))
    if st == RIG_OK and with_margin:
        margin = min(margin, _depth_margin(rows, X, P))
    return done(st, X, P, vc, iters, attempts, margin)


def rig_calibrate_host(keypoints_lists, col_count, row_count, square_len, cameras, dists, masks=None, models=None):
    """``(rms, R [C, 3, 3], T [C, 3, 1])`` with q_c = R[c] q_0 + T[c].  Raises where cv2's calibrations would: ValueError for a view
    that has rows and cannot be used (too few, degenerate) or a failed calibration (no timestamp with two views, a camera that
    shares no view with the others), IndexError for an id outside the board.  An empty view is not an error."""
    r = rig_calibrate_host_full(keypoints_lists, col_count, row_count, square_len, cameras, dists, masks, models=models)
    _raise_like_cv2(r, col_count, row_count, "rig", empty_ok=True)
    return r.rms, r.R, r.T.reshape(-1, 3, 1).copy()


def rig_pair(result: RigResult, a: int, b: int, camera_a, camera_b):
    """The stereo pair (a, b) of a solved rig -> ``(R, T, E, F)`` with q_b = R q_a + T, from X_b o X_a^-1, and
    ``stereo.essential_fundamental`` with the two camera matrices: what ``rectify.stereo_rectify_host`` takes.  F relates pixels
    of two PINHOLE cameras (undistorted ones): between cameras of which one is a fisheye it means nothing; R, T and E hold for any
    pair."""
    if result.status != RIG_OK:
        raise ValueError(f"the rig was not solved (status {result.status})")
    C = result.R.shape[0]
    if not (0 <= a < C and 0 <= b < C and a != b):
        raise ValueError(f"two different cameras of 0 .. {C - 1} are required")
    R = result.R[b] @ result.R[a].T
    T = result.T[b] - R @ result.T[a]
    E, F = essential_fundamental(R, T, _camera(camera_a), _camera(camera_b))
    return R, T, E, F


# ------------------------------------------------------------------------------------------------ the device solver

class _RigCamera(_ctypes.Structure):
    """DcxRigCamera of include/deepcharuco_amd.h."""
    _fields_ = [("d_counts", _ctypes.c_void_p), ("d_starts", _ctypes.c_void_p), ("d_rows", _ctypes.c_void_p),
                ("d_xy", _ctypes.c_void_p), ("pool", _ctypes.c_int), ("d_mask", _ctypes.c_void_p),
                ("camera9", _ctypes.c_double * 9), ("dist", _ctypes.c_double * 8), ("n_dist", _ctypes.c_int)]


def workspace_bytes(n_cams: int, batch: int, pools) -> int:
    """Bytes of device workspace ``rig_calibrate_pools`` needs."""
    from . import _lib
    pools = [int(p) for p in pools]
    if len(pools) != int(n_cams):
        raise ValueError("one pool size per camera is required")
    n = int(_lib.lib().dcx_rig_calibrate_workspace_bytes(int(n_cams), int(batch), (_ctypes.c_int * len(pools))(*pools)))
    if n == 0:
        raise ValueError(f"2 to {RIG_MAX_CAMERAS} cameras, batch >= 1 and pools >= 0 are required")
    return n


def rig_calibrate_pools(packed_list, batch: int, pools, refined: bool, col_count, row_count, square_len, cameras, dists,
                        masks=None, models=None) -> RigResult:
    """The rig of C cameras from C ``infer_batch_device`` results of ``batch`` frames each, read in place from the C corner pools
    (the conventions of ``pnp.solve_pnp_pool``; frame t of every pool was taken at the same instant).  ``pools``: the pool size per
    camera.  ``masks``: None, or per camera None or a contiguous uint8 device tensor of at least that pool's size by SLOT, the
    ``inliers`` that ``pnp.solve_pnp_ransac_pool`` and ``calib.calibrate_charuco_ransac_pool`` write: rows with 0 are dropped
    before the checks.  With a mask the slot ranges of that pool's views must not overlap (DcxError).  ``models``: None
    (``dcx_rig_calibrate_pool``) or per camera "pinhole" / "fisheye" (``dcx_rig_calibrate_models_pool``).  The call synchronises the
    current stream (the tree, the medians and the LM loop's state word are read on the host) and cannot be captured in a graph."""
    import torch
    from . import _lib
    cams, dists = _cameras(cameras, dists, models)
    C = len(cams)
    models = _models(models, C)
    pools = [int(p) for p in pools]
    if len(packed_list) != C or len(pools) != C:
        raise ValueError(f"{C} cameras need {C} pools and {C} pool sizes")
    dev = packed_list[0].device
    if any(p.device != dev for p in packed_list):
        raise ValueError("the pools must be on one device")
    mk = _mask_lists(masks, C)
    _device_masks(mk, pools, dev)
    table = (_RigCamera * C)()
    for c in range(C):
        counts_p, starts_p, rows_p, xy_p = _pool_ptrs(packed_list[c], batch, pools[c], refined)
        cam9, d8, nd = _model_args(cameras[c], dists[c], models and models[c])
        table[c] = _RigCamera(counts_p, starts_p, rows_p, xy_p, pools[c], _lib.ptr(mk[c]), cam9, d8, nd)
    st, pose, info = _outputs(batch, C, dev)
    nbytes = workspace_bytes(C, batch, pools)
    ws = _dev.workspace(None, dev, nbytes)
    res = (_ctypes.c_double * (RESULT_HEAD + 6 * (C - 1)))()
    par = (_ctypes.c_int32 * C)()
    tail = (int(batch), int(col_count), int(row_count), float(square_len), ws.data_ptr(), nbytes, st.data_ptr(), pose.data_ptr(),
            info.data_ptr(), par, res)
    with torch.cuda.device(dev):
        _call("rig_calibrate", (C, table), models and [(_ctypes.c_int * C)(*(MODELS.index(m) for m in models))], tail)
        view_status, rvecs, tvecs, stamp_rms, stamp_points, view_rms, view_points = _unpack(st, pose, info)
    r = np.array(res[:], np.float64)
    status = int(r[5])
    R, T, rvec = np.zeros((C, 3, 3)), np.zeros((C, 3)), np.zeros((C, 3))
    if status == RIG_OK:
        X = r[RESULT_HEAD:].reshape(C - 1, 6)
        rvec[1:], T[1:] = X[:, :3], X[:, 3:]
        R = np.stack([_rodrigues(v) for v in rvec])
    return RigResult(status, float(r[0]), R, T, rvec, np.array(par[:], np.int32), view_status, view_points, view_rms, rvecs, tvecs,
                     stamp_rms, stamp_points, int(r[1]), int(r[2]), int(r[3]), int(r[4]))


def rig_calibrate_device(keypoints_lists: Sequence, col_count, row_count, square_len, cameras, dists, masks=None,
                         device="cuda", models=None) -> RigResult:
    """``rig_calibrate_host_full`` on the GPU from ``infer_image``-format keypoint arrays ([x, y, id] rows; one list per camera,
    equally long) -> ``RigResult``.  ``masks`` and ``models`` as for the host definition.  IndexError if a view with >= 4 rows carries an id
    outside the board."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    cams, dists = _cameras(cameras, dists, models)            # ValueError before anything is uploaded
    C = len(cams)
    if len(keypoints_lists) != C:
        raise ValueError(f"{len(keypoints_lists)} keypoint lists for {C} cameras")
    B = len(keypoints_lists[0])
    if any(len(k) != B for k in keypoints_lists):
        raise ValueError("every camera needs as many views as camera 0")
    packs, dm = _upload(keypoints_lists, _mask_lists(masks, C), dev)
    with torch.cuda.device(dev):
        r = rig_calibrate_pools([p[0] for p in packs], B, [p[2] for p in packs], True, col_count, row_count, square_len, cameras,
                                dists, None if masks is None else dm, models)
    return _no_bad_id(r, col_count, row_count)


# ------------------------------------------------------------------------------------------------ rig pose: one board pose from every camera
# With the rig held fixed (X_c known, from a ``RigResult`` or as R, T), the board's pose P_t in camera 0's frame from everything
# the C cameras saw at instant t.  Every timestamp is solved on its own.  Steps, all in float64:
#
# 1. per view (t, c): ``stereo._view_poses``, unchanged: the status, the rows after the mask, the view's own pose.  ``view_status`` and
#    ``view_points`` are what ``rig_calibrate_host_full`` reports for the same input;
# 2. which rows CONTRIBUTE, judged on the rows and not on the status: the rows of a view do if the view is not TRUNCATED, has at
#    least one kept row, every kept id is on the board and, for a fisheye camera, every kept pixel is inside the model (the test
#    of ``fisheye._solve``).  So a TOO_FEW view with 1 to 3 good rows contributes, and so does a DEGENERATE view of collinear rows:
#    every row is a constraint once another camera fixes the pose.  Otherwise none of the view's rows do;
# 3. seeds: every PNP_OK view is one.  Seed c is P = X_c^-1 o pose_{c,t} by ``_initial_rig``'s step 3 (c = 0: the view's own pose,
#    unchanged); its score is the JOINT COST there: the squared pixel residual over every contributing row of every camera
#    (cameras ascending, rows in pool order), +inf if a row is not in front of its camera.  The start is the seed with the lowest
#    score, the lowest camera among equals.  No seed -> PNP_TOO_FEW (no view solves on its own); every score +inf ->
#    PNP_DEGENERATE.  There is NO minimal solver for an instant at which no camera alone has four usable rows;
# 4. Levenberg-Marquardt over the 6 parameters of P_t on the joint cost with ``pnp._solve``'s rules, unchanged (damping
#    1 + 10^lg from lg = -3, a step accepted on cost <= prev_cost, a row behind its camera makes a trial's cost +inf and so a
#    rejection, lg + 1 on a rejection up to 16, at most 20 accepted steps, stop at |dp| / |p| < FLT_EPSILON, the same NONFINITE /
#    DEGENERATE endings).  The Jacobians are ``stereo._evaluate``'s P columns: a row of camera c >= 1 sees P through R(X_c);
# 5. outputs (``RigPoseResult``); everything continuous, and ``iterations``, is zero unless the timestamp's status is PNP_OK.
#
# ``rig_pose_host_full`` is the readable definition and the test pin; ``rig_pose_pools`` / ``rig_pose_device`` run the same steps on
# the GPU (csrc/dcx_rigpose.hip), without a host synchronisation, so the call can be captured in a graph.  The two agree to
# rounding (summation order), not bit for bit.

class RigPoseResult(NamedTuple):
    status: np.ndarray           # int32 [T], pnp.PNP_* per timestamp
    rvec: np.ndarray             # [T, 3] the board's pose P_t in camera 0's frame; zeros unless the status is PNP_OK
    tvec: np.ndarray             # [T, 3]
    rms: np.ndarray              # [T] sqrt(cost / rows) at the solution (px)
    iterations: np.ndarray       # int64 [T] accepted LM steps
    rows: np.ndarray             # int64 [T] the contributing rows of the timestamp, whatever the status
    seed: np.ndarray             # int32 [T] the camera whose pose started the solve, -1 if none did
    view_status: np.ndarray      # int32 [T, C], pnp.PNP_* per view: the view solved on its own
    view_points: np.ndarray      # int64 [T, C] rows the view brings (after its mask), contributing or not
    view_rms: np.ndarray         # [T, C] rms of the view at the solution; zero where it did not contribute


def _rig_x(rig):
    """``rig``: a solved ``RigResult`` or ``(R [C, 3, 3], T [C, 3])`` with camera 0 the identity -> (X [C - 1, 6] of (rvec, T), the
    sine term of every ``_rvec_of`` taken).  Both forms go through R, so they give the same bits."""
    if isinstance(rig, RigResult):
        if rig.status != RIG_OK:
            raise ValueError(f"the rig was not solved (status {rig.status})")
        R, T = rig.R, rig.T
    else:
        R, T = rig
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64)
    if R.ndim != 3 or R.shape[1:] != (3, 3) or not 2 <= R.shape[0] <= RIG_MAX_CAMERAS:
        raise ValueError(f"R must be [C, 3, 3] with C = 2 .. {RIG_MAX_CAMERAS}")
    T = T.reshape(R.shape[0], 3)
    if not (np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("the rig must be finite")
    if not np.array_equal(R[0], np.eye(3)) or T[0].any():
        raise ValueError("camera 0 must be the identity")
    return np.array([np.r_[_rvec_of(R[c]), T[c]] for c in range(1, R.shape[0])]), [_sine(R[c]) for c in range(1, R.shape[0])]


def _kept_rows(keypoints, mask, pool_order):
    """A view's rows after its mask, in pool order: the rows ``stereo._view_poses`` judges."""
    kp, order = _pool_rows(keypoints, pool_order)
    keep = np.ones(kp.shape[0], bool) if mask is None else np.asarray(mask).astype(bool).ravel()
    return kp[order][keep[order]]


def _contributes(kp, cam, n_ids):
    """Step 2 for the kept rows of a view that is not TRUNCATED."""
    if kp.shape[0] < 1:
        return False
    ids = kp[:, 2].astype(np.int64)
    if ids.min() < 0 or ids.max() >= n_ids:
        return False
    if len(cam) > 2 and cam[2] == "fisheye":
        from . import fisheye
        return bool(np.isfinite(fisheye._undistort(kp[:, :2].astype(np.float32).astype(np.float64), cam[0], cam[1])).all())
    return True


def _joint(rows, cams, X, p, jac):
    """The joint cost at P = p -> (residuals (M, 2), cost, J (2M, 6)): ``stereo._evaluate``'s residuals and P columns over one
    timestamp's contributing rows.  cost = +inf (and no residuals) if a row is not in front of its camera."""
    ev = _evaluate(rows, cams, X, p[None], jac)
    if ev is None:
        return None, math.inf, None
    return ev[0], float((ev[0] * ev[0]).sum()), ev[2].reshape(-1, 6) if jac else None


def rig_pose_host_full(keypoints_lists, col_count, row_count, square_len, cameras, dists, rig, masks=None, pool_order=False,
                       with_margin=False, models=None):
    """The definition (the comment above) -> ``RigPoseResult`` (with ``with_margin``: ``(result, margin)``).

    ``keypoints_lists``, ``cameras``, ``dists``, ``masks``, ``pool_order`` and ``models`` as ``rig_calibrate_host_full`` takes them;
    ``rig``: a ``RigResult`` (ValueError unless it is RIG_OK) or ``(R [C, 3, 3], T [C, 3])`` with camera 0 the identity.  Nothing
    raises for a timestamp that cannot be solved.

    ``with_margin``: the smallest relative distance of a discrete decision from its threshold: the gap between the best and the
    second-best seed score relative to the best (infinite with one seed), the sine term of every ``_rvec_of`` of step 3 and of the
    rig's own rotations from its switch at 1e-5, and the depth of every contributing row at the solution from 0 (relative to its
    distance from the camera centre)."""
    cams, _ = _cameras(cameras, dists, models)
    C = len(cams)
    X, sines = _rig_x(rig)
    if X.shape[0] != C - 1:
        raise ValueError(f"a rig of {X.shape[0] + 1} cameras for {C} cameras")
    if len(keypoints_lists) != C:
        raise ValueError(f"{len(keypoints_lists)} keypoint lists for {C} cameras")
    B = len(keypoints_lists[0])
    for c in range(C):
        if len(keypoints_lists[c]) != B:
            raise ValueError(f"{B} views of camera 0 but {len(keypoints_lists[c])} of camera {c}")
    mk = _mask_lists(masks, C)
    view_status, view_points, poses, _, _ = _view_poses(keypoints_lists, mk, cams, (col_count, row_count, square_len), pool_order)
    n_ids = (col_count - 1) * (row_count - 1)
    margin = min([math.inf] + [abs(s - 1e-5) / 1e-5 for s in sines])
    status = np.full(B, PNP_TOO_FEW, np.int32)
    rv, tv, rms, vr = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros(B), np.zeros((B, C))
    iters, nrows, seed = np.zeros(B, np.int64), np.zeros(B, np.int64), np.full(B, -1, np.int32)
    for t in range(B):
        views = []
        for c in range(C):
            kp = _kept_rows(keypoints_lists[c][t], None if mk[c] is None else mk[c][t], pool_order)
            if view_status[t, c] != PNP_TRUNCATED and _contributes(kp, cams[c], n_ids):
                views.append((c, object_points(kp[:, 2].astype(np.int64), col_count, row_count, square_len), kp[:, :2].astype(np.float32)))
        nrows[t] = sum(v[1].shape[0] for v in views)
        seeds = [c for c in range(C) if view_status[t, c] == PNP_OK]
        if not seeds:
            continue                                             # PNP_TOO_FEW: no view solves on its own
        rows = _rows_of([views], C)                              # (a seed's view contributes: there are rows)
        best, second, start = math.inf, math.inf, None
        for c in seeds:
            p0, sine = (poses[t, 0].copy(), None) if c == 0 else _seed_pose(X[c - 1], poses[t, c])
            if sine is not None:
                margin = min(margin, abs(sine - 1e-5) / 1e-5)
            score = _joint(rows, cams, X, p0, False)[1]
            if score < best:
                best, second, start, seed[t] = score, best, p0, c
            elif score < second:
                second = score
        if start is None:
            status[t] = PNP_DEGENERATE
            continue
        if second < math.inf:
            margin = min(margin, (second - best) / best if best > 0 else math.inf)
        st, p, cost, it = _lm.refine_pose(lambda q, jac: _joint(rows, cams, X, q, jac), start, LM_MAX_ITER, LM_EPS)
        status[t] = st = LM_STATUS[st]
        if st != PNP_OK:
            continue
        rv[t], tv[t], rms[t], iters[t] = p[:3], p[3:], math.sqrt(cost / nrows[t]), it
        res = _joint(rows, cams, X, p, False)[0]
        for (c, o, _), a in zip(views, rows.vstarts):
            r = res[a:a + o.shape[0]]
            vr[t, c] = math.sqrt(float((r * r).sum()) / o.shape[0])
        if with_margin:
            margin = min(margin, _depth_margin(rows, X, p[None]))
    r = RigPoseResult(status, rv, tv, rms, iters, nrows, seed, view_status.astype(np.int32), view_points.astype(np.int64), vr)
    return (r, margin) if with_margin else r


def rig_pose_host(keypoints_lists, col_count, row_count, square_len, cameras, dists, rig, masks=None, models=None):
    """``(ok bool [T], rvecs [T, 3], tvecs [T, 3])``: the board's pose in camera 0's frame per timestamp (zeros where ``ok`` is
    False).  Raises where ``rig_calibrate_host`` raises: IndexError for an id outside the board, ValueError for a view that has
    rows none of which can be used (a fisheye view with a pixel outside the model) and for refused arguments.  A view of 1 to 3 rows
    or of collinear rows is used here and no error; a timestamp that cannot be solved is ``ok`` = False, not an error."""
    r = rig_pose_host_full(keypoints_lists, col_count, row_count, square_len, cameras, dists, rig, masks, models=models)
    cams, _ = _cameras(cameras, dists, models)
    mk = _mask_lists(masks, len(cams))
    n_ids = (col_count - 1) * (row_count - 1)
    for t, c in np.argwhere(r.view_points > 0):
        kp = _kept_rows(keypoints_lists[c][t], None if mk[c] is None else mk[c][t], False)
        ids = kp[:, 2].astype(np.int64)
        if ids.min() < 0 or ids.max() >= n_ids:
            raise _bad_id_error(col_count, row_count)
        if not _contributes(kp, cams[c], n_ids):
            raise ValueError(f"view {int(t)} of camera {int(c)} cannot be used (status {int(r.view_status[t, c])})")
    return r.status == PNP_OK, r.rvec, r.tvec


# ------------------------------------------------------------------------------------------------ rig pose on the device

POSE_HEAD_WORDS = 2            # d_head of dcx_rig_pose_pool: {a masked pool's views share slots, reserved (0)}


def rig_pose_workspace_bytes(n_cams: int, batch: int, pools) -> int:
    """Bytes of device workspace ``rig_pose_pools`` needs."""
    from . import _lib
    pools = [int(p) for p in pools]
    if len(pools) != int(n_cams):
        raise ValueError("one pool size per camera is required")
    n = int(_lib.lib().dcx_rig_pose_workspace_bytes(int(n_cams), int(batch), (_ctypes.c_int * len(pools))(*pools)))
    if n == 0:
        raise ValueError(f"2 to {RIG_MAX_CAMERAS} cameras, batch >= 1 and pools >= 0 are required")
    return n


def _pose_outputs(out, batch, n_cams, dev):
    """-> (head int32 [2], status int32 [B], pose float64 [B, 8], info int32 [B, 2], view_status int32 [B, C], view_info float64
    [B, C, 2]): the caller's ``out`` checked, or new tensors."""
    import torch
    specs = ((torch.int32, (POSE_HEAD_WORDS,)), (torch.int32, (batch,)), (torch.float64, (batch, 8)), (torch.int32, (batch, 2)),
             (torch.int32, (batch, n_cams)), (torch.float64, (batch, n_cams, 2)))
    if out is not None and len(out) != len(specs):
        raise ValueError("out must be the six tensors rig_pose_pools returns")
    msg = (f"out must be (int32 [2], int32 [{batch}], float64 [{batch}, 8], int32 [{batch}, 2], int32 [{batch}, {n_cams}], float64 "
           f"[{batch}, {n_cams}, 2]) contiguous tensors on {dev}")
    return tuple(_dev.tensor(None if out is None else out[i], dev, dt, shape, msg, "numel") for i, (dt, shape) in enumerate(specs))


def rig_pose_pools(packed_list, batch: int, pools, refined: bool, col_count, row_count, square_len, cameras, dists, rig, masks=None,
                   models=None, workspace=None, out=None):
    """The board's pose per timestamp from C ``infer_batch_device`` results of ``batch`` frames each and a fixed rig, read in place
    from the C corner pools (the conventions of ``rig_calibrate_pools``: ``pools``, ``masks``, ``models``).  ``rig``: a
    ``RigResult`` (ValueError unless RIG_OK) or ``(R, T)``.  Enqueued on the current stream: no host synchronisation, and nothing
    allocated when ``workspace`` (at least ``rig_pose_workspace_bytes`` bytes) and ``out`` are given, so the call can be captured
    in a graph.  Returns the device tensors ``(head, status, pose, info, view_status, view_info)`` (``out`` = those six,
    preallocated); ``unpack_rig_poses`` makes a ``RigPoseResult`` of them and raises DcxError if a masked pool's views share
    slots, which only the device can see."""
    import torch
    from . import _lib
    cams, dists = _cameras(cameras, dists, models)
    C = len(cams)
    models = _models(models, C)
    X, _ = _rig_x(rig)
    pools = [int(p) for p in pools]
    if X.shape[0] != C - 1 or len(packed_list) != C or len(pools) != C:
        raise ValueError(f"{C} cameras need a rig of {C} cameras, {C} pools and {C} pool sizes")
    dev = packed_list[0].device
    if any(p.device != dev for p in packed_list):
        raise ValueError("the pools must be on one device")
    mk = _mask_lists(masks, C)
    _device_masks(mk, pools, dev)
    table = (_RigCamera * C)()
    for c in range(C):
        counts_p, starts_p, rows_p, xy_p = _pool_ptrs(packed_list[c], batch, pools[c], refined)
        cam9, d8, nd = _model_args(cameras[c], dists[c], models and models[c])
        table[c] = _RigCamera(counts_p, starts_p, rows_p, xy_p, pools[c], _lib.ptr(mk[c]), cam9, d8, nd)
    outs = _pose_outputs(out, batch, C, dev)
    nbytes = rig_pose_workspace_bytes(C, batch, pools)
    ws = _dev.workspace(workspace, dev, nbytes, f"workspace must be a contiguous tensor of at least {nbytes} bytes on {dev}")
    tags = None if models is None else (_ctypes.c_int * C)(*(MODELS.index(m) for m in models))
    x = (_ctypes.c_double * (6 * (C - 1)))(*X.ravel().tolist())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_rig_pose_pool(C, table, tags, x, int(batch), int(col_count), int(row_count), float(square_len),
                                                ws.data_ptr(), ws.numel() * ws.element_size(), *(o.data_ptr() for o in outs),
                                                _lib.current_stream()), "dcx_rig_pose_pool")
    return outs


def unpack_rig_poses(head, status, pose, info, view_status, view_info) -> RigPoseResult:
    """``rig_pose_pools``' device tensors -> a ``RigPoseResult`` on the host (this synchronises).  DcxError (DCX_E_ARG) if the
    call found a masked pool whose views share slots, as ``rig_calibrate_pools`` raises for the same breach."""
    from . import _lib
    head, status, pose, info, view_status, view_info = (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
                                                        for v in (head, status, pose, info, view_status, view_info))
    if int(head.ravel()[0]):
        raise _lib.DcxError(-1, "dcx_rig_pose_pool (two views of a masked pool share slots)")
    B = status.size
    pose, info, view_info = pose.reshape(B, 8), info.reshape(B, 2), view_info.reshape(B, -1, 2)
    return RigPoseResult(status.reshape(B).astype(np.int32), pose[:, 0:3].copy(), pose[:, 3:6].copy(), pose[:, 6].copy(),
                         pose[:, 7].astype(np.int64), info[:, 1].astype(np.int64), info[:, 0].astype(np.int32),
                         view_status.reshape(B, -1).astype(np.int32), view_info[:, :, 1].astype(np.int64), view_info[:, :, 0].copy())


def rig_pose_device(keypoints_lists: Sequence, col_count, row_count, square_len, cameras, dists, rig, masks=None, device="cuda",
                    models=None) -> RigPoseResult:
    """``rig_pose_host_full`` on the GPU from ``infer_image``-format keypoint arrays ([x, y, id] rows; one list per camera, equally
    long) -> ``RigPoseResult``.  ``rig``, ``masks`` and ``models`` as for the host definition."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    cams, dists = _cameras(cameras, dists, models)            # ValueError before anything is uploaded
    C = len(cams)
    _rig_x(rig)
    if len(keypoints_lists) != C:
        raise ValueError(f"{len(keypoints_lists)} keypoint lists for {C} cameras")
    B = len(keypoints_lists[0])
    if any(len(k) != B for k in keypoints_lists):
        raise ValueError("every camera needs as many views as camera 0")
    packs, dm = _upload(keypoints_lists, _mask_lists(masks, C), dev)
    with torch.cuda.device(dev):
        outs = rig_pose_pools([p[0] for p in packs], B, [p[2] for p in packs], True, col_count, row_count, square_len, cameras, dists,
                              rig, None if masks is None else dm, models)
        return unpack_rig_poses(*outs)


# ------------------------------------------------------------------------------------------------ how well the rig is determined
# The covariances of the rig's extrinsics X_c and of the board poses P_t at a solved rig, the intrinsics held fixed:
# ``calib.calibration_uncertainty_host``'s definition with the rig's 6 (C - 1) shared parameters in the intrinsics' place.
# ``rig_uncertainty_host`` is the definition and the pin of csrc/dcx_rig_cov.hip; ``stereo.stereo_uncertainty_*`` are the C = 2 case
# through the same functions.

RIGCOV_STRIDE = 42             # DCX_RIGCOV_STRIDE: the row stride of cov_rig in d_global, 6 (RIG_MAX_CAMERAS - 1)
RIGCOV_STD, RIGCOV_SIGMA2 = 1764, 1806          # DCX_RIGCOV_STD; DCX_RIGCOV_SIGMA2, then dof, points, stamps, status, 0
RIGCOV_GLOBAL_WORDS = 1812     # DCX_RIGCOV_GLOBAL_WORDS
# csrc/dcx_rig_cov.hip's summation orders.  A view's 91 entries: its rows in pool order, 64 at a time (a masked row adds zeros).
# U_t: the usable cameras ascending.  The timestamps' parts of V, of the Schur sum, of the cost and of the counts: chunks of
# REDUCE_COV_CHUNK timestamps in order, one thread per entry; then slice s of REDUCE_COV_SLICES adds the chunks s, s + 16, ... in
# order and the slices are added serially, 0 first.  The cost of a timestamp: its usable cameras ascending.  cov_pose_t: for a
# ascending, Y[r, a] * (sum over k ascending of S^-1[a, k] Y[c, k]), added to U_t^-1[r, c].
REDUCE_COV_CHUNK, REDUCE_COV_SLICES = 16, 16


class RigUncertainty(NamedTuple):
    status: int                  # calib.COV_*
    cov_rig: np.ndarray          # [n, n], n = 6 (C - 1): rvec_c, T_c per camera, cameras 1 .. C - 1 ascending
    std_rig: np.ndarray          # [C, 6]: the roots of cov_rig's diagonal; row 0 (the reference camera) is zeros
    cov_poses: np.ndarray        # [T, 6, 6]: rvec then tvec of P_t; zeros for a timestamp that was not used
    std_poses: np.ndarray        # [T, 6]
    baseline_std: np.ndarray     # [C]: the standard deviation of |T_c|; 0 for camera 0
    sigma2: float                # sum |r|^2 / dof (px^2)
    dof: int                     # 2 * points - 6 (C - 1) - 6 * stamps
    points: int                  # kept rows of the usable views of the used timestamps
    stamps: int                  # timestamps used


def _rig_model(result_or_model, n_cams: int, batch: int):
    """``result_or_model`` of the uncertainty calls -> (X [C - 1, 6], P [T, 6], view_status int32 [T, C]).  A ``RigResult`` (or,
    for two cameras, a ``StereoResult``) must be solved (ValueError); a tuple is taken as it stands."""
    r = result_or_model
    if hasattr(r, "view_status") and hasattr(r, "rvecs"):
        if r.status != RIG_OK:
            raise ValueError(f"the calibration failed (status {r.status}): there is no solution to take an uncertainty at")
        rvec, T = np.asarray(r.rvec, np.float64).reshape(-1, 3), np.asarray(r.T, np.float64).reshape(-1, 3)
        if rvec.shape[0] == n_cams - 1 == 1:                    # a StereoResult: X_1 alone
            rvec, T = np.r_[np.zeros((1, 3)), rvec], np.r_[np.zeros((1, 3)), T]
        R, rvecs, tvecs, vs = rvec, r.rvecs, r.tvecs, r.view_status
    else:
        try:
            R, T, rvecs, tvecs, vs = r
        except (TypeError, ValueError):
            raise ValueError("result_or_model must be a RigResult or (R [C, 3, 3] or rvec [C, 3], T [C, 3], rvecs [T, 3], tvecs "
                             "[T, 3], view_status [T, C])") from None
    R = np.asarray(R, np.float64)
    rvec = np.stack([_rvec_of(m) for m in R]) if R.ndim == 3 else R.reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3)
    P = np.c_[np.asarray(rvecs, np.float64).reshape(-1, 3), np.asarray(tvecs, np.float64).reshape(-1, 3)]
    vs = np.asarray(vs).astype(np.int32).reshape(P.shape[0], -1)
    if rvec.shape[0] != n_cams or T.shape[0] != n_cams or vs.shape != (batch, n_cams):
        raise ValueError(f"{n_cams} cameras and {batch} timestamps need a rig of {n_cams} cameras, {batch} board poses and view "
                         f"statuses [{batch}, {n_cams}]")
    return np.c_[rvec, T][1:], P, vs


def _uncertainty_result(status, C, B, used, points, sigma2=0.0, cov=None, blocks=None, X=None) -> RigUncertainty:
    n = 6 * (C - 1)
    cr, cp, base = np.zeros((n, n)), np.zeros((B, 6, 6)), np.zeros(C)
    if status == COV_OK:
        cr, cp[used] = cov, blocks
        for c in range(1, C):
            t, s = X[c - 1, 3:], slice(6 * (c - 1) + 3, 6 * c)
            norm = math.sqrt(float(t @ t))
            if norm > 0:
                u = t / norm
                base[c] = math.sqrt(max(float(u @ cr[s, s] @ u), 0.0))
    return RigUncertainty(int(status), cr, np.r_[np.zeros((1, 6)), np.sqrt(np.diag(cr)).reshape(C - 1, 6)], cp,
                          np.sqrt(np.diagonal(cp, axis1=1, axis2=2)), base, float(sigma2), int(2 * points - n - 6 * len(used)),
                          int(points), int(len(used)))


def _uncertainty_host(keypoints_lists, board, cams, mk, X, P, view_status, pool_order=False) -> RigUncertainty:
    """The definition (``rig_uncertainty_host``) on checked arguments."""
    col_count, row_count, square_len = board
    C, B = len(cams), len(keypoints_lists[0])
    n_ids = (col_count - 1) * (row_count - 1)
    usable = view_status == PNP_OK
    used = np.flatnonzero(usable.sum(1) >= 2)
    stamps, points, bad = [], 0, False
    for t in used:
        views = []
        for c in np.flatnonzero(usable[t]):
            kp = _kept_rows(keypoints_lists[c][t], None if mk[c] is None or mk[c][t] is None else mk[c][t], pool_order)
            points += kp.shape[0]
            ids = kp[:, 2].astype(np.int64)
            if kp.shape[0] and (ids.min() < 0 or ids.max() >= n_ids):
                bad = True                                        # (an id that is not on the board has no point to project)
            elif kp.shape[0]:
                views.append((int(c), object_points(ids, col_count, row_count, square_len), kp[:, :2].astype(np.float32)))
        bad |= not views                                          # (no row at all: U_t = 0)
        stamps.append(views)

    def out(status, *a):
        return _uncertainty_result(status, C, B, used, points, *a)

    dof = 2 * points - 6 * (C - 1) - 6 * used.size
    if not used.size:
        return out(COV_NO_VIEWS)
    if dof <= 0:
        return out(COV_NO_DOF)
    if bad or not (np.isfinite(X).all() and np.isfinite(P[used]).all()):
        return out(COV_SINGULAR)
    rows = _rows_of(stamps, C)
    nb = _normal_blocks(rows, cams, X, P[used], _view_segments(rows))
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
    return out(COV_OK, sigma2, cov, blocks, X)


def rig_uncertainty_host(keypoints_lists, col_count, row_count, square_len, cameras, dists, result_or_model, masks=None,
                         models=None, pool_order=False) -> RigUncertainty:
    """How well a solved rig is determined: the covariance of the rig's extrinsics X_c = (rvec_c, T_c), c = 1 .. C - 1, and of every
    used timestamp's board pose P_t, GIVEN THE CAMERA MODELS: the intrinsics and distortion coefficients are held fixed, as the rig
    calibration holds them, so their own uncertainty (``calib.calibration_uncertainty_*``) is not propagated into these numbers.
    In float64 on the host; the definition and the pin of ``dcx_rig_uncertainty_pool``.

    ``keypoints_lists``, ``cameras``, ``dists``, ``masks``, ``models`` and ``pool_order`` as ``rig_calibrate_host_full`` takes them.
    ``result_or_model``: the ``RigResult`` of a calibration of these views (ValueError unless it is ``RIG_OK``), or the tuple
    ``(R [C, 3, 3] or rvec [C, 3], T [C, 3], rvecs [T, 3], tvecs [T, 3], view_status [T, C])`` with camera 0's entries ignored;
    the tuple is not checked for connectivity.

    A view is usable iff its ``view_status`` is ``PNP_OK``; a timestamp is used iff two of its views are usable.  The rows are the
    usable views' rows after their masks, in pool order, exactly as ``rig_calibrate_host_full`` builds them.  With the UNDAMPED
    normal blocks of ``stereo._normal_blocks`` at (X, P) (U_t 6 x 6, W_t n x 6, V n x n block diagonal, n = 6 (C - 1)):
    S = V - sum W_t U_t^-1 W_t^T, Y_t = U_t^-1 W_t^T (``_lm.schur_covariance``), dof = 2 points - n - 6 stamps,
    sigma^2 = sum |r|^2 / dof, cov_rig = sigma^2 S^-1 (in the order rvec_c, T_c per camera, cameras ascending),
    cov_pose_t = sigma^2 (U_t^-1 + Y_t S^-1 Y_t^T); standard deviations are the roots of the diagonals.  ``baseline_std[c]`` is
    the standard deviation of |T_c|, sqrt(u^T Cov(T_c) u) with u = T_c / |T_c| (first order; host arithmetic on ``cov_rig``).

    The sigma^2 convention is ``calib.calibration_uncertainty_host``'s: residuals (two per point) minus parameters; ``sigma2``,
    ``dof``, ``points`` and ``stamps`` are returned for a caller who wants another.  Not reported: the cross-covariances between
    the X_c and the P_t.

    Statuses, in this order: ``COV_NO_VIEWS`` (no used timestamp), ``COV_NO_DOF`` (dof <= 0), ``COV_SINGULAR`` (a U_t or S that is
    not positive definite, which includes a camera c >= 1 without a usable view in any used timestamp; a point not in front of its
    camera; an id outside the board in a used view; a value that is not finite; on the device also a used view whose slots leave
    its pool).  Everything but the status and the counts is zero unless ``COV_OK``; unused timestamps get zeros."""
    cams, _ = _cameras(cameras, dists, models)
    C = len(cams)
    if len(keypoints_lists) != C:
        raise ValueError(f"{len(keypoints_lists)} keypoint lists for {C} cameras")
    B = len(keypoints_lists[0])
    if any(len(k) != B for k in keypoints_lists):
        raise ValueError("every camera needs as many views as camera 0")
    X, P, vs = _rig_model(result_or_model, C, B)
    return _uncertainty_host(keypoints_lists, (col_count, row_count, square_len), cams, _mask_lists(masks, C), X, P, vs, pool_order)


# ---- on the device

def rig_uncertainty_workspace_bytes(n_cams: int, batch: int, pools) -> int:
    """Bytes of device workspace ``rig_uncertainty_pools`` needs."""
    from . import _lib
    pools = [int(p) for p in pools]
    if len(pools) != int(n_cams):
        raise ValueError("one pool size per camera is required")
    n = int(_lib.lib().dcx_rig_uncertainty_workspace_bytes(int(n_cams), int(batch), (_ctypes.c_int * len(pools))(*pools)))
    if n == 0:
        raise ValueError(f"2 to {RIG_MAX_CAMERAS} cameras, batch >= 1 and pools >= 0 are required")
    return n


def _device_model(result_or_model, n_cams, batch, dev):
    """``result_or_model`` of ``rig_uncertainty_pools`` -> (X [C - 1, 6] on the host, view_status int32 [B, C] and pose float64
    [B, 8] on ``dev``).  The four-entry tuple ``(R or rvec, T, view_status, pose)`` carries the last two as the calibration wrote
    them, arrays or device tensors (taken as they are); everything else goes through ``_rig_model`` and is uploaded."""
    import torch
    r = result_or_model
    if isinstance(r, (tuple, list)) and len(r) == 4:
        R, T, vs, pose = r
        X = _rig_model((R, T, np.zeros((batch, 3)), np.zeros((batch, 3)), np.zeros((batch, n_cams), np.int32)), n_cams, batch)[0]
    else:
        X, P, vs = _rig_model(r, n_cams, batch)
        pose = np.zeros((batch, 8))
        pose[:, :6] = P
    return (X, _device_or_upload(vs, dev, torch.int32, (batch, n_cams), "view_status"),
            _device_or_upload(pose, dev, torch.float64, (batch, 8), "pose"))


def rig_uncertainty_pools(packed_list, batch: int, pools, refined: bool, col_count, row_count, square_len, cameras, dists,
                          result_or_model, masks=None, models=None, workspace=None, out=None):
    """``rig_uncertainty_host`` on the GPU, read in place from the C corner pools the calibration read (the conventions of
    ``rig_calibrate_pools``: ``pools``, ``masks``, ``models``) -> device tensors ``(global_ float64 [RIGCOV_GLOBAL_WORDS], pose_cov
    float64 [B, COV_POSE_WORDS])``, which ``unpack_rig_uncertainty`` turns into a ``RigUncertainty``.

    ``result_or_model``: what ``rig_uncertainty_host`` takes, or ``(R [C, 3, 3] or rvec [C, 3], T [C, 3], view_status [B, C] int32,
    pose [B, 8] float64)`` with the last two as arrays or as the device tensors ``dcx_rig_calibrate_pool`` wrote.  ``workspace``: at
    least ``rig_uncertainty_workspace_bytes`` bytes; ``out``: the two output tensors.  Five launches on the current stream; no
    synchronisation, and given device tensors throughout nothing is allocated and the call can be captured in a graph (a result or
    host arrays are uploaded first).  Unlike the calibration, views of a masked pool may share slots here."""
    import torch
    from . import _lib
    cams, dists = _cameras(cameras, dists, models)
    C = len(cams)
    models = _models(models, C)
    pools = [int(p) for p in pools]
    if len(packed_list) != C or len(pools) != C:
        raise ValueError(f"{C} cameras need {C} pools and {C} pool sizes")
    dev = packed_list[0].device
    if any(p.device != dev for p in packed_list):
        raise ValueError("the pools must be on one device")
    X, vs_d, pose_d = _device_model(result_or_model, C, batch, dev)
    mk = _mask_lists(masks, C)
    _device_masks(mk, pools, dev)
    table = (_RigCamera * C)()
    for c in range(C):
        counts_p, starts_p, rows_p, xy_p = _pool_ptrs(packed_list[c], batch, pools[c], refined)
        cam9, d8, nd = _model_args(cameras[c], dists[c], models and models[c])
        table[c] = _RigCamera(counts_p, starts_p, rows_p, xy_p, pools[c], _lib.ptr(mk[c]), cam9, d8, nd)
    nbytes = rig_uncertainty_workspace_bytes(C, batch, pools)
    ws = _dev.workspace(workspace, dev, nbytes, f"workspace must be a contiguous tensor of at least {nbytes} bytes on {dev}")
    if out is None:
        out = (torch.empty((RIGCOV_GLOBAL_WORDS,), dtype=torch.float64, device=dev),
               torch.empty((batch, COV_POSE_WORDS), dtype=torch.float64, device=dev))
    glob = _dev.tensor(out[0], dev, torch.float64, (RIGCOV_GLOBAL_WORDS,), f"out[0] must be a contiguous float64 tensor of "
                       f"{RIGCOV_GLOBAL_WORDS} values on {dev}")
    pcov = _dev.tensor(out[1], dev, torch.float64, (batch, COV_POSE_WORDS), f"out[1] must be a contiguous float64 tensor "
                       f"[{batch}, {COV_POSE_WORDS}] on {dev}")
    tags = None if models is None else (_ctypes.c_int * C)(*(MODELS.index(m) for m in models))
    x = (_ctypes.c_double * (6 * (C - 1)))(*X.ravel().tolist())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_rig_uncertainty_pool(C, table, tags, x, int(batch), int(col_count), int(row_count), float(square_len),
                                                       vs_d.data_ptr(), pose_d.data_ptr(), ws.data_ptr(),
                                                       ws.numel() * ws.element_size(), glob.data_ptr(), pcov.data_ptr(),
                                                       _lib.current_stream()), "dcx_rig_uncertainty_pool")
    return glob, pcov


def unpack_rig_uncertainty(global_, pose_cov, T) -> RigUncertainty:
    """The two tensors of ``rig_uncertainty_pools`` and the rig's T [C, 3] (a ``RigResult``'s, or the tuple's) -> a
    ``RigUncertainty`` on the host (this synchronises).  ``baseline_std`` is host arithmetic on ``cov_rig``, as in the definition."""
    g, p = global_.cpu().numpy(), pose_cov.cpu().numpy()
    T = np.asarray(T, np.float64).reshape(-1, 3)
    C = T.shape[0]
    n = 6 * (C - 1)
    s2, dof, points, stamps, status = g[RIGCOV_SIGMA2:RIGCOV_SIGMA2 + 5]
    cov = g[:RIGCOV_STD].reshape(RIGCOV_STRIDE, RIGCOV_STRIDE)[:n, :n].copy()
    base = np.zeros(C)
    if int(status) == COV_OK:
        for c in range(1, C):
            s = slice(6 * (c - 1) + 3, 6 * c)
            norm = math.sqrt(float(T[c] @ T[c]))
            if norm > 0:
                u = T[c] / norm
                base[c] = math.sqrt(max(float(u @ cov[s, s] @ u), 0.0))
    return RigUncertainty(int(status), cov, np.r_[np.zeros((1, 6)), g[RIGCOV_STD:RIGCOV_STD + n].reshape(C - 1, 6)],
                          p[:, :36].reshape(-1, 6, 6).copy(), p[:, 36:42].copy(), base, float(s2), int(dof), int(points), int(stamps))


def _model_T(result_or_model):
    r = result_or_model
    return r.T if hasattr(r, "view_status") else r[1]


def rig_uncertainty_device(keypoints_lists: Sequence, col_count, row_count, square_len, cameras, dists, result_or_model, masks=None,
                           device="cuda", models=None) -> RigUncertainty:
    """``rig_uncertainty_host`` on the GPU from ``infer_image``-format keypoint arrays ([x, y, id] rows; one list per camera,
    equally long), the views the calibration was given -> ``RigUncertainty``.  ``result_or_model``, ``masks`` and ``models`` as for
    the host definition."""
    import torch
    from .models._handles import require_cuda
    dev = require_cuda(device)
    cams, dists = _cameras(cameras, dists, models)            # ValueError before anything is uploaded
    C = len(cams)
    if len(keypoints_lists) != C:
        raise ValueError(f"{len(keypoints_lists)} keypoint lists for {C} cameras")
    B = len(keypoints_lists[0])
    if any(len(k) != B for k in keypoints_lists):
        raise ValueError("every camera needs as many views as camera 0")
    packs, dm = _upload(keypoints_lists, _mask_lists(masks, C), dev)
    with torch.cuda.device(dev):
        g, p = rig_uncertainty_pools([p[0] for p in packs], B, [p[2] for p in packs], True, col_count, row_count, square_len, cameras,
                                     dists, result_or_model, None if masks is None else dm, models)
        T = np.asarray(_model_T(result_or_model), np.float64).reshape(-1, 3)
        return unpack_rig_uncertainty(g, p, T if T.shape[0] == C else np.r_[np.zeros((1, 3)), T])
