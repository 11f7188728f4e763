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
"""
from __future__ import annotations

import ctypes as _ctypes
import math
from typing import NamedTuple, Sequence

import numpy as np

from . import _dev, _lm
from .calib import _no_bad_id
from .pnp import PNP_OK, _camera, _pool_ptrs, _rodrigues, _rvec_of
# every step that does not depend on the number of cameras is stereo.py's, kept once
from .stereo import (MODELS, STEREO_EPS, STEREO_MAX_ITER, _call, _depth_margin, _device_masks, _model_args, _model_cameras, _models,
                     _outputs, _raise_like_cv2, _refine, _rig_init, _sine, _total, _unpack, _upload, _view_poses, _view_segments,
                     essential_fundamental)
from .stereo import _rig_rows as _rows_of
from .stereo import _dist, _evaluate, _model_of     # noqa: F401  (the names the tests reach through this module)

# overall status (include/deepcharuco_amd.h); per-view statuses are pnp's PNP_*
RIG_OK, RIG_NO_STAMPS, RIG_DEGENERATE, RIG_NONFINITE = _lm.LM_OK, _lm.LM_NO_UNITS, _lm.LM_DEGENERATE, _lm.LM_NONFINITE
RIG_DISCONNECTED = 4
RIG_MAX_CAMERAS = 8
RIG_MAX_ITER, RIG_EPS = STEREO_MAX_ITER, STEREO_EPS      # step 4's rules are stereo's: ``stereo._refine`` runs both
RESULT_HEAD = 8                # h_result of dcx_rig_calibrate_pool: 8 words, then X_1 .. X_{C-1}
REDUCE_CHUNK, REDUCE_SLICES = 16, 16   # csrc/dcx_rig.hip's kChunk, kSlices: the two fan-ins of the per-attempt reduction

__all__ = ["RigResult", "rig_calibrate_host", "rig_calibrate_host_full", "rig_calibrate_pools", "rig_calibrate_device", "rig_pair",
           "workspace_bytes", "RIG_OK", "RIG_NO_STAMPS", "RIG_DEGENERATE", "RIG_NONFINITE", "RIG_DISCONNECTED"]


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
            Rc = _rodrigues(X[c, :3])
            R = Rc.T @ _rodrigues(poses[t, c, :3])
            margin = min(margin, abs(_sine(R) - 1e-5) / 1e-5)
            P[i] = np.r_[_rvec_of(R), Rc.T @ (poses[t, c, 3:] - X[c, 3:])]
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
