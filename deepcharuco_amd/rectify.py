"""Stereo rectification without OpenCV: the rectifying transforms of a calibrated rig (``cv2.stereoRectify`` with
CALIB_ZERO_DISPARITY), the undistort + rectify map (``cv2.initUndistortRectifyMap``, fixed point), the remap of u8 frames through it
(``cv2.remap`` INTER_LINEAR / BORDER_CONSTANT) and the detected corners in rectified coordinates (``cv2.undistortPoints`` with R
and P), on the host and on the GPU (csrc/dcx_rectify.hip).

Conventions: cameras as the PnP entry points take them (K without skew, 0 / 4 / 5 / 8 distortion coefficients), the rig as cv2's
q1 = R q0 + T (what ``stereo.stereo_calibrate_pool`` returns), pools as ``pnp.solve_pnp_pool`` reads them.  All geometry in float64.

1. ``stereo_rectify_host`` (numpy only: once per rig, over 18 numbers and the 2 (W + H) border pixels).  Bouguet's construction:
   om = rvec(R), r_r = exp(-om / 2), t = r_r T; ``axis`` = 0 if |t0| > |t1| else 1 (1: a vertical rig); u = +-e_axis with the sign
   of t[axis]; w = t x u scaled to the angle between t and u, acos(|t[axis]| / |t|) (evaluated as atan2(|t x u|, |t[axis]|), the
   same angle without acos's loss near 1); R1 = exp(w) r_r^T, R2 = exp(w) r_r, Tn = (R2 T)[axis].  f = min(fy0, fy1).  Per camera
   the four image corners (0, 0), (W-1, 0), (W-1, H-1), (0, H-1) are undistorted (step 3's Newton), rotated by R_c and averaged to
   (xm, ym); c_c = ((W-1)/2 - f xm, (H-1)/2 - f ym), and both cameras get the mean of c_0 and c_1.  With ``alpha`` in [0, 1]
   EVERY border pixel centre of each camera is undistorted and rotated (cv2 samples a 9 x 9 grid); inner rectangle = (max x of
   the left edge, min x of the right edge, max y of the top edge, min y of the bottom edge), each extreme polished between the
   extreme pixel's neighbours so that it holds for the continuous edge; outer = min / max over all the pixel centres;
   with the principal point kept, s0 f is the smallest focal length at which both inner rectangles cover [0, W-1] x [0, H-1] and
   s1 f the largest at which both outer rectangles fit inside it; f <- f (s0 (1 - alpha) + s1 alpha).
   P1 = [f 0 cx 0; 0 f cy 0; 0 0 1 0], P2 = P1 with P2[axis, 3] = Tn f; Q (x0, y0, d, 1)^T with d the difference of the ``axis``
   coordinates (camera 0 minus camera 1) is the homogeneous 3-D point in rectified camera 0's frame (Z = -f Tn / d).
2. the map, for output pixel (u, v): x = (u - P02) / P00, y = (v - P12) / P11, q = R^T (x, y, 1); q_z <= 0, a non-finite
   result or one beyond +-2^15 px gives the sentinel INT32_MIN in both components ("outside"); else m = the camera's projection of
   (q_x / q_z, q_y / q_z) through the distortion model and the entry is rint(32 m) as int32 (5 fractional bits, ties to even).
   R = None: identity; P = None: K, so ``cv2.undistort`` falls out of the same call.
3. rectified points: pixel -> P R undistort(pixel).  Undistortion is Newton on the distortion model's analytic 2 x 2 Jacobian from
   the normalised pixel: stop when both components of the step are below 1e-15, at most 20 steps, NaN if it has not converged by
   then or if the rotated z <= 0.  Only the left 3 x 3 of P is used (as cv2.undistortPoints does).
4. the remap (integer, so host and device agree bit for bit): x0 = mx >> 5, y0 = my >> 5 (arithmetic shifts: a floor), fx = mx & 31,
   fy = my & 31; taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), each tap outside the source reads ``border`` (per tap:
   BORDER_CONSTANT), a sentinel entry gives ``border``;
   out = ((32-fx)(32-fy) p00 + fx (32-fy) p10 + (32-fx) fy p01 + fx fy p11 + 512) >> 10 per channel.

Deviations from cv2:
* undistortion by Newton to convergence where cv2.undistortPoints (and this package's PnP, for cv2's sake) runs 5 fixed-point
  rounds: with k1 = -0.25 five rounds are up to 4.8e-3 px off over a 320 x 240 frame (Newton: 7e-14 px in at most 5 steps), and
  rows of two rectified images are compared far below that;
* ``alpha`` uses every border pixel, not a 9 x 9 grid, so that at alpha = 0 no output pixel reads outside the source and at
  alpha = 1 no source pixel falls outside the output, exactly; no valid-pixel ROIs are returned;
* f = min(fy0, fy1) for both rig orientations;
* the remap is cv2's 5-bit INTER_LINEAR scheme with the four weights as exact products; cv2's own weight table is rounded and
  patched to sum to 2^15, so bit parity with ``cv2.remap`` is not claimed.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _dev, pnp
from .pnp import _camera, _dist, _distort, _rodrigues, _rvec_of

MAP_SENTINEL = int(np.iinfo(np.int32).min)     # both components of a map entry that is outside
MAP_BITS = 5                                   # fractional bits of a map entry
MAP_LIMIT = 32768.0                            # |m| beyond this many px is outside
NEWTON_MAX_ITER = 20
NEWTON_EPS = 1e-15
REMAP_FRAME_GROUP = 8                          # csrc/dcx_rectify.hip's kFrameGroup: frames one thread remaps with its map entries held

__all__ = ["Rectification", "stereo_rectify_host", "reproject_to_3d", "undistort_points_newton", "undistort_rectify_map_host",
           "undistort_rectify_map_device", "rectify_points_host", "rectify_points_pool", "remap_host", "remap_device",
           "MAP_SENTINEL", "REMAP_FRAME_GROUP"]


class Rectification(NamedTuple):
    R1: np.ndarray               # 3x3: camera 0's frame -> rectified camera 0's
    R2: np.ndarray               # 3x3: camera 1's frame -> rectified camera 1's
    P1: np.ndarray               # 3x4
    P2: np.ndarray               # 3x4, P2[axis, 3] = Tn f
    Q: np.ndarray                # 4x4 disparity -> depth
    axis: int                    # 0: the epipolar lines are rows (a horizontal rig); 1: columns
    Tn: float                    # (R2 T)[axis]: the signed baseline along the rectified axis


# ------------------------------------------------------------------------------------------------ the fp64 steps

def undistort_points_newton(pix, camera_matrix, dist_coeffs) -> np.ndarray:
    """Pixels (N, 2) -> normalised undistorted coordinates (N, 2) by Newton (module docstring, step 3); NaN rows where it has not
    converged within 20 steps."""
    K, k = _camera(camera_matrix), _dist(dist_coeffs)
    pix = np.asarray(pix, np.float64).reshape(-1, 2)
    x0 = (pix[:, 0] - K[0, 2]) / K[0, 0]
    y0 = (pix[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    done = np.zeros(x.shape[0], bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_MAX_ITER):
            xd, yd, _, a, b, d = _distort(x, y, k, True)
            ex, ey = xd - x0, yd - y0
            det = a * d - b * b
            sx, sy = (d * ex - b * ey) / det, (a * ey - b * ex) / det
            live = ~done
            x = np.where(live, x - sx, x)
            y = np.where(live, y - sy, y)
            done |= live & (np.abs(sx) < NEWTON_EPS) & (np.abs(sy) < NEWTON_EPS)
            if done.all():
                break
    out = np.stack([x, y], 1)
    out[~done] = np.nan
    return out


def _rot(R) -> np.ndarray:
    if R is None:
        return np.eye(3)
    R = np.asarray(R, np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError("R must be a finite 3x3 matrix")
    return R


def _newcam(P, K) -> np.ndarray:
    """P (3x3 or 3x4, None: K) -> (fx, fy, cx, cy) of its left 3x3."""
    if P is None:
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    P = np.asarray(P, np.float64)
    if P.shape not in ((3, 3), (3, 4)):
        raise ValueError("P must be 3x3 or 3x4")
    if P[0, 1] != 0.0 or not (np.isfinite(P).all() and P[0, 0] != 0.0 and P[1, 1] != 0.0):
        raise ValueError("P needs finite entries, no skew and non-zero P[0,0], P[1,1]")
    return np.array([P[0, 0], P[1, 1], P[0, 2], P[1, 2]])


def _rectify_normalised(pix, camera_matrix, dist_coeffs, R, undistort=undistort_points_newton) -> np.ndarray:
    """Pixels -> R undistort(pixel) divided by its z: (N, 2), NaN where Newton has not converged or z <= 0.  ``undistort``: the
    camera model's (pixels, camera_matrix, dist_coeffs) -> normalised points, NaN rows where there is none."""
    n = undistort(pix, camera_matrix, dist_coeffs)
    R = _rot(R)
    X = R[0, 0] * n[:, 0] + R[0, 1] * n[:, 1] + R[0, 2]
    Y = R[1, 0] * n[:, 0] + R[1, 1] * n[:, 1] + R[1, 2]
    Z = R[2, 0] * n[:, 0] + R[2, 1] * n[:, 1] + R[2, 2]
    with np.errstate(all="ignore"):
        out = np.stack([X / Z, Y / Z], 1)
    out[~(Z > 0)] = np.nan
    return out


def _rectify_points(undistort, pix, camera_matrix, dist_coeffs, R, P) -> np.ndarray:
    """Step 3 for the camera model whose ``undistort`` is given (``_rectify_normalised``)."""
    K = _camera(camera_matrix)
    f = _newcam(P, K)
    n = _rectify_normalised(pix, camera_matrix, dist_coeffs, R, undistort)
    return np.stack([f[0] * n[:, 0] + f[2], f[1] * n[:, 1] + f[3]], 1)


def rectify_points_host(pix, camera_matrix, dist_coeffs, R=None, P=None) -> np.ndarray:
    """The definition of step 3: pixels (N, 2) -> rectified pixels (N, 2), float64, NaN rows where undefined."""
    return _rectify_points(undistort_points_newton, pix, camera_matrix, dist_coeffs, R, P)


def _border_pixels(W: int, H: int):
    """Every border pixel centre, edge by edge -> (left, right, top, bottom), each (n, 2)."""
    ys, xs = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    left = np.stack([np.zeros(H), ys], 1)
    right = np.stack([np.full(H, W - 1.0), ys], 1)
    top = np.stack([xs, np.zeros(W)], 1)
    bottom = np.stack([xs, np.full(W, H - 1.0)], 1)
    return left, right, top, bottom


def _edge_extreme(K, d, Rc, W: int, H: int, edge: int, samples: np.ndarray) -> float:
    """The inner rectangle's side on one edge of the source frame (0 left: max x, 1 right: min x, 2 top: max y, 3 bottom: min y) over
    the CONTINUOUS edge: the extreme of the pixel-centre ``samples``, polished by a golden-section search between that pixel's two
    neighbours.  (Between two pixel centres a curved edge passes the extreme sample by up to its curvature / 8: 1e-5 px with
    k1 = -0.25, enough for an output pixel on the frame's side to read just outside the source.)"""
    comp, sign = (0, -1.0) if edge == 0 else (0, 1.0) if edge == 1 else (1, -1.0) if edge == 2 else (1, 1.0)
    n = H if edge < 2 else W
    fixed = 0.0 if edge in (0, 2) else (W - 1.0 if edge == 1 else H - 1.0)

    def val(s):                                   # sign * coordinate at edge parameter s: minimised
        pix = np.array([[fixed, s]]) if edge < 2 else np.array([[s, fixed]])
        return sign * float(_rectify_normalised(pix, K, d, Rc)[0, comp])

    v = sign * samples[:, comp]
    i = int(np.argmin(v))
    best = float(v[i])
    a, b = float(max(i - 1, 0)), float(min(i + 1, n - 1))
    g = 0.5 * (math.sqrt(5.0) - 1.0)
    c, e = b - g * (b - a), a + g * (b - a)
    fc, fe = val(c), val(e)
    for _ in range(60):
        if fc < fe:
            b, e, fe = e, c, fc
            c = b - g * (b - a)
            fc = val(c)
        else:
            a, c, fc = c, e, fe
            e = a + g * (b - a)
            fe = val(e)
        best = min(best, fc, fe)
    return sign * best


def _rectifying_rotations(R, T):
    """Step 1's rotations, which no camera model enters: the rig (R, T) -> (R1, R2, axis, Tn).  Each camera turns half of R towards
    the other, then both turn the baseline onto the image axis it is closer to.  ValueError for a zero or non-finite T."""
    R, T = _rot(R), np.asarray(T, np.float64).reshape(3)
    om = _rvec_of(R)
    r_r = _rodrigues(-0.5 * om)
    t = r_r @ T
    nt = math.sqrt(float(t @ t))
    if not (math.isfinite(nt) and nt > 0):
        raise ValueError("T must be finite and non-zero")
    axis = 0 if abs(t[0]) > abs(t[1]) else 1
    u = np.zeros(3)
    u[axis] = 1.0 if t[axis] > 0 else -1.0
    w = np.cross(t, u)
    nw = math.sqrt(float(w @ w))
    if nw > 0:
        w = w * (math.atan2(nw, abs(t[axis])) / nw)
    wR = _rodrigues(w)
    R1, R2 = wR @ r_r.T, wR @ r_r
    return R1, R2, axis, float((R2 @ T)[axis])


def _projections(f: float, cx: float, cy: float, axis: int, Tn: float):
    """-> (P1, P2, Q) of two rectified cameras with the focal length f and the principal point (cx, cy)."""
    P1 = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]], np.float64)
    P2 = P1.copy()
    P2[axis, 3] = Tn * f
    Q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1.0 / Tn, 0]], np.float64)
    return P1, P2, Q


def stereo_rectify_host(camera0, dist0, camera1, dist1, image_size, R, T, alpha: Optional[float] = None) -> Rectification:
    """The rectifying transforms of a rig (module docstring, step 1).  ``image_size`` = (W, H), shared by both cameras;
    ``alpha``: None (no scaling) or a value in [0, 1].  ValueError for refused cameras, a zero T or a border that cannot be
    undistorted."""
    cams = [(_camera(camera0), dist0), (_camera(camera1), dist1)]
    for _, d in cams:
        _dist(d)
    W, H = int(image_size[0]), int(image_size[1])
    if W < 2 or H < 2:
        raise ValueError("image_size must be (W, H) with both >= 2")
    if alpha is not None and not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha must be None or in [0, 1]")
    R1, R2, axis, Tn = _rectifying_rotations(R, T)

    f = min(cams[0][0][1, 1], cams[1][0][1, 1])
    Rs = (R1, R2)
    corners = np.array([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], np.float64)
    cc = np.zeros(2)
    for (K, d), Rc in zip(cams, Rs):
        n = _rectify_normalised(corners, K, d, Rc)
        if not np.isfinite(n).all():
            raise ValueError("an image corner cannot be undistorted and rectified")
        cc += 0.5 * np.array([(W - 1) / 2 - f * n[:, 0].mean(), (H - 1) / 2 - f * n[:, 1].mean()])
    cx, cy = float(cc[0]), float(cc[1])

    if alpha is not None:
        lo, hi = [], []                     # lower bounds of f (inner rectangles cover the frame), upper bounds (outer ones fit)
        for (K, d), Rc in zip(cams, Rs):
            edges = [_rectify_normalised(e, K, d, Rc) for e in _border_pixels(W, H)]
            allp = np.concatenate(edges)
            if not np.isfinite(allp).all():
                raise ValueError("a border pixel cannot be undistorted and rectified")
            inner = [_edge_extreme(K, d, Rc, W, H, e, edges[e]) for e in range(4)]      # left, right, top, bottom
            lo += [cx / -inner[0], (W - 1 - cx) / inner[1], cy / -inner[2], (H - 1 - cy) / inner[3]]
            hi += [cx / -allp[:, 0].min(), (W - 1 - cx) / allp[:, 0].max(), cy / -allp[:, 1].min(), (H - 1 - cy) / allp[:, 1].max()]
        s0, s1 = max(lo) / f, min(hi) / f
        if not (math.isfinite(s0) and math.isfinite(s1) and s0 > 0 and s1 > 0):
            raise ValueError("the principal point lies outside a rectified frame: alpha cannot be applied")
        a = float(alpha)
        f = f * (s0 * (1.0 - a) + s1 * a)

    P1, P2, Q = _projections(f, cx, cy, axis, Tn)
    return Rectification(R1, R2, P1, P2, Q, axis, Tn)


def reproject_to_3d(Q, xy0, xy1, axis: int) -> np.ndarray:
    """Rectified pixels of one point in camera 0 (N, 2) and camera 1 (N, 2) -> the point in rectified camera 0's frame (N, 3)."""
    Q = np.asarray(Q, np.float64)
    xy0, xy1 = np.asarray(xy0, np.float64).reshape(-1, 2), np.asarray(xy1, np.float64).reshape(-1, 2)
    d = xy0[:, axis] - xy1[:, axis]
    h = np.stack([xy0[:, 0], xy0[:, 1], d, np.ones_like(d)], 1) @ Q.T
    with np.errstate(all="ignore"):
        return h[:, :3] / h[:, 3:4]


def _rectify_map(distort, K, k, R, P, width, height, quantised) -> np.ndarray:
    """Step 2 for the camera (K, k) of the model whose ``distort`` (x, y, k, False) -> (xd, yd, ...) is given."""
    Rm, f = _rot(R), _newcam(P, K)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("width and height must be >= 1")
    x = ((np.arange(width, dtype=np.float64) - f[2]) / f[0])[None, :]
    y = ((np.arange(height, dtype=np.float64) - f[3]) / f[1])[:, None]
    qx = Rm[0, 0] * x + Rm[1, 0] * y + Rm[2, 0]
    qy = Rm[0, 1] * x + Rm[1, 1] * y + Rm[2, 1]
    qz = Rm[0, 2] * x + Rm[1, 2] * y + Rm[2, 2]
    with np.errstate(all="ignore"):
        xd, yd = distort(qx / qz, qy / qz, k, False)[:2]
        mx, my = K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
        ok = (qz > 0) & (np.abs(mx) <= MAP_LIMIT) & (np.abs(my) <= MAP_LIMIT)          # (NaN and inf compare false)
    if not quantised:
        return np.stack([np.where(ok, mx, np.nan), np.where(ok, my, np.nan)], 2)
    scale = float(1 << MAP_BITS)
    out = np.full((height, width, 2), MAP_SENTINEL, np.int32)
    out[..., 0][ok] = np.rint(scale * mx[ok]).astype(np.int32)
    out[..., 1][ok] = np.rint(scale * my[ok]).astype(np.int32)
    return out


def undistort_rectify_map_host(camera_matrix, dist_coeffs, R, P, width: int, height: int, quantised: bool = True) -> np.ndarray:
    """The definition of step 2 -> int32 [height, width, 2] (x, y in 1/32 px, MAP_SENTINEL outside); with ``quantised=False``
    float64 [height, width, 2] source pixels, NaN outside."""
    return _rectify_map(_distort, _camera(camera_matrix), _dist(dist_coeffs), R, P, width, height, quantised)


def remap_host(src, map_, border: int = 0) -> np.ndarray:
    """The definition of step 4: ``src`` uint8 (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3) (a 3-D array whose last axis is 3 is
    one colour frame), ``map_`` int32 (out_h, out_w, 2) -> uint8 of the same leading / channel axes and (out_h, out_w)."""
    src, m = np.asarray(src), np.asarray(map_)
    if src.dtype != np.uint8 or m.dtype != np.int32 or m.ndim != 3 or m.shape[2] != 2:
        raise ValueError("src must be uint8 and the map int32 (out_h, out_w, 2)")
    if not 0 <= int(border) <= 255:
        raise ValueError("border must be in [0, 255]")
    colour = src.ndim == 4 or (src.ndim == 3 and src.shape[-1] == 3)
    single = src.ndim == (3 if colour else 2)
    if src.ndim not in (2, 3, 4) or (src.ndim == 4 and src.shape[-1] != 3):
        raise ValueError("src must be (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3)")
    s = src[None] if single else src
    s = s if colour else s[..., None]                        # (B, H, W, C)
    H, W = s.shape[1], s.shape[2]
    mx, my = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    outside = (m[..., 0] == MAP_SENTINEL) & (m[..., 1] == MAP_SENTINEL)
    x0, y0, fx, fy = mx >> MAP_BITS, my >> MAP_BITS, mx & 31, my & 31
    acc = np.full(s.shape[:1] + m.shape[:2] + s.shape[3:], 512, np.int64)
    for dy, dx, wgt in ((0, 0, (32 - fx) * (32 - fy)), (0, 1, fx * (32 - fy)), (1, 0, (32 - fx) * fy), (1, 1, fx * fy)):
        xx, yy = x0 + dx, y0 + dy
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & ~outside
        tap = s[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        tap = np.where(inside[None, :, :, None], tap, int(border))
        acc += wgt[None, :, :, None] * tap
    out = (acc >> 10).astype(np.uint8)
    out = out if colour else out[..., 0]
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------ the device entry points

def _rp_args(R, P, K):
    import ctypes as C
    r = None if R is None else (C.c_double * 9)(*_rot(R).ravel().tolist())
    p = None
    if P is not None:
        _newcam(P, K)
        P = np.asarray(P, np.float64)
        P4 = np.zeros((3, 4))
        P4[:, :P.shape[1]] = P
        p = (C.c_double * 12)(*P4.ravel().tolist())
    return r, p


# One body per wrapper for both camera models, given as ``pnp``'s wrappers take a model: its ``_camera_args`` and its C entry.

def _map_device(camera_args, entry, camera_matrix, dist_coeffs, R, P, width, height, device, out):
    import torch
    from . import _lib
    from .models._handles import require_cuda
    cam = camera_args(camera_matrix, dist_coeffs)
    r, p = _rp_args(R, P, _camera(camera_matrix))
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("width and height must be >= 1")
    if out is None:
        out = torch.empty((height, width, 2), dtype=torch.int32, device=require_cuda(device))
    if out.dtype != torch.int32 or tuple(out.shape) != (height, width, 2) or not out.is_contiguous() or out.device.type != "cuda":
        raise ValueError(f"out must be a contiguous int32 [{height}, {width}, 2] GPU tensor")
    with torch.cuda.device(out.device):
        _lib.check(getattr(_lib.lib(), entry)(*cam, r, p, width, height, out.data_ptr(), _lib.current_stream()), entry)
    return out


def undistort_rectify_map_device(camera_matrix, dist_coeffs, R, P, width: int, height: int, device="cuda", out=None):
    """``undistort_rectify_map_host`` on the GPU -> int32 device tensor [height, width, 2] (``out``: that tensor, preallocated and
    contiguous).  Enqueued on the current stream; nothing is allocated when ``out`` is given.  Equal to the host map except where
    32 m is within rounding of a half-integer (the two sum in different orders), and there by 1."""
    return _map_device(pnp._camera_args, "dcx_undistort_rectify_map", camera_matrix, dist_coeffs, R, P, width, height, device, out)


def _points_pool(camera_args, entry, packed, batch, pool, refined, camera_matrix, dist_coeffs, R, P, out):
    import torch
    from . import _lib
    dev = packed.device
    batch, pool = int(batch), int(pool)
    rows_p, xy_p = pnp._pool_ptrs(packed, batch, pool, refined)[2:]
    cam = camera_args(camera_matrix, dist_coeffs)
    r, p = _rp_args(R, P, _camera(camera_matrix))
    out = _dev.tensor(out, dev, torch.float64, (pool, 2), f"out must be a contiguous float64 [{pool}, 2] tensor on {dev}", "numel")
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), entry)(rows_p, xy_p, pool, *cam, r, p, out.data_ptr() if pool else None,
                                              _lib.current_stream()), entry)
    return out


def rectify_points_pool(packed, batch: int, pool: int, refined: bool, camera_matrix, dist_coeffs, R=None, P=None, out=None):
    """Every slot of a corner pool (``pnp.solve_pnp_pool``'s conventions: ``refined`` takes RefineNet's xy, else the integer x, y of
    the rows) in rectified coordinates, read in place -> float64 device tensor [pool, 2] by slot (``out``: that tensor,
    preallocated); NaN where ``rectify_points_host`` gives NaN.  Slots of no frame are converted too (whatever they hold).
    Enqueued on the current stream, no host sync, nothing allocated when ``out`` is given (capture-safe)."""
    return _points_pool(pnp._camera_args, "dcx_rectify_points_pool", packed, batch, pool, refined, camera_matrix, dist_coeffs, R, P,
                        out)


def remap_device(frames, map_, border: int = 0, out=None):
    """``remap_host`` on the GPU: ``frames`` a uint8 GPU tensor (B, H, W), (H, W), (B, H, W, 3) or (H, W, 3) (a 3-D tensor whose last
    axis is 3 is one colour frame) whose pixels are contiguous (any row pitch and frame stride), ``map_`` a contiguous int32 GPU
    tensor (out_h, out_w, 2) -> uint8 tensor of the same leading / channel axes and (out_h, out_w), contiguous (``out``: that
    tensor, preallocated).  One launch on the current stream, no host sync, nothing allocated when ``out`` is given
    (capture-safe).  A rectified batch feeds ``infer_batch`` / ``ResidentStream`` as any batch of frames does."""
    import torch
    from . import _lib
    if frames.device.type != "cuda" or frames.dtype != torch.uint8 or frames.ndim not in (2, 3, 4):
        raise ValueError("frames must be a uint8 GPU tensor (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3)")
    if frames.ndim == 4 and frames.shape[-1] != 3:
        raise ValueError("colour frames must be (B, H, W, 3)")
    dev = frames.device
    colour = frames.ndim == 4 or (frames.ndim == 3 and frames.shape[-1] == 3)
    single = frames.ndim == (3 if colour else 2)
    x = frames[None] if single else frames
    ch = 3 if colour else 1
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if B < 1 or H < 1 or W < 1:
        raise ValueError("frames must not be empty")
    frames_p, frame_stride, pitch = _dev.u8_frames(x, ch)[:3]
    if (map_.device != dev or map_.dtype != torch.int32 or map_.ndim != 3 or map_.shape[2] != 2 or not map_.is_contiguous()
            or map_.numel() == 0):
        raise ValueError(f"the map must be a contiguous int32 (out_h, out_w, 2) tensor on {dev}")
    if not 0 <= int(border) <= 255:
        raise ValueError("border must be in [0, 255]")
    oh, ow = int(map_.shape[0]), int(map_.shape[1])
    shape = ((B,) if not single else ()) + (oh, ow) + ((3,) if colour else ())
    out = _dev.tensor(out, dev, torch.uint8, shape, f"out must be a contiguous uint8 {shape} tensor on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_remap_u8(frames_p, frame_stride, pitch, H, W, ch, map_.data_ptr(), oh, ow, B, int(border),
                                           out.data_ptr(), _lib.current_stream()), "dcx_remap_u8")
    return out
