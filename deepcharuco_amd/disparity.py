"""Dense stereo matching without OpenCV: semi-global matching over census costs on a rectified pair (what a cv2 user does with
``StereoSGBM`` after ``rectify.remap_device``), a speckle filter for disparity maps (``cv2.filterSpeckles``) and the disparity map
as 3-D points (``cv2.reprojectImageTo3D``), on the host and on the GPU (csrc/dcx_sgm.hip, csrc/dcx_speckle.hip).  Every step of
the matcher and of the filter is integer, so the device equals ``sgm_host`` and ``filter_speckles_host`` bit for bit.

Conventions: ``left`` is rectified camera 0 and ``right`` rectified camera 1 of a horizontal rig (``Rectification.axis == 0``), the
disparity d = x_left - x_right is ``rectify.reproject_to_3d``'s d.  A vertical rig (``axis == 1``) passes both frames transposed
(and transposes the result back); nothing else is done for it.  The output is cv2's: int16, the disparity times 16, invalid
pixels hold 16 (min_disparity - 1).

With m = min_disparity, D = num_disparities and d in [0, D) the candidate (the disparity itself is m + d):

1. census, 9 wide x 7 tall, 62 bits in a uint64: rows top to bottom, columns left to right, the centre skipped; at each neighbour
   the word is shifted left by one and ``neighbour < centre`` ORed in.  A neighbour outside the image reads the edge-replicated
   pixel.
2. cost C(y, x, d) = popcount(cenL[y, x] ^ cenR[y, clamp(x - m - d, 0, W - 1)]).  The clamp keeps the volume dense; step 5 removes
   the winners that relied on it.
3. four paths (left -> right, right -> left, top -> bottom, bottom -> top):
   L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d - 1) + P1, L_r(q, d + 1) + P1, M + P2) - M, q the previous pixel of the path,
   M = min_k L_r(q, k); a term with d +- 1 outside [0, D) is left out; at a path's first pixel L_r = C.  S = sum_r L_r
   <= 4 (62 + 255) = 1268.
   With ``paths=8`` S also receives the four diagonal paths, whose directions (dy, dx) are (+1, +1), (-1, -1), (+1, -1) and
   (-1, +1): the same recursion with q = p - (dy, dx); a pixel whose q lies outside the frame is a path's first pixel (L_r = C),
   so in a 1 x W or H x 1 frame every diagonal has one pixel.  S <= 8 (62 + 255) = 2536: still a u16, and S << 16 | d a word.
   Steps 4 - 7 read that larger S unchanged (the uniqueness rule is a ratio).  ``paths=4`` is the default.
4. the winner d* = argmin_d S, the lowest d on ties.
5. a pixel is invalid if x - m - d* lies outside [0, W); or (cv2's uniqueness rule) some d with |d - d*| > 1 has
   S[d] (100 - uniqueness) < S[d*] 100; or, with lr_max_diff >= 0, |dR(x - m - d*) - d*| > lr_max_diff, where for a right pixel xr
   dR(xr) = argmin_d S(y, xr + m + d, d) over the d whose column lies in [0, W), the lowest d on ties (the right view's winner made
   from the same S, as cv2 does).
6. sub-pixel: with 0 < d* < D - 1, num = S[d*-1] - S[d*+1], den = S[d*-1] + S[d*+1] - 2 S[d*]; den > 0 gives
   off = floor((16 num + den) / (2 den)) (a FLOOR division: the parabola's offset in sixteenths, rounded half up, in [-8, 8]), else
   off = 0.  The output is 16 (m + d*) + off.
7. with speckle_window_size > 0, the speckle filter on that map: ``filter_speckles_host`` with new_val = 16 (m - 1),
   max_speckle_size = speckle_window_size and max_diff = 16 speckle_range, as cv2's ``StereoSGBM`` calls ``filterSpeckles``.

The speckle filter (``filter_speckles_host``, cv2.filterSpeckles): pixels equal to new_val are never touched and belong to no
component.  Among the others, two 4-neighbours p, q of one frame are joined when |disp16[p] - disp16[q]| <= max_diff (in at least
32 bits); the components are the connected components of that graph (connectivity is transitive: a ramp whose neighbours differ
by max_diff is one component however far its ends are apart); every pixel of a component of at most max_speckle_size pixels
becomes new_val.  The result depends on the component sizes only, so on no order of visiting.

Deviations from cv2.StereoSGBM, on purpose: census costs instead of Birchfield-Tomasi on Sobel-filtered images (integer, no
pre-filter cap to tune, and two popcounts per candidate); P2 fixed rather than scaled by the local gradient; four paths by
default and eight with ``paths=8`` (MODE_HH's directions; MODE_SGBM's five and the 16 of the literature are not built); no
pre-filter cap.  Eight paths are an option and no general gain: on a depth edge that runs diagonally they leave fewer wrong
pixels, on an axis-aligned rectangle slightly more, since the diagonals cross its corners (DESIGN 3.13b has both figures).

``min_disparity`` must keep every output inside an int16: -2047 <= m and m + D <= 2047.
"""
from __future__ import annotations

import numpy as np

from . import _dev

CENSUS_W, CENSUS_H = 9, 7
DISPARITY_SHIFT = 4                          # fractional bits of an output value
NUM_DISPARITIES = (64, 128, 256)
PATHS = (4, 8)                               # aggregation paths: the axis-aligned four, or those and the four diagonals
MAX_DEVICE_WIDTH = 4096                      # csrc/dcx_sgm.hip keeps a row's right-view winners in LDS

MAX_SPECKLE_PIXELS = 1 << 30                 # csrc/dcx_speckle.hip labels a frame's pixels with 32-bit indices
MAX_SPECKLE_SIDE = 1 << 20                   # and walks a frame's tiles in one grid

__all__ = ["census_host", "cost_volume_host", "aggregate_host", "select_host", "sgm_host", "filter_speckles_host",
           "disparity_to_points_host", "sgm_workspace_bytes", "sgm_device", "filter_speckles_workspace_bytes",
           "filter_speckles_device", "disparity_to_points_device", "NUM_DISPARITIES", "PATHS", "MAX_DEVICE_WIDTH"]


def _params(min_disparity, num_disparities, p1, p2, uniqueness, lr_max_diff):
    vals = (min_disparity, num_disparities, p1, p2, uniqueness, lr_max_diff)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
        raise ValueError("the matcher's parameters must be integers")
    m, D, p1, p2, u, lr = (int(v) for v in vals)
    if D not in NUM_DISPARITIES:
        raise ValueError(f"num_disparities must be one of {NUM_DISPARITIES}")
    if not 0 <= p1 <= p2 <= 255:
        raise ValueError("0 <= p1 <= p2 <= 255 is required")
    if not 0 <= u < 100:
        raise ValueError("uniqueness must be in [0, 100)")
    if m < -2047 or m + D > 2047:
        raise ValueError("min_disparity must keep 16 (m - 1) and 16 (m + D) inside an int16: -2047 <= m, m + D <= 2047")
    return m, D, p1, p2, u, max(lr, -1)


def _paths(paths) -> int:
    if isinstance(paths, bool) or not isinstance(paths, (int, np.integer)) or int(paths) not in PATHS:
        raise ValueError(f"paths must be one of {PATHS}")
    return int(paths)


def _speckle_params(new_val, max_speckle_size, max_diff):
    vals = (new_val, max_speckle_size, max_diff)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
        raise ValueError("the speckle filter's parameters must be integers")
    nv, size, diff = (int(v) for v in vals)
    if not -32768 <= nv <= 32767:
        raise ValueError("new_val must be an int16 value")
    if size < 0:
        raise ValueError("max_speckle_size must not be negative")
    if not 0 <= diff <= 65535:
        raise ValueError("0 <= max_diff <= 65535 is required")
    return nv, size, diff


def _sgm_speckle_params(speckle_window_size, speckle_range):
    """-> (max_speckle_size, max_diff) of step 7."""
    vals = (speckle_window_size, speckle_range)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
        raise ValueError("speckle_window_size and speckle_range must be integers")
    size, rng = (int(v) for v in vals)
    if size < 0 or not 0 <= 16 * rng <= 65535:
        raise ValueError("speckle_window_size >= 0 and 0 <= 16 speckle_range <= 65535 are required")
    return size, 16 * rng


# ------------------------------------------------------------------------------------------------ the definition, step by step

def census_host(img) -> np.ndarray:
    """Step 1: uint8 (H, W) -> uint64 (H, W)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.size == 0:
        raise ValueError("census needs a non-empty uint8 (H, W) image")
    H, W = img.shape
    ry, rx = CENSUS_H // 2, CENSUS_W // 2
    pad = np.pad(img, ((ry, ry), (rx, rx)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for dy in range(CENSUS_H):
        for dx in range(CENSUS_W):
            if dy == ry and dx == rx:
                continue
            out = (out << np.uint64(1)) | (pad[dy:dy + H, dx:dx + W] < img).astype(np.uint64)
    return out


def _popcount64(v) -> np.ndarray:
    v = np.ascontiguousarray(v, np.uint64)
    return np.unpackbits(v.view(np.uint8).reshape(v.shape + (8,)), axis=-1).sum(-1, dtype=np.int32)


def cost_volume_host(cen_left, cen_right, min_disparity: int, num_disparities: int) -> np.ndarray:
    """Step 2: two census images (H, W) -> int32 (H, W, D)."""
    H, W = cen_left.shape
    x = np.arange(W)[:, None] - int(min_disparity) - np.arange(int(num_disparities))[None, :]
    return _popcount64(cen_left[:, :, None] ^ cen_right[:, np.clip(x, 0, W - 1)])


def _path(C, p1: int, p2: int, reverse: bool, first=None) -> np.ndarray:
    """One path along axis 1 of C (N, n, D) -> L of the same shape.  ``first`` bool (N, n): the pixels, beside each line's first,
    at which a path begins (L = C)."""
    n, D = C.shape[1], C.shape[2]
    big = np.int32(1 << 20)
    L = np.empty_like(C)
    order = range(n - 1, -1, -1) if reverse else range(n)
    prev = None
    for i in order:
        if prev is None:
            cur = C[:, i].copy()
        else:
            M = prev.min(1, keepdims=True)
            lo = np.concatenate([np.full((prev.shape[0], 1), big, np.int32), prev[:, :-1]], 1) + p1      # L(q, d - 1) + P1
            hi = np.concatenate([prev[:, 1:], np.full((prev.shape[0], 1), big, np.int32)], 1) + p1       # L(q, d + 1) + P1
            cur = C[:, i] + np.minimum(np.minimum(prev, lo), np.minimum(hi, M + p2)) - M
            if first is not None:
                cur = np.where(first[:, i, None], C[:, i], cur)
        L[:, i] = cur
        prev = cur
    return L


def _diagonals(C, p1: int, p2: int, slope: int) -> np.ndarray:
    """The two paths of one diagonal family, (dy, dx) = (+1, slope) and (-1, -slope), summed: C (H, W, D) -> (H, W, D).  The
    frame's diagonals are laid end to end on W lines of H pixels: line c holds, at row y, the pixel of column (c + slope y) mod W,
    and wherever the previous pixel of a path, p - (dy, dx), lies outside the frame a new path begins.  Every pixel is on exactly
    one line."""
    H, W, _ = C.shape
    y = np.broadcast_to(np.arange(H)[None, :], (W, H))
    x = (np.arange(W)[:, None] + slope * y) % W
    lines = C[y, x]                                                          # (W, H, D)
    out = np.zeros_like(C)
    for reverse in (False, True):
        dy, dx = (-1, -slope) if reverse else (1, slope)
        first = (y - dy < 0) | (y - dy >= H) | (x - dx < 0) | (x - dx >= W)
        out[y, x] += _path(lines, p1, p2, reverse, first)
    return out


def aggregate_host(C, p1: int, p2: int, paths: int = 4) -> np.ndarray:
    """Step 3: the cost volume int32 (H, W, D) -> S int32 (H, W, D), the sum of the four paths, or with ``paths=8`` of those and
    the four diagonal ones."""
    paths = _paths(paths)
    C = np.ascontiguousarray(C, np.int32)
    Ct = np.ascontiguousarray(C.transpose(1, 0, 2))
    S = _path(C, p1, p2, False) + _path(C, p1, p2, True)
    S += (_path(Ct, p1, p2, False) + _path(Ct, p1, p2, True)).transpose(1, 0, 2)
    if paths == 8:
        S += _diagonals(C, p1, p2, 1) + _diagonals(C, p1, p2, -1)
    return S


def select_host(S, min_disparity: int, uniqueness: int, lr_max_diff: int) -> np.ndarray:
    """Steps 4 - 6: S int (H, W, D) -> int16 (H, W)."""
    S = np.asarray(S).astype(np.int64)
    H, W, D = S.shape
    m, u, lr = int(min_disparity), int(uniqueness), int(lr_max_diff)
    d = np.arange(D)
    best = S.argmin(2)                                                       # (the first minimum: the lowest d)
    Sb = np.take_along_axis(S, best[..., None], 2)[..., 0]
    x = np.arange(W)[None, :]
    xr = x - m - best
    valid = (xr >= 0) & (xr < W)
    far = np.abs(d[None, None, :] - best[..., None]) > 1
    valid &= ~(far & (S * (100 - u) < Sb[..., None] * 100)).any(2)
    if lr >= 0:
        col = np.arange(W)[:, None] + m + d[None, :]                         # (xr, d) -> the left column
        inside = (col >= 0) & (col < W)
        SR = np.where(inside[None], S[:, np.clip(col, 0, W - 1), d[None, :]], np.iinfo(np.int64).max)
        dR = SR.argmin(2)                                                    # (H, W) by xr
        valid &= np.abs(np.take_along_axis(dR, np.clip(xr, 0, W - 1), 1) - best) <= lr
    lo = np.take_along_axis(S, np.clip(best - 1, 0, D - 1)[..., None], 2)[..., 0]
    hi = np.take_along_axis(S, np.clip(best + 1, 0, D - 1)[..., None], 2)[..., 0]
    num, den = lo - hi, lo + hi - 2 * Sb
    sub = (best > 0) & (best < D - 1) & (den > 0)
    off = np.where(sub, (16 * num + den) // np.where(sub, 2 * den, 1), 0)    # (numpy's // on integers is a floor division)
    out = np.where(valid, 16 * (m + best) + off, 16 * (m - 1))
    return out.astype(np.int16)


def _components(disp, new_val: int, max_diff: int):
    """One frame int16 (H, W) -> (alive bool (H W), root int64 (H W)): the component of pixel p is named by its smallest pixel
    index, root[p] (p itself where p is not alive).  Union-find over all edges at once: every round hooks, for each edge whose
    ends have different roots, the larger root under the smaller (the smallest wins where several ask), then follows every pixel's
    entry until each points at a root.  A pixel's entry never grows and some root is hooked in every round but the last."""
    H, W = disp.shape
    v = disp.astype(np.int64).ravel()
    alive = v != new_val
    idx = np.arange(H * W).reshape(H, W)
    ends = []
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        a, b = a.ravel(), b.ravel()
        join = alive[a] & alive[b] & (np.abs(v[a] - v[b]) <= max_diff)
        ends.append((a[join], b[join]))
    a, b = np.concatenate([e[0] for e in ends]), np.concatenate([e[1] for e in ends])
    root = np.arange(H * W)
    while True:
        while True:
            up = root[root]
            if np.array_equal(up, root):
                break
            root = up
        ra, rb = root[a], root[b]
        apart = ra != rb
        if not apart.any():
            return alive, root
        np.minimum.at(root, np.maximum(ra, rb)[apart], np.minimum(ra, rb)[apart])


def filter_speckles_host(disp16, new_val: int, max_speckle_size: int, max_diff: int) -> np.ndarray:
    """The speckle filter's definition (module docstring; ``cv2.filterSpeckles``): ``disp16`` int16 (H, W) or (B, H, W), each
    frame on its own -> a copy of the same shape in which every pixel of a component of at most ``max_speckle_size`` pixels holds
    ``new_val``.  ``new_val`` an int16 value, ``max_speckle_size`` >= 0 (0 changes nothing), 0 <= ``max_diff`` <= 65535, all
    integers; ValueError otherwise."""
    nv, size, diff = _speckle_params(new_val, max_speckle_size, max_diff)
    disp16 = np.asarray(disp16)
    if disp16.dtype != np.int16 or disp16.ndim not in (2, 3) or disp16.size == 0:
        raise ValueError("disp16 must be a non-empty int16 array (H, W) or (B, H, W)")
    if disp16.ndim == 3:
        return np.stack([filter_speckles_host(f, nv, size, diff) for f in disp16])
    alive, root = _components(disp16, nv, diff)
    count = np.bincount(root[alive], minlength=root.size)
    out = disp16.copy()
    out.reshape(-1)[alive & (count[root] <= size)] = nv
    return out


def sgm_host(left, right, min_disparity: int = 0, num_disparities: int = 64, p1: int = 7, p2: int = 86, uniqueness: int = 10,
             lr_max_diff: int = 1, speckle_window_size: int = 0, speckle_range: int = 0, paths: int = 4) -> np.ndarray:
    """The definition (module docstring): ``left``, ``right`` uint8 (H, W) or (B, H, W), rectified on a horizontal rig, ``left``
    camera 0 -> int16 of the same shape, the disparity times 16, 16 (min_disparity - 1) where invalid.  A vertical rig passes
    transposed frames.  ``lr_max_diff`` < 0 switches the left-right check off; ``speckle_window_size`` > 0 switches the speckle
    filter (step 7) on; ``paths`` is 4 or 8 (step 3).  ValueError for anything else that the module docstring does not allow."""
    m, D, p1, p2, u, lr = _params(min_disparity, num_disparities, p1, p2, uniqueness, lr_max_diff)
    size, diff = _sgm_speckle_params(speckle_window_size, speckle_range)
    paths = _paths(paths)
    left, right = np.asarray(left), np.asarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.shape != right.shape or left.ndim not in (2, 3) or left.size == 0:
        raise ValueError("left and right must be non-empty uint8 arrays of one shape, (H, W) or (B, H, W)")
    if left.ndim == 3:
        return np.stack([sgm_host(a, b, m, D, p1, p2, u, lr, size, diff // 16, paths) for a, b in zip(left, right)])
    C = cost_volume_host(census_host(left), census_host(right), m, D)
    out = select_host(aggregate_host(C, p1, p2, paths), m, u, lr)
    return filter_speckles_host(out, 16 * (m - 1), size, diff) if size > 0 else out


def _q44(Q) -> np.ndarray:
    Q = np.asarray(Q, np.float64)
    if Q.shape != (4, 4) or not np.isfinite(Q).all():
        raise ValueError("Q must be a finite 4x4 matrix")
    return Q


def disparity_to_points_host(disp16, Q, min_disparity: int = 0) -> np.ndarray:
    """A disparity map int16 (..., H, W) -> float64 (..., H, W, 3): for pixel (x, y) with d = disp16 / 16 the point
    Q (x, y, d, 1)^T dehomogenised, each row of Q summed left to right: ``rectify.reproject_to_3d(Q, (x, y), (x - d, y), 0)``.
    NaN where the pixel is invalid (disp16 < 16 min_disparity) or d == 0."""
    Q = _q44(Q)
    disp16 = np.asarray(disp16)
    if disp16.dtype != np.int16 or disp16.ndim < 2:
        raise ValueError("disp16 must be int16 (..., H, W)")
    H, W = disp16.shape[-2:]
    x = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], disp16.shape)
    y = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], disp16.shape)
    d = disp16.astype(np.float64) / 16.0
    h = [((Q[i, 0] * x + Q[i, 1] * y) + Q[i, 2] * d) + Q[i, 3] for i in range(4)]
    with np.errstate(all="ignore"):
        out = np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], -1)
    out[(disp16 < 16 * int(min_disparity)) | (disp16 == 0)] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ the device entry points

def sgm_workspace_bytes(batch: int, height: int, width: int, num_disparities: int) -> int:
    """Bytes of device workspace with which ``sgm_device`` takes the whole batch in one chunk: per frame two census images and S
    (u16), H W (16 + 2 D).  A smaller workspace that holds at least one frame is accepted and the batch is chunked."""
    from . import _lib
    n = int(_lib.lib().dcx_sgm_workspace_bytes(int(batch), int(height), int(width), int(num_disparities)))
    if n == 0:
        raise ValueError("refused shape: batch, height >= 1, 1 <= width <= 4096 and num_disparities in (64, 128, 256) are required")
    return n


def sgm_device(left, right, min_disparity: int = 0, num_disparities: int = 64, p1: int = 7, p2: int = 86, uniqueness: int = 10,
               lr_max_diff: int = 1, out=None, workspace=None, speckle_window_size: int = 0, speckle_range: int = 0,
               paths: int = 4):
    """``sgm_host`` on the GPU: ``left``, ``right`` uint8 GPU tensors (H, W) or (B, H, W) of one shape whose rows are contiguous
    (any row pitch and frame stride, each tensor its own) -> int16 tensor of the same shape, contiguous (``out``: that tensor,
    preallocated).  ``workspace``: a uint8 GPU tensor of ``sgm_workspace_bytes`` bytes, or fewer but at least one frame's (the batch
    is then taken in chunks); allocated when None.  Enqueued on the current stream, no host sync, deterministic; nothing is
    allocated when ``out`` and ``workspace`` are given (capture-safe).  Equal to ``sgm_host`` bit for bit.  width <= 4096.
    With ``speckle_window_size`` > 0 the speckle filter (step 7) follows on the same stream, in place on ``out`` and in the same
    workspace, which the matcher is done with by then and which holds at least 18 frames of the filter's per frame of its own.
    ``paths=8`` adds the diagonal paths' two launches per chunk; the workspace is the same."""
    import torch
    from . import _lib
    m, D, p1, p2, u, lr = _params(min_disparity, num_disparities, p1, p2, uniqueness, lr_max_diff)
    size, diff = _sgm_speckle_params(speckle_window_size, speckle_range)
    paths = _paths(paths)
    for t in (left, right):
        if t.device.type != "cuda" or t.dtype != torch.uint8 or t.ndim not in (2, 3):
            raise ValueError("left and right must be uint8 GPU tensors (H, W) or (B, H, W)")
    if left.shape != right.shape or left.device != right.device or left.numel() == 0:
        raise ValueError("left and right must be non-empty, of one shape and on one device")
    dev = left.device
    single = left.ndim == 2
    (pl, fl, tl, B, H, W), (pr, fr, tr, _, _, _) = (_dev.u8_frames(t[None] if single else t, unit_axes_free=True) for t in (left, right))
    if W > MAX_DEVICE_WIDTH:
        raise ValueError(f"sgm_device takes frames up to {MAX_DEVICE_WIDTH} wide")
    shape = tuple(left.shape)
    out = _dev.tensor(out, dev, torch.int16, shape, f"out must be a contiguous int16 {shape} tensor on {dev}")
    if workspace is None:
        workspace = torch.empty(sgm_workspace_bytes(B, H, W, D), dtype=torch.uint8, device=dev)
    _dev.workspace(workspace, dev, 0, f"workspace must be a contiguous, 8-byte aligned uint8 tensor on {dev}", aligned_u8=True)
    if workspace.numel() < sgm_workspace_bytes(1, H, W, D):
        raise ValueError("the workspace does not hold one frame: see sgm_workspace_bytes(1, height, width, num_disparities)")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_sgm_u8_paths(pl, fl, tl, pr, fr, tr, B, H, W, m, D, p1, p2, u, lr, paths, out.data_ptr(),
                                               workspace.data_ptr(), workspace.numel(), _lib.current_stream()), "dcx_sgm_u8_paths")
        if size > 0:
            _lib.check(_lib.lib().dcx_filter_speckles_s16(out.data_ptr(), out.data_ptr(), B, H, W, 16 * (m - 1), size, diff,
                                                          workspace.data_ptr(), workspace.numel(), _lib.current_stream()),
                       "dcx_filter_speckles_s16")
    return out


def filter_speckles_workspace_bytes(batch: int, height: int, width: int) -> int:
    """Bytes of device workspace with which ``filter_speckles_device`` takes the whole batch in one chunk: a 32-bit label and a
    32-bit size per pixel, 8 H W per frame.  A smaller workspace that holds at least one frame is accepted and the batch is chunked."""
    from . import _lib
    n = int(_lib.lib().dcx_filter_speckles_workspace_bytes(int(batch), int(height), int(width)))
    if n == 0:
        raise ValueError(f"refused shape: batch >= 1, 1 <= height, width <= {MAX_SPECKLE_SIDE} and height * width <= "
                         f"{MAX_SPECKLE_PIXELS} are required")
    return n


def filter_speckles_device(disp16, new_val: int, max_speckle_size: int, max_diff: int, out=None, workspace=None):
    """``filter_speckles_host`` on the GPU: ``disp16`` a contiguous int16 GPU tensor (H, W) or (B, H, W) -> int16 tensor of the
    same shape (``out``: that tensor, preallocated and contiguous; it may be ``disp16`` itself, any other overlap is the caller's
    error).  ``workspace``: a uint8 GPU tensor of ``filter_speckles_workspace_bytes`` bytes, or fewer but at least one frame's (the
    batch is then taken in chunks); allocated when None.  Four launches per chunk on the current stream, no host sync; nothing is
    allocated when ``out`` and ``workspace`` are given (capture-safe).  Equal to ``filter_speckles_host`` bit for bit."""
    import torch
    from . import _lib
    nv, size, diff = _speckle_params(new_val, max_speckle_size, max_diff)
    if disp16.device.type != "cuda" or disp16.dtype != torch.int16 or disp16.ndim not in (2, 3) or not disp16.is_contiguous() \
            or disp16.numel() == 0:
        raise ValueError("disp16 must be a non-empty contiguous int16 GPU tensor (H, W) or (B, H, W)")
    dev = disp16.device
    shape = tuple(disp16.shape)
    B = int(shape[0]) if disp16.ndim == 3 else 1
    H, W = int(shape[-2]), int(shape[-1])
    one = filter_speckles_workspace_bytes(1, H, W)
    out = _dev.tensor(out, dev, torch.int16, shape, f"out must be a contiguous int16 {shape} tensor on {dev}")
    if workspace is None:
        workspace = torch.empty(B * one, dtype=torch.uint8, device=dev)
    _dev.workspace(workspace, dev, 0, f"workspace must be a contiguous, 8-byte aligned uint8 tensor on {dev}", aligned_u8=True)
    if workspace.numel() < one:
        raise ValueError("the workspace does not hold one frame: see filter_speckles_workspace_bytes(1, height, width)")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_filter_speckles_s16(disp16.data_ptr(), out.data_ptr(), B, H, W, nv, size, diff,
                                                      workspace.data_ptr(), workspace.numel(), _lib.current_stream()),
                   "dcx_filter_speckles_s16")
    return out


def disparity_to_points_device(disp16, Q, min_disparity: int = 0, out=None):
    """``disparity_to_points_host`` on the GPU: ``disp16`` a contiguous int16 GPU tensor (H, W) or (B, H, W) -> float32 tensor
    (..., H, W, 3) (``out``: that tensor, preallocated and contiguous).  fp64 in the host definition's order, rounded to float32
    once, at the store.  One launch on the current stream; nothing is allocated when ``out`` is given."""
    import ctypes as C
    import torch
    from . import _lib
    Q = _q44(Q)
    if disp16.device.type != "cuda" or disp16.dtype != torch.int16 or disp16.ndim not in (2, 3) or not disp16.is_contiguous() \
            or disp16.numel() == 0:
        raise ValueError("disp16 must be a non-empty contiguous int16 GPU tensor (H, W) or (B, H, W)")
    m = int(min_disparity)
    if m < -2047 or m > 2047:
        raise ValueError("min_disparity must be in [-2047, 2047]")
    dev = disp16.device
    shape = tuple(disp16.shape) + (3,)
    out = _dev.tensor(out, dev, torch.float32, shape, f"out must be a contiguous float32 {shape} tensor on {dev}")
    B = int(disp16.shape[0]) if disp16.ndim == 3 else 1
    H, W = int(disp16.shape[-2]), int(disp16.shape[-1])
    q = (C.c_double * 16)(*Q.ravel().tolist())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dcx_disparity_to_points(disp16.data_ptr(), B, H, W, m, q, out.data_ptr(), _lib.current_stream()),
                   "dcx_disparity_to_points")
    return out
