"""Image resizing without OpenCV (``cv2.resize``: INTER_NEAREST, INTER_LINEAR, INTER_AREA by integer and by fractional factors) on the
host and on the GPU (csrc/dcx_resize.hip), the way between the resized frame's pixels and the camera's, and the detector behind a resize.  The
networks are trained on 320 x 240 frames; the reference's callers shrink theirs with ``cv2.resize(..., INTER_LINEAR)`` first
(src/inference.py:135).  Here a batch that already lies on the GPU (a ``ResidentStream``'s decoded frames, a rectified batch out
of ``remap_device``) gets there in one launch.

``resize_host`` is the definition and ``resize_device`` equals it bit for bit.  The formulas are cv2's as published (imgproc's
resize.cpp: the 11-bit fixed-point INTER_LINEAR of 8-bit images, its rule that an exact 2 x 2 reduction is INTER_AREA, the
integer-factor INTER_AREA, computeResizeAreaTab and the general area invoker, INTER_NEAREST).  cv2 cannot be run where this package is tested, so they are NOT pinned against cv2.

With (sh, sw) the source and (dh, dw) the output size, channels independent:

* ``"nearest"``: sx = min(floor(dx * (1.0 / (dw / sw))), sw - 1), the same in y, all float64.
* ``"area"``: only sw = fx dw and sh = fy dh with integers 1 <= fx, fy <= 64 (ValueError otherwise).  sum = the integer sum of the
  fx fy source pixels; fx = fy = 2: out = (sum + 2) >> 2; otherwise out = rint(float32(sum) * float32(1.0 / (fx fy))), ties to even
  (float32(sum) is exact).
* ``"linear"``: sw = 2 dw and sh = 2 dh gives ``"area"``'s result (cv2's rule).  Otherwise per axis scale = 1.0 / (dn / sn),
  f = float32((d + 0.5) * scale - 0.5) (product and difference each rounded to float64, no fused multiply-add), s = floor(f),
  f = f - float32(s) in float32.  In x: s < 0 gives f = 0, s = 0; s >= sw - 1 gives f = 0, s = sw - 1; the second tap is
  min(s + 1, sw - 1).  In y the two rows are clip(s, 0, sh - 1) and clip(s + 1, 0, sh - 1) and f is kept.  Coefficients
  c0 = rint(float32(1 - f) * 2048), c1 = rint(f * 2048) in float32, ties to even, each rounded on its own (they need not sum to
  2048).  Horizontal pass, int32: r = S[x0] a0 + S[x1] a1.  Vertical: out = (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2.
  The result stays in 0..255 and within 0.78 gray levels of float64 bilinear interpolation.
* ``"area_any"``: cv2's general INTER_AREA for shrinking, a box filter with fractional end taps.  dh > sh, dw > sw (area does not
  enlarge), sh > 64 dh or sw > 64 dw are refused (ValueError).  It is no code of ``INTERPOLATIONS`` (those are
  ``dcx_resize_u8``'s): the C entry is ``dcx_resize_area_u8``.

  1. Routing (cv2's fast-path rule).  sw = fx dw AND sh = fy dh with integer factors: ``"area"``'s result, bit for bit (identity
     and 2 x 2 included).  Otherwise BOTH axes take the general path, also one whose own factor is an integer.
  2. The tap table of an axis, float64, each operation rounded once, no fused multiply-add, scale = 1.0 / (dn / sn).  For output
     index d: f1 = d * scale, f2 = f1 + scale, cell = min(scale, sn - f1); s1 = ceil(f1), s2 = min(floor(f2), sn - 1),
     s1 = min(s1, s2).  Taps in this order: if s1 - f1 > 1e-3: (s1 - 1, float32((s1 - f1) / cell)); for s in s1 .. s2 - 1:
     (s, float32(1.0 / cell)); if f2 - s2 > 1e-3: (s2, float32(min(min(f2 - s2, 1.0), cell) / cell)).  (An end tap that covers
     1e-3 of its pixel or less is dropped and the others are not renormalised: cv2's rule.)
  3. A pixel, float32 throughout, every product and every sum rounded on its own.  For each y-tap (sy, b) in order:
     h = the sum over the x-taps (sx, a) in order of float32(S[sy, sx]) * a, starting from the first product; v = b * h for the
     first y-tap and v = v + b * h for the others; out = clip(rint(v), 0, 255), ties to even.  Horizontal first, then vertical,
     is part of the definition: it is cv2's order and it fixes the bits.

  Before the final rounding the result is within a few 1e-5 gray levels of the float64 box integral where no sliver is dropped
  (tests/test_resize_any_host.py gates it at 0.5 + 255 n 2^-23 after rounding, n = (ceil(scale_x) + 1)(ceil(scale_y) + 1)).

In front of the detector ``"area_any"`` is the default: ``"linear"`` by an odd integer factor has f = 0 on both axes and reads
ONE source pixel per output pixel, by an even factor the four around the centre (by 4.5, 4 of every 20.25); a thin dark ChArUco
line between them is sampled or missed by where it falls.  ``"area"`` and ``"area_any"`` weigh every source pixel by the share of
it that the output pixel covers; on integer factors they are the same bits, and ``"area_any"`` also takes the 1440 x 1080 window
of a 1080p frame (4.5).

Sizes are (height, width) everywhere in this module; points are (x, y) and ``origin`` is the (x0, y0) of a cropped window.
"""
from __future__ import annotations

import numpy as np

from . import _dev

INTERPOLATIONS = {"nearest": 0, "linear": 1, "area": 2}        # dcx_resize_u8's codes
MAX_SIDE = 32768                                               # every dimension: 1 .. MAX_SIDE
MAX_AREA_FACTOR = 64
AREA_ANY = "area_any"                                          # no code of dcx_resize_u8: its own entry, dcx_resize_area_u8
AREA_ANY_EPS = 1e-3                                            # cv2's rule: an end tap that covers less of its pixel is dropped
COEF_BITS = 11                                                 # cv2's INTER_RESIZE_COEF_BITS

__all__ = ["resize_host", "resize_device", "map_points", "scale_camera_matrix", "infer_batch_resized", "INTERPOLATIONS"]


def _size(size):
    try:
        dh, dw = int(size[0]), int(size[1])
        ok = len(size) == 2 and dh == size[0] and dw == size[1]
    except (TypeError, ValueError, IndexError):
        ok = False
    if not ok or not (1 <= dh <= MAX_SIDE and 1 <= dw <= MAX_SIDE):
        raise ValueError(f"size must be (out_h, out_w) with both in 1..{MAX_SIDE}")
    return dh, dw


def _mode(interpolation):
    """-> the code of ``dcx_resize_u8``, or AREA_ANY itself."""
    if interpolation == AREA_ANY:
        return AREA_ANY
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {sorted(INTERPOLATIONS) + [AREA_ANY]}")
    return INTERPOLATIONS[interpolation]


def _area_factors(sh, sw, dh, dw):
    fy, fx = sh // dh, sw // dw
    if fy * dh != sh or fx * dw != sw or not (1 <= fy <= MAX_AREA_FACTOR and 1 <= fx <= MAX_AREA_FACTOR):
        raise ValueError(f"\"area\" needs integer factors in 1..{MAX_AREA_FACTOR}: {sh}x{sw} -> {dh}x{dw} is refused")
    return fy, fx


def _layout(ndim, last):
    """(colour, single) of a frames array by the rules of ``rectify.remap_host``."""
    colour = ndim == 4 or (ndim == 3 and last == 3)
    return colour, ndim == (3 if colour else 2)


def _linear_axis(dn: int, sn: int, is_x: bool):
    """-> (first tap, second tap, c0, c1) of every output index of one axis (module docstring)."""
    scale = 1.0 / (dn / sn)
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if is_x:
        lo, hi = s < 0, s >= sn - 1
        f[lo | hi] = 0
        s[lo] = 0
        s[hi] = sn - 1
        s0, s1 = s, np.minimum(s + 1, sn - 1)
    else:
        s0, s1 = np.clip(s, 0, sn - 1), np.clip(s + 1, 0, sn - 1)
    one = np.float32(1 << COEF_BITS)
    c0 = np.rint((np.float32(1) - f) * one).astype(np.int32)
    c1 = np.rint(f * one).astype(np.int32)
    return s0, s1, c0, c1


def _nearest_axis(dn: int, sn: int):
    scale = 1.0 / (dn / sn)
    return np.minimum(np.floor(np.arange(dn, dtype=np.float64) * scale).astype(np.int64), sn - 1)


def _area(s, dh, dw):
    B, sh, sw, C = s.shape
    fy, fx = _area_factors(sh, sw, dh, dw)
    total = s.reshape(B, dh, fy, dw, fx, C).astype(np.int64).sum(axis=(2, 4))
    if fx == 2 and fy == 2:
        return ((total + 2) >> 2).astype(np.uint8)
    return np.rint(total.astype(np.float32) * np.float32(1.0 / (fx * fy))).astype(np.uint8)


def _area_any_routes_to_area(sh, sw, dh, dw):
    """``"area_any"``'s refusals (ValueError), then cv2's fast-path rule: integer factors on BOTH axes are ``"area"``'s."""
    if dh > sh or dw > sw:
        raise ValueError(f"\"area_any\" does not enlarge: {sh}x{sw} -> {dh}x{dw} is refused")
    if sh > MAX_AREA_FACTOR * dh or sw > MAX_AREA_FACTOR * dw:
        raise ValueError(f"\"area_any\" reduces by at most {MAX_AREA_FACTOR}: {sh}x{sw} -> {dh}x{dw} is refused")
    return sh % dh == 0 and sw % dw == 0


def _area_any_axis(dn: int, sn: int):
    """The tap table of one axis of ``"area_any"`` (module docstring) -> (index (dn, K) int64, weight (dn, K) float32, count (dn,)):
    row d holds the taps of output index d in order, padded with (0, 0.0) beyond ``count[d]``."""
    scale = 1.0 / (dn / sn)
    f1 = np.arange(dn, dtype=np.float64) * scale
    f2 = f1 + scale
    cell = np.minimum(scale, sn - f1)
    s2 = np.minimum(np.floor(f2), sn - 1)
    s1 = np.minimum(np.ceil(f1), s2)
    first = (s1 - f1) > AREA_ANY_EPS
    last = (f2 - s2) > AREA_ANY_EPS
    w_first = ((s1 - f1) / cell).astype(np.float32)
    w_mid = (1.0 / cell).astype(np.float32)
    w_last = (np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell).astype(np.float32)
    s1, s2 = s1.astype(np.int64), s2.astype(np.int64)
    mid = s2 - s1
    count = first + mid + last
    K = int(count.max())
    k = np.arange(K)[None, :] - first[:, None]                                # position among the whole pixels; -1: the first tap
    is_mid, is_last = (k >= 0) & (k < mid[:, None]), (k == mid[:, None]) & last[:, None]
    index = np.where(k < 0, s1[:, None] - 1, np.where(is_mid, s1[:, None] + k, np.where(is_last, s2[:, None], 0)))
    weight = np.where(k < 0, w_first[:, None], np.where(is_mid, w_mid[:, None], np.where(is_last, w_last[:, None], np.float32(0))))
    return index, weight.astype(np.float32), count.astype(np.int64)


def _tap_sum(values, index, weight, count, axis):
    """Along ``axis`` of float32 ``values``: per output index the first tap's product, then the others added in order, every
    product and every sum rounded to float32 on its own."""
    shape = [1] * values.ndim
    shape[axis] = -1
    acc = None
    for k in range(index.shape[1]):
        prod = np.take(values, index[:, k], axis=axis) * weight[:, k].reshape(shape)
        acc = prod if acc is None else np.where((k < count).reshape(shape), acc + prod, acc)
    assert acc.dtype == np.float32
    return acc


def _area_any(s, dh, dw):
    """The general path of ``"area_any"``: horizontal first, then vertical."""
    h = _tap_sum(s.astype(np.float32), *_area_any_axis(dw, s.shape[2]), axis=2)
    v = _tap_sum(h, *_area_any_axis(dh, s.shape[1]), axis=1)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def resize_host(frames, size, interpolation="linear") -> np.ndarray:
    """The definition (module docstring): ``frames`` uint8 (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3) (a 3-D array whose last
    axis is 3 is one colour frame, as for ``rectify.remap_host``), ``size`` = (out_h, out_w) -> uint8 of the same leading / channel
    axes.  cv2's formulas as published, not pinned against cv2."""
    src = np.asarray(frames)
    dh, dw = _size(size)
    mode = _mode(interpolation)
    if src.dtype != np.uint8 or src.ndim not in (2, 3, 4) or (src.ndim == 4 and src.shape[-1] != 3) or src.size == 0:
        raise ValueError("frames must be a non-empty uint8 (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3) array")
    colour, single = _layout(src.ndim, src.shape[-1])
    s = src[None] if single else src
    s = s if colour else s[..., None]                                          # (B, H, W, C)
    sh, sw = s.shape[1], s.shape[2]
    if sh > MAX_SIDE or sw > MAX_SIDE:
        raise ValueError(f"frames beyond {MAX_SIDE} px a side are refused")
    if mode == AREA_ANY and _area_any_routes_to_area(sh, sw, dh, dw):
        mode = 2
    if mode == 2 or (mode == 1 and sw == 2 * dw and sh == 2 * dh):
        out = _area(s, dh, dw)
    elif mode == AREA_ANY:
        out = _area_any(s, dh, dw)
    elif mode == 0:
        out = s[:, _nearest_axis(dh, sh)][:, :, _nearest_axis(dw, sw)]
    else:
        x0, x1, a0, a1 = _linear_axis(dw, sw, True)
        y0, y1, b0, b1 = _linear_axis(dh, sh, False)
        a0, a1 = a0[None, None, :, None], a1[None, None, :, None]
        b0, b1 = b0[None, :, None, None], b1[None, :, None, None]
        t = s.astype(np.int32)
        r0, r1 = t[:, y0], t[:, y1]
        r0 = r0[:, :, x0] * a0 + r0[:, :, x1] * a1
        r1 = r1[:, :, x0] * a0 + r1[:, :, x1] * a1
        out = ((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
    out = out if colour else out[..., 0]
    return np.ascontiguousarray(out[0] if single else out)


def resize_device(frames, size, interpolation="linear", out=None):
    """``resize_host`` on the GPU, bit for bit: ``frames`` a uint8 GPU tensor (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3) whose
    pixels are contiguous, at any row pitch and frame stride -- a cropped view ``frames[:, y0:y1, x0:x1]`` costs nothing (that is
    how a 16:9 frame gets its 4:3 window), so does a batch taken with a step -> uint8 tensor of the same leading / channel axes and
    ``size``, contiguous (``out``: that tensor, preallocated).  One launch on the current stream, no host sync, nothing allocated
    when ``out`` is given (capture-safe)."""
    import torch
    from . import _lib
    dh, dw = _size(size)
    mode = _mode(interpolation)
    if (not isinstance(frames, torch.Tensor) or frames.device.type != "cuda" or frames.dtype != torch.uint8
            or frames.ndim not in (2, 3, 4)):
        raise ValueError("frames must be a uint8 GPU tensor (H, W), (B, H, W), (H, W, 3) or (B, H, W, 3)")
    if frames.ndim == 4 and frames.shape[-1] != 3:
        raise ValueError("colour frames must be (B, H, W, 3)")
    dev = frames.device
    colour, single = _layout(frames.ndim, frames.shape[-1])
    x = frames[None] if single else frames
    ch = 3 if colour else 1
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if B < 1 or H < 1 or W < 1:
        raise ValueError("frames must not be empty")
    if mode == 2:
        _area_factors(H, W, dh, dw)
    elif mode == AREA_ANY:
        _area_any_routes_to_area(H, W, dh, dw)                                 # (the refusals; the entry routes)
    frames_p, frame_stride, pitch = _dev.u8_frames(x, ch)[:3]
    shape = ((B,) if not single else ()) + (dh, dw) + ((3,) if colour else ())
    out = _dev.tensor(out, dev, torch.uint8, shape, f"out must be a contiguous uint8 {shape} tensor on {dev}")
    with torch.cuda.device(dev):
        if mode == AREA_ANY:
            _lib.check(_lib.lib().dcx_resize_area_u8(frames_p, frame_stride, pitch, H, W, ch, dh, dw, B, out.data_ptr(),
                                                     _lib.current_stream()), "dcx_resize_area_u8")
        else:
            _lib.check(_lib.lib().dcx_resize_u8(frames_p, frame_stride, pitch, H, W, ch, dh, dw, B, mode, out.data_ptr(),
                                                _lib.current_stream()), "dcx_resize_u8")
    return out


def _ratios(src_size, dst_size):
    (sh, sw), (dh, dw) = src_size, dst_size
    if not (sh > 0 and sw > 0 and dh > 0 and dw > 0):
        raise ValueError("sizes must be (height, width), all positive")
    return float(sw) / float(dw), float(sh) / float(dh)


def map_points(xy, src_size, dst_size, origin=(0, 0), inverse=False):
    """Points of the resized frame -> pixels of the source: x_src = (x + 0.5) * sw / dw - 0.5 + x0, the same in y (pixel centres
    sit at the half-integers of the continuous image; ``origin`` = (x0, y0) of the resized window in the source, for a cropped
    view).  ``src_size`` = (sh, sw) is the size of what was resized, ``dst_size`` = (dh, dw) what it was resized to.
    ``inverse=True``: source pixels -> the resized frame, x = (x_src - x0 + 0.5) * dw / sw - 0.5.

    ``xy``: a numpy array (returned as float64) or a torch tensor of a floating dtype (e.g. a corner pool's ``xy`` view; same
    dtype and device, plain tensor ops on the current stream), last axis (x, y[, more]): columns after the first two (an id) are
    kept.  A new array is returned."""
    rx, ry = _ratios(src_size, dst_size)
    x0, y0 = float(origin[0]), float(origin[1])
    if isinstance(xy, np.ndarray) or not hasattr(xy, "clone"):
        out = np.array(xy, dtype=np.float64)
    else:
        if not xy.is_floating_point():
            raise ValueError("a torch tensor of points must have a floating dtype")
        out = xy.clone()
    if out.ndim < 1 or out.shape[-1] < 2:
        raise ValueError("points must have a last axis (x, y[, ...])")
    if inverse:
        out[..., 0] = (out[..., 0] - x0 + 0.5) / rx - 0.5
        out[..., 1] = (out[..., 1] - y0 + 0.5) / ry - 0.5
    else:
        out[..., 0] = (out[..., 0] + 0.5) * rx - 0.5 + x0
        out[..., 1] = (out[..., 1] + 0.5) * ry - 0.5 + y0
    return out


def scale_camera_matrix(K, src_size, dst_size, origin=(0, 0)) -> np.ndarray:
    """The camera matrix of the resized image from the camera's own: fx' = fx dw / sw, cx' = (cx + 0.5 - x0) dw / sw - 0.5, the
    same in y (sizes and ``origin`` as for ``map_points``).  Distortion coefficients act on normalised coordinates and are
    unchanged.  A point projected with K and taken to the resized frame (``map_points(..., inverse=True)``) is the point projected
    with the result."""
    rx, ry = _ratios(src_size, dst_size)
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be 3x3")
    x0, y0 = float(origin[0]), float(origin[1])
    out = K.copy()
    out[0, 0], out[0, 1] = K[0, 0] / rx, K[0, 1] / rx
    out[1, 1] = K[1, 1] / ry
    out[0, 2] = (K[0, 2] + 0.5 - x0) / rx - 0.5
    out[1, 2] = (K[1, 2] + 0.5 - y0) / ry - 0.5
    return out


def infer_batch_resized(frames, size, dust_bin_ids: int, deepc, refinenet=None, interpolation="area_any", **kw):
    """``resize_device`` to ``size`` = (height, width) (by default ``"area_any"``: ``"area"``'s bits on integer factors, and any
    other reduction up to 64, e.g. 4.5 for a 1080p frame's 1440 x 1080 window), then ``inference.infer_batch`` (its keyword
    arguments pass through): frames (B, H, W) gray or (B, H, W, 3) BGR uint8 of any size, a GPU tensor (a view with a row pitch / frame stride is taken as it
    stands) or a host array (uploaded first) -> ``infer_batch``'s result with x and y taken back to the SOURCE's pixels by
    ``map_points``: per frame float64 [x, y, id] rows in the same order (``np.array([])`` for a frame without corners)."""
    import torch
    from .inference import infer_batch
    from .models._handles import unwrap
    dev = unwrap(deepc).device
    d = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
    if d.dtype != torch.uint8 or not (d.ndim == 3 or (d.ndim == 4 and d.shape[3] == 3)) or (d.ndim == 3 and d.shape[2] == 3):
        raise ValueError("expected (B,H,W) uint8 gray frames or (B,H,W,3) uint8 BGR frames")
    d = d.to(dev)
    src_size = (int(d.shape[1]), int(d.shape[2]))
    dst_size = _size(size)
    res = infer_batch(resize_device(d, dst_size, interpolation), dust_bin_ids, deepc, refinenet, **kw)
    kps = res[0] if kw.get("conf") else res
    kps = [k if k.size == 0 else map_points(np.asarray(k, np.float64), src_size, dst_size) for k in kps]
    return (kps, res[1]) if kw.get("conf") else kps
