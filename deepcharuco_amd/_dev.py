"""What the device wrappers (pnp, calib, stereo, rectify, disparity) share in front of a C call.  Every check reads attributes only:
with the tensors given nothing here allocates or synchronises (capture-safe entries rely on it).  The error texts are the callers'."""
import math

from .corner_pool import layout, ptrs


def pool_ptrs(packed, batch, pool, refined):
    """The corner pool's layout check -> the addresses of (counts, starts, rows, xy or None)."""
    import torch
    at = layout(batch, pool)
    if packed.dtype != torch.int32 or not packed.is_contiguous() or packed.numel() < (at.conf if refined else at.xy):
        raise ValueError("packed must be a contiguous int32 corner pool of at least packed_len(batch, pool) words")
    counts_p, starts_p, rows_p, xy_p, _ = ptrs(packed.data_ptr(), batch, pool)
    return counts_p, starts_p, rows_p, xy_p if refined else None


def tensor(t, dev, dtype, shape, message, rule="shape", zeros=False):
    """The caller's ``t``, or when None a new tensor of ``shape`` (rule "min": no axis empty) -> a contiguous ``dtype`` tensor on
    ``dev`` of exactly that shape, or (rule "numel") that many values, or (rule "min") at least as many; else ValueError(message)."""
    import torch
    if t is None:
        return (torch.zeros if zeros else torch.empty)(tuple(max(s, 1) if rule == "min" else s for s in shape), dtype=dtype, device=dev)
    n, have = math.prod(shape), t.numel()
    size_ok = tuple(t.shape) == tuple(shape) if rule == "shape" else have >= n if rule == "min" else have == n
    if t.device != dev or t.dtype != dtype or not size_ok or not t.is_contiguous():
        raise ValueError(message)
    return t


def workspace(ws, dev, nbytes, message=None, aligned_u8=False):
    """The caller's workspace -> itself if it is contiguous, on ``dev``, of at least ``nbytes`` bytes and, with ``aligned_u8``, a
    uint8 tensor at an 8-byte aligned address, ValueError(message) otherwise; None -> a new one of ``nbytes``, float64-backed."""
    import torch
    if ws is None:
        return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev)
    if (ws.device != dev or not ws.is_contiguous() or ws.numel() * ws.element_size() < nbytes
            or (aligned_u8 and (ws.dtype != torch.uint8 or ws.data_ptr() % 8))):
        raise ValueError(message)
    return ws


def u8_frames(x, ch=1, unit_axes_free=False):
    """A uint8 batch (B, H, W) or, ``ch`` = 3, (B, H, W, 3) whose pixels are contiguous within a row, at any row pitch and frame
    stride -> (data_ptr, frame_stride, pitch, B, H, W).  ``unit_axes_free``: the stride of an axis of length 1 is not looked at."""
    st = x.stride()
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    pitch = int(st[1]) if H > 1 or not unit_axes_free else W * ch
    frame_stride = int(st[0]) if B > 1 else 0
    if ((st[2] != ch or (ch == 3 and st[3] != 1)) and (W > 1 or not unit_axes_free)) or pitch < W * ch or frame_stride < 0:
        raise ValueError("the pixels of a row must be contiguous, the pitch at least a row and the frame stride not negative")
    return x.data_ptr(), frame_stride, pitch, B, H, W
