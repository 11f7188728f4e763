"""The packed corner pool's word layout: the one place in the package that knows it.

The C ABI takes five separate pointers (``d_counts``, ``d_starts``, ``d_rows``, ``d_xy``, ``d_conf``); that they lie in ONE int32
buffer, so that one D2H or one all-gather moves a batch's result, is this package's decision:

    counts[B] | starts[B] | rows[pool][4] | xy[pool][2] | conf[pool][2]

``rows[p]`` = (x, y, id, cell) int32, ``xy`` and ``conf`` float32 bit patterns; frame b owns the slots
``[starts[b], starts[b] + counts[b])``.  ``infer_batch_device``'s docstring is the public description of what the words mean.
numpy only at import; torch where a function needs it.
"""
from collections import namedtuple
from typing import Sequence

import numpy as np

Layout = namedtuple("Layout", "counts starts rows xy conf")


def packed_len(batch: int, pool: int, conf: bool = False) -> int:
    """int32 words of the packed result of a batch: counts[B] | starts[B] | rows[pool][4] | xy[pool][2] (| conf[pool][2])."""
    return 2 * batch + (8 if conf else 6) * pool


def layout(batch: int, pool: int) -> Layout:
    """The word offset of every section."""
    return Layout(0, batch, 2 * batch, 2 * batch + 4 * pool, 2 * batch + 6 * pool)


def ptrs(address: int, batch: int, pool: int) -> tuple:
    """The byte addresses of (counts, starts, rows, xy, conf) in a pool that starts at ``address``."""
    return tuple(address + 4 * word for word in layout(batch, pool))


def views(packed: np.ndarray, batch: int, pool: int) -> tuple:
    """A 1-D int32 array -> views ``(counts, starts, rows (pool, 4) int32, xy (pool, 2) float32, conf (pool, 2) float32)``; a section
    the buffer ends before is None (``xy`` of an unrefined pool cut there, ``conf`` of a pool without confidences)."""
    at = layout(batch, pool)
    end = packed_len(batch, pool, True)
    n = packed.shape[0]
    return (packed[:at.starts], packed[at.starts:at.rows],
            packed[at.rows:at.xy].reshape(pool, 4) if n >= at.xy else None,
            packed[at.xy:at.conf].view(np.float32).reshape(pool, 2) if n >= at.conf else None,
            packed[at.conf:end].view(np.float32).reshape(pool, 2) if n >= end else None)


def frame_keypoints(rows: np.ndarray, xy, start: int, count: int, refined: bool) -> tuple:
    """One frame's slots -> ((count, 3) rows [x, y, id] sorted by id, stable w.r.t. slot order (inference.py:68-69): float64 from
    ``xy`` when refined, int64 from the integer rows otherwise; the sort's indices, for what else is kept by slot)."""
    stop = start + count
    ids = rows[start:stop, 2]
    a = np.empty((count, 3), np.float64 if refined else np.int64)
    a[:, 0:2] = xy[start:stop] if refined else rows[start:stop, 0:2]          # (the assignment widens: float32 -> float64 / int32 -> int64)
    a[:, 2] = ids
    order = ids.argsort(kind="stable")
    return a[order], order


def _pool_rows(keypoints, pool_order=False):
    """A view's [x, y, id] rows -> (rows (n, 3), an empty array gives (0, 3); the indices that put them in the order the corner pool
    holds them: id-sorted stably as ``pack_keypoints`` lays them, or as they stand with ``pool_order``)."""
    kp = np.asarray(keypoints)
    kp = kp.reshape(-1, 3) if kp.size else np.zeros((0, 3))
    return kp, np.arange(kp.shape[0]) if pool_order else np.argsort(kp[:, 2], kind="stable")


def _caller_order(keypoints):
    """The inverse of ``_pool_rows``' id sort: ``mask[_caller_order(kp)]`` takes a mask by pool slot back to the caller's rows."""
    return np.argsort(_pool_rows(keypoints)[1], kind="stable")


def pack_keypoints(keypoints_list: Sequence, device):
    """Host keypoint lists -> ``(packed, batch, pool)``: a corner pool on ``device`` (counts | starts | rows | xy) that the frames
    fill exactly, id-sorted like the reference.  Only the id word of a row is written (x, y, cell stay 0): the image points are
    ``xy``, which may be non-finite and so never pass through an integer."""
    import torch
    b = len(keypoints_list)
    kps = [_pool_rows(kp) for kp in keypoints_list]
    n = np.array([k.shape[0] for k, _ in kps], np.int64)
    pool = max(int(n.sum()), 1)
    packed = np.zeros(packed_len(b, pool), np.int32)
    counts, starts, rows, xy, _ = views(packed, b, pool)
    counts[:] = n
    starts[:] = np.concatenate([[0], np.cumsum(n)[:-1]])
    for (kp, order), s in zip(kps, starts.tolist()):
        if not kp.shape[0]:
            continue
        kp = kp[order]                                         # inference.py:68-69
        ids = kp[:, 2].astype(np.int64)
        rows[s:s + kp.shape[0], 2] = np.clip(ids, -1, np.iinfo(np.int32).max)
        xy[s:s + kp.shape[0]] = kp[:, :2].astype(np.float32)
    return torch.from_numpy(packed).to(device), b, pool
