"""Hand-built corner pools for the tests of the pool forms (PnP, calibration, stereo): frames laid at chosen slots."""
import numpy as np

from deepcharuco_amd.corner_pool import packed_len, views


def lay_frames(frames, pool, order=None, gap=0, first=0, filler=0, cell=None, id_sorted=False):
    """[x, y, id] frames -> (packed int32 pool (counts | starts | rows | xy), owned bool[pool]: the slots that hold a frame's row).

    The frames go into the pool in ``order`` (default: as listed), the first at slot ``first``, ``gap`` free slots after each;
    ``id_sorted`` sorts a frame's rows stably by id before they are laid.  A row's words are (rint(x), rint(y), id, ``cell``) and
    its xy the float32 (x, y).  Every row word no frame owns holds ``filler``, and so does an owned row's cell word when ``cell``
    is None; free xy words are 0.  Rows past the pool's end are dropped as the kernels drop them: the count stays whole."""
    B = len(frames)
    packed = np.zeros(packed_len(B, pool), np.int32)
    counts, starts, rows, xy, _ = views(packed, B, pool)
    rows[:] = filler
    owned = np.zeros(pool, bool)
    s = first
    for b in range(B) if order is None else order:
        kp = frames[b]
        if id_sorted and len(kp):
            kp = kp[np.argsort(kp[:, 2], kind="stable")]
        counts[b], starts[b] = len(kp), s
        k = min(len(kp), pool - s)
        if k > 0:
            rows[s:s + k, 0:2] = np.rint(kp[:k, :2])
            rows[s:s + k, 2] = kp[:k, 2]
            if cell is not None:
                rows[s:s + k, 3] = cell
            xy[s:s + k] = kp[:k, :2]
            owned[s:s + k] = True
        s += len(kp) + gap
    return packed, owned
