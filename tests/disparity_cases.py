"""Scenes for the stereo matcher's tests (tests/test_disparity_host.py, tests/test_gpu_disparity.py).  Nothing here imports
deepcharuco_amd."""
import functools

import numpy as np


def texture(rng, h, w):
    """A random u8 texture, 2 x 2 box-smoothed."""
    t = rng.integers(0, 256, (h + 1, w + 1)).astype(np.int64)
    return ((t[:-1, :-1] + t[1:, :-1] + t[:-1, 1:] + t[1:, 1:] + 2) >> 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def two_plane_scene(h=48, w=160, seed=7, d_back=12, d_front=37, rect=(12, 36, 50, 110)):
    """A textured left frame whose background lies at disparity ``d_back`` and whose rectangle rect = (y0, y1, x0, x1) at
    ``d_front``; the right frame by forward mapping (background first, then foreground, unfilled pixels random).
    -> (left, right, true disparity (h, w), occluded (h, w): the left pixel's place in the right frame went to another pixel,
    off_frame (h, w): x - d < 0).  The arrays are shared: do not write to them."""
    rng = np.random.default_rng(seed)
    left = texture(rng, h, w)
    truth = np.full((h, w), d_back, np.int64)
    y0, y1, x0, x1 = rect
    truth[y0:y1, x0:x1] = d_front
    right = rng.integers(0, 256, (h, w), dtype=np.uint8)
    owner = np.full((h, w), -1, np.int64)                         # the left column that a right pixel shows
    ys, xs = np.mgrid[0:h, 0:w]
    for front in (False, True):
        sel = (truth == d_front) == front
        xr = xs - truth
        ok = sel & (xr >= 0)
        right[ys[ok], xr[ok]] = left[ok]
        owner[ys[ok], xr[ok]] = xs[ok]
    xr = xs - truth
    off_frame = xr < 0
    occluded = ~off_frame & (owner[ys, np.clip(xr, 0, w - 1)] != xs)
    for a in (left, right, truth, occluded, off_frame):
        a.setflags(write=False)
    return left, right, truth, occluded, off_frame


def shifted_pair(rng, h, w, d):
    """A textured pair whose true disparity is ``d`` everywhere (right[x] = left[x + d], the rest random)."""
    left = texture(rng, h, w)
    right = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if d < w:
        right[:, :w - d] = left[:, d:]
    return left, right
