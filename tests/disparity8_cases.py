"""The scene for the eight-path matcher's tests (tests/test_disparity8_host.py, tests/test_gpu_disparity8.py): a front plane whose
edges run diagonally.  Nothing here imports deepcharuco_amd."""
import functools

import numpy as np

import disparity_cases as dc


@functools.lru_cache(maxsize=None)
def band_scene(seed=0, h=48, w=160, d_back=12, d_front=37):
    """A textured left frame whose background lies at disparity ``d_back`` and whose diagonal band,
    (x + y > 90) & (x - y < 100), at ``d_front``; the right frame by forward mapping (background first, then the band, unfilled
    pixels random).  -> (left, right, true disparity (h, w)).  The arrays are shared: do not write to them."""
    rng = np.random.default_rng(seed)
    left = dc.texture(rng, h, w)
    right = rng.integers(0, 256, (h, w)).astype(np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    front = (xs + ys > 90) & (xs - ys < 100)
    truth = np.where(front, d_front, d_back).astype(np.int64)
    xr = xs - truth
    for sel in (~front, front):
        ok = sel & (xr >= 0)
        right[ys[ok], xr[ok]] = left[ok]
    for a in (left, right, truth):
        a.setflags(write=False)
    return left, right, truth
