"""Scenes for the tests of the stereo kernels at their launch limits and under graph replay (tests/test_disparity_limits_host.py,
tests/test_gpu_disparity_limits.py, tests/test_gpu_disparity_graph.py).  Nothing here imports deepcharuco_amd.  The arrays are
shared between tests: every one is read-only."""
import functools

import numpy as np

import disparity_cases as dc
import speckle_cases as sc

MAX_WIDTH = 4096                             # csrc/dcx_sgm.hip: kMaxWidth
SGM_CHUNK_CAP = 16384                        # csrc/dcx_sgm.hip: kMaxChunk
SPECKLE_CHUNK_CAP = 32768                    # csrc/dcx_speckle.hip: kMaxChunk
SGM_PERIOD, SPECKLE_PERIOD = 7, 11           # 16384 mod 7 = 4 and 32768 mod 11 = 10: a tail chunk that re-read frame 0 would show
SMALL = (2, 3)                               # the frames of the chunk-cap batches

NV = sc.NV
SPECKLE = dict(speckle_window_size=100, speckle_range=2)
FILTER = (NV, 3, 16)                         # (new_val, max_speckle_size, max_diff) of the filter-alone cases
SMALL_SPECKLE = dict(speckle_window_size=2, speckle_range=0)                  # 2 x 3 frames: only equal values join, pairs and singles go
SMALL_FILTER = (NV, 2, 16)                   # the same for the filter alone (the maps' values are 40 apart)
REORDER = (2, 0, 1)                          # the frame order that a replay swaps in


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def tiled(period, n):
    """Frames repeating with the period of ``period`` (P, ...): -> (n, ...)."""
    reps = -(-n // len(period))
    return np.tile(period, (reps,) + (1,) * (period.ndim - 1))[:n]


# ------------------------------------------------------------------------------------------------ B1, B2: width and line length

@functools.lru_cache(maxsize=None)
def wide_pair(h):
    """h x 4096, true disparity 9 everywhere."""
    return _frozen(*dc.shifted_pair(np.random.default_rng([51, h]), h, MAX_WIDTH, 9))


@functools.lru_cache(maxsize=None)
def tall_pair(w, h=2100):
    """h x w (w = 3 or 1): the true disparity is w - 1 px (0 in a single column), and the middle third of the right frame is noise."""
    rng = np.random.default_rng([52, w])
    left, right = dc.shifted_pair(rng, h, w, w - 1)
    right[h // 3:2 * h // 3] = rng.integers(0, 256, (2 * h // 3 - h // 3, w), dtype=np.uint8)
    return _frozen(left, right)


# ------------------------------------------------------------------------------------------------ B3, B4: the chunk caps

@functools.lru_cache(maxsize=None)
def sgm_period():
    """One period of the matcher's chunk-cap batch: (left, right) uint8 (7, 2, 3)."""
    rng = np.random.default_rng(53)
    left = rng.integers(0, 256, (SGM_PERIOD,) + SMALL, dtype=np.uint8)
    right = rng.integers(0, 256, (SGM_PERIOD,) + SMALL, dtype=np.uint8)
    right[::2, :, :2] = left[::2, :, 1:]                                      # every other frame has a true disparity of 1
    return _frozen(left, right)


@functools.lru_cache(maxsize=None)
def speckle_period():
    """One period of the filter's chunk-cap batch: int16 (11, 2, 3)."""
    return _frozen(sc.random_map(6, (SPECKLE_PERIOD,) + SMALL))


# ------------------------------------------------------------------------------------------------ B5: the int16 range's ends

EDGES = {"low": dict(min_disparity=-2047, num_disparities=64, width=2112, true=-2047),      # valid pixels hold -32752, invalid -32768
         "high": dict(min_disparity=1791, num_disparities=256, width=2100, true=2046)}      # valid pixels hold 32736
EDGE_H = 5


@functools.lru_cache(maxsize=None)
def edge_scene(end):
    """A 5-row pair whose true match is the candidate range's edge (``EDGES[end]``), in the few columns where that candidate lies
    on the frame: right[:, x - true] = left[:, x].  -> (left, right, match (W,) bool: the columns that have a true match)."""
    w, d = EDGES[end]["width"], EDGES[end]["true"]
    rng = np.random.default_rng([54, w])
    if d < 0:
        right, left = dc.shifted_pair(rng, EDGE_H, w, -d)
    else:
        left, right = dc.shifted_pair(rng, EDGE_H, w, d)
    x = np.arange(w)
    return _frozen(left, right, (x - d >= 0) & (x - d < w))


@functools.lru_cache(maxsize=None)
def narrow_pair():
    """5 x 70: at m = -2047 no candidate lies on the frame."""
    return _frozen(*dc.shifted_pair(np.random.default_rng(55), EDGE_H, 70, 9))


# ------------------------------------------------------------------------------------------------ A1, B6, B7: small batches

@functools.lru_cache(maxsize=None)
def small_batch(seed, h=11, w=70):
    """Three pairs h x w with true disparities that differ from frame to frame: (left, right) uint8 (3, h, w)."""
    rng = np.random.default_rng([56, seed])
    pairs = [dc.shifted_pair(rng, h, w, d) for d in ((9, 2, 17), (5, 12, 0))[seed % 2]]
    return _frozen(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))


@functools.lru_cache(maxsize=None)
def broadcast_batch(h=11, w=70):
    """One left frame and three right frames, that frame at disparities 9, 3 and 20: (left (h, w), right (3, h, w))."""
    rng = np.random.default_rng(57)
    left = dc.texture(rng, h, w)
    right = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    for r, d in zip(right, (9, 3, 20)):
        r[:, :w - d] = left[:, d:]
    return _frozen(left, right)


@functools.lru_cache(maxsize=None)
def speckle_batch(seed):
    """int16 (3, 40, 70): 2 x 3 tiles to a frame."""
    return _frozen(sc.random_map(seed, (3, 40, 70)))


@functools.lru_cache(maxsize=None)
def two_plane_batch(order=(0, 1, 2)):
    """The two-plane scene, upside down and mirrored (the batch of test_gpu_speckle.py::test_sgm_device_with_the_filter), the frames
    in ``order``."""
    left, right = dc.two_plane_scene()[:2]
    bl, br = np.stack([left, left[::-1], left[:, ::-1]]), np.stack([right, right[::-1], right[:, ::-1]])
    return _frozen(np.ascontiguousarray(bl[list(order)]), np.ascontiguousarray(br[list(order)]))
