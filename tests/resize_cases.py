"""The shapes tests/test_resize_host.py and tests/test_gpu_resize.py share, as (sh, sw, dh, dw), and their frames.

Chosen for the paths of csrc/dcx_resize.hip and the branches of resize.resize_host: odd sizes, spans shorter than one 16-byte chunk
and longer than one, a single source row, a single output pixel, an upscale (taps clamp on both sides in x, rows clip in y), a
reduction by a hair (37x53 -> 36x52), the identity, the 2x rule of "linear", and one larger shape per mode."""
import numpy as np

LINEAR_SHAPES = [(13, 17, 5, 7), (30, 40, 7, 9), (97, 131, 24, 32), (1, 9, 3, 4), (5, 7, 1, 1), (9, 11, 20, 31), (37, 53, 36, 52),
                 (8, 8, 8, 8), (48, 64, 24, 32)]
AREA_FACTORS = [(2, 2), (3, 3), (4, 4), (6, 6), (7, 7), (3, 2), (1, 5), (64, 1)]          # (fy, fx), onto 5 x 7 outputs
AREA_SHAPES = [(5 * fy, 7 * fx, 5, 7) for fy, fx in AREA_FACTORS]
COMMON_SHAPE = (96, 128, 24, 32)
MODES = ("nearest", "linear", "area")


def shapes(mode):
    return (AREA_SHAPES if mode == "area" else LINEAR_SHAPES) + [COMMON_SHAPE]


def all_cases():
    """(mode, (sh, sw, dh, dw)) for every shape of every mode."""
    return [(m, s) for m in MODES for s in shapes(m)]


def case_id(case):
    m, (sh, sw, dh, dw) = case
    return f"{m}-{sh}x{sw}-{dh}x{dw}"


def noise(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def extremes(shape, seed=0):
    """Frames of 0 and 255 only: the largest steps a tap can see."""
    return (np.random.default_rng(seed + 1000).integers(0, 2, shape) * 255).astype(np.uint8)
