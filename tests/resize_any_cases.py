"""The shapes tests/test_resize_any_host.py and tests/test_gpu_resize_any.py share for "area_any" (cv2's general INTER_AREA), as
(sh, sw, dh, dw); the frames are resize_cases.noise / extremes.

GENERAL_SHAPES take the general path (a fractional factor on at least one axis), INTEGER_SHAPES the routing rule (integer factors
on both axes are "area"'s).  What each one is there for:

  (9, 9, 2, 2)          4.5, one tile
  (54, 72, 12, 16)      the ratio of a 1080p frame's 4:3 window, 1440 x 1080 -> 320 x 240
  (10, 10, 3, 3)        3.33...: the last cell's f2 may land a hair under sn
  (37, 53, 36, 52)      a reduction by a hair: almost every pixel is two taps per axis
  (15, 31, 5, 7)        integer in y, fractional in x: both axes must take the general path
  (127, 9, 2, 4)        63.5 in y: 65 taps, 66 staged rows (the span is the whole 9-pixel row, so they fit without a narrower tile)
  (127, 900, 2, 400)    63.5 in y by 2.25 in x: the tile width is halved until 66 staged rows fit (once for gray, three times for
                        BGR: ten tiles per output row)
  (7, 13, 1, 1)         a single output pixel
  (1, 9, 1, 4)          a single source row
  (8, 8, 8, 5)          scale 1 on one axis; exact ties before the final rounding
  (9, 900, 2, 400)      in BGR an output row is 1,200 bytes: more than one workgroup tile
  (1, 2003, 1, 2002)    SLIVER_SHAPE, the only one with end taps below 1e-3 (cell edges have fractions that are multiples of
                        1/2002, so the first two are dropped): there for the rule, and left out of the exact-math gate
  (15, 14, 5, 7), (12, 12, 6, 6), (5, 7, 5, 7)   integer both ways, 2 x 2 and the identity"""
from resize_cases import extremes, noise  # noqa: F401  (the frames of both test files)

SLIVER_SHAPE = (1, 2003, 1, 2002)
GENERAL_SHAPES = [(9, 9, 2, 2), (54, 72, 12, 16), (10, 10, 3, 3), (37, 53, 36, 52), (15, 31, 5, 7), (127, 9, 2, 4), (127, 900, 2, 400),
                  (7, 13, 1, 1), (1, 9, 1, 4), (8, 8, 8, 5), (9, 900, 2, 400), SLIVER_SHAPE]
INTEGER_SHAPES = [(15, 14, 5, 7), (12, 12, 6, 6), (5, 7, 5, 7)]
SHAPES = GENERAL_SHAPES + INTEGER_SHAPES
EXACT_SHAPES = [s for s in GENERAL_SHAPES if s != SLIVER_SHAPE]            # no true sliver is dropped: dn < 1000 on both axes
MODE = "area_any"


def shape_id(shape):
    sh, sw, dh, dw = shape
    return f"{sh}x{sw}-{dh}x{dw}"
