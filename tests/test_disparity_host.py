"""The stereo matcher's definition (deepcharuco_amd/disparity.py, numpy): every step on cases small enough to verify by hand, the
argument refusals, its accuracy on a two-plane scene and the 3-D points against the corner path (rectify.reproject_to_3d)."""
import numpy as np
import pytest

import disparity_cases as dc
import rectify_exact as rx
import stereo_exact as sx
from deepcharuco_amd import disparity as dp, rectify as rc


def _word(bits: str) -> int:
    assert len(bits) == 62
    return int(bits, 2)


# ------------------------------------------------------------------------------------------------ step 1: census

def test_census_1x1_is_zero():
    """Every neighbour is the replicated centre itself: no bit is set."""
    c = dp.census_host(np.array([[200]], np.uint8))
    assert c.dtype == np.uint64 and c.shape == (1, 1) and int(c[0, 0]) == 0


def test_census_3x3_edge_replication_and_bit_order():
    """img = 1..9.  Centre pixel 5: the window's rows are the image rows 0,0,0,1,2,2,2 and its columns 0,0,0,0,1,2,2,2,2, so three rows
    of nine 1s (1, 2, 3 < 5), the centre row 4,4,4,4,.,6,6,6,6 -> 11110000, three rows of nine 0s; the first neighbour is the most
    significant bit.  Pixel 9 (bottom right): rows 0,0,1,2,2,2,2, columns 0,0,0,1,2,2,2,2,2: three rows all smaller, the centre row
    7,7,7,8,.,9,9,9,9 -> 11110000, three more rows 7,7,7,8,9,9,9,9,9 -> 111100000.  Pixel 1 (top left): nothing is smaller."""
    img = np.arange(1, 10, dtype=np.uint8).reshape(3, 3)
    c = dp.census_host(img)
    assert int(c[1, 1]) == _word("1" * 27 + "11110000" + "0" * 27)
    assert int(c[2, 2]) == _word("1" * 27 + "11110000" + "111100000" * 3)
    assert int(c[0, 0]) == 0


def test_cost_is_popcount_with_clamped_column():
    cl = np.array([[0b1011, 0, (1 << 62) - 1]], np.uint64)
    cr = np.array([[0b0001, 0b1111, 0]], np.uint64)
    C = dp.cost_volume_host(cl, cr, 0, 64)
    assert C.shape == (1, 3, 64)
    assert C[0, 0, 0] == 2 and C[0, 0, 1] == 2 and C[0, 0, 63] == 2          # x - d < 0 clamps to column 0
    assert C[0, 2, 0] == 62 and C[0, 2, 1] == 58 and C[0, 2, 2] == 61
    C = dp.cost_volume_host(cl, cr, -2, 64)                                   # m = -2: d = 0 looks two columns to the right
    assert C[0, 0, 0] == 3 and C[0, 0, 1] == 1 and C[0, 0, 2] == 2 and C[0, 0, 3] == 2 and C[0, 2, 0] == 62      # (clamped at both ends)


# ------------------------------------------------------------------------------------------------ step 3: the recursion

def _line_costs():
    """A 1 x 4 line, D = 64: cost 20 everywhere but C(x0, 3) = 0, C(x0, 63) = 1, C(x1, 4) = 0, C(x2, 10) = 0, C(x3, 10) = 5."""
    C = np.full((1, 4, 64), 20, np.int32)
    C[0, 0, 3], C[0, 0, 63], C[0, 1, 4], C[0, 2, 10], C[0, 3, 10] = 0, 1, 0, 0, 5
    return C


def test_recursion_by_hand():
    """P1 = 3, P2 = 8, left to right.
    x0: L = C, M = 0.
    x1 (M + P2 = 8): L(4) = 0 + min(20, L(3) + 3 = 3, 23, 8) = 3; L(3) = 20 + 0 = 20; L(2) = 20 + (L(3) + 3) = 23; L(5) = 20 + 8;
        L(63) = 20 + min(1, 23, -, 8) = 21 (no d + 1 term); L(62) = 20 + min(20, 23, 1 + 3, 8) = 24; L(0) = 20 + min(20, -, 23, 8) = 28
        (no d - 1 term); every other 28.  M = 3.
    x2 (M + P2 = 11): L(10) = 0 + 11 - 3 = 8; L(4) = 20 + 3 - 3 = 20; L(3) = L(5) = 20 + (3 + 3) - 3 = 23; L(2) = 20 + 11 - 3 = 28;
        L(63) = 20 + min(21, 27, -, 11) - 3 = 28; every other 28.  M = 8.
    x3 (M + P2 = 16): L(10) = 5 + 8 - 8 = 5; L(9) = L(11) = 20 + (8 + 3) - 8 = 23; L(4) = 20 + 16 - 8 = 28; every other 28."""
    L = dp._path(_line_costs(), 3, 8, False)[0]
    x1 = np.full(64, 28)
    x1[[4, 3, 2, 63, 62]] = 3, 20, 23, 21, 24
    x2 = np.full(64, 28)
    x2[[10, 4, 3, 5]] = 8, 20, 23, 23
    x3 = np.full(64, 28)
    x3[[10, 9, 11]] = 5, 23, 23
    assert np.array_equal(L[0], _line_costs()[0, 0])
    assert np.array_equal(L[1], x1) and np.array_equal(L[2], x2) and np.array_equal(L[3], x3)


def test_four_paths_on_a_line():
    """On a 1 x 4 image the vertical paths have one pixel each (L = C), and the right-to-left path is the left-to-right path of
    the mirrored line: S = L_lr + L_rl + 2 C."""
    C = _line_costs()
    lr = dp._path(C, 3, 8, False)
    rl = dp._path(C[:, ::-1], 3, 8, False)[:, ::-1]
    assert np.array_equal(dp._path(C, 3, 8, True), rl)
    S = dp.aggregate_host(C, 3, 8)
    assert np.array_equal(S, lr + rl + 2 * C)
    assert S[0, 3, 10] == 5 + 5 + 10                                         # (the right-to-left path starts at x3: L = C)
    tall = dp.aggregate_host(np.ascontiguousarray(C.transpose(1, 0, 2)), 3, 8)                # the same line as a column
    assert np.array_equal(tall.transpose(1, 0, 2), S)


# ------------------------------------------------------------------------------------------------ steps 4 - 6

def _flat_S(w=8, value=100):
    return np.full((1, w, 64), value, np.int64)


def test_subpixel_is_a_floor_division():
    """S(5) = 10, S(4) = 11, S(6) = 12: num = -1, den = 3, off = floor(-13 / 6) = -3 (C's / would give -2).  S(4) = 12, S(6) = 13:
    num = -1, den = 5, off = floor(-11 / 10) = -2.  Mirrored (S(4) = 12, S(6) = 11): num = 1, den = 3, off = floor(19 / 6) = 3.
    S(4) = 11, S(6) = 31: off = floor(-298 / 44) = -7; S(4) = 11, S(6) = 50: off = floor(-583 / 82) = -8; S(6) = S(5): off = 8.
    Columns x < 5 have x - d* < 0: invalid."""
    for lo, hi, off in ((11, 12, -3), (12, 13, -2), (12, 11, 3), (20, 20, 0), (11, 31, -7), (11, 50, -8), (30, 10, 8)):
        S = _flat_S()
        S[0, :, 5], S[0, :, 4], S[0, :, 6] = 10, lo, hi
        out = dp.select_host(S, 0, 0, -1)
        assert out.dtype == np.int16
        assert np.array_equal(out[0], [-16] * 5 + [16 * 5 + off] * 3), (lo, hi, out)
    S = _flat_S()
    S[0, :, 0], S[0, :, 1] = 10, 50                                           # d* = 0: no sub-pixel step
    assert np.array_equal(dp.select_host(S, 3, 0, -1)[0], [32] * 3 + [48] * 5)            # m = 3: x < 3 invalid (16 (m - 1) = 32), else 16 m
    S = _flat_S(80)
    S[0, :, 63], S[0, :, 62] = 10, 50                                         # d* = D - 1: no sub-pixel step
    assert np.array_equal(dp.select_host(S, 0, 0, -1)[0], [-16] * 63 + [16 * 63] * 17)


def test_ties_take_the_lowest_disparity():
    S = _flat_S()
    S[0, :, 7], S[0, :, 2] = 40, 40
    assert np.array_equal(dp.select_host(S, 0, 0, -1)[0], [-16] * 2 + [32] * 6)


def test_uniqueness_boundary():
    """uniqueness = 10, S(d*) = 90: a far candidate at 100 gives 100 * 90 = 9000 < 90 * 100 = 9000, false: valid; at 99 it gives
    8910 < 9000: invalid.  The neighbours d* +- 1 are exempt whatever they hold."""
    for far, ok in ((100, True), (99, False)):
        S = _flat_S(8, 200)
        S[0, :, 2], S[0, :, 1], S[0, :, 3], S[0, :, 30] = 90, 91, 91, far
        out = dp.select_host(S, 0, 10, -1)
        assert np.array_equal(out[0, 2:] != -16, [ok] * 6), (far, out)
        assert (out[0, :2] == -16).all()
    S = _flat_S(8, 200)
    S[0, :, 2], S[0, :, 4] = 90, 99                                           # |d - d*| = 2 is far enough
    assert (dp.select_host(S, 0, 10, -1) == -16).all()
    assert (dp.select_host(S, 0, 0, -1)[0, 2:] != -16).all()                   # uniqueness = 0 never invalidates the minimum


def test_left_right_check():
    """W = 8, S = 100 but S(x = 6, d = 3) = 10 and S(x = 7, d = 4) = 5.  Pixel 6 wins d* = 3 and looks at right pixel 3, whose
    candidates are S(3, 0), S(4, 1), S(5, 2), S(6, 3) = 10, S(7, 4) = 5: dR = 4.  |4 - 3| = 1 passes lr_max_diff = 1, fails 0.  Pixel 7
    wins d* = 4, the same right pixel, and passes both.  Pixel 3 ties at d* = 0 and looks at that right pixel too: |4 - 0| fails
    both.  Every other pixel ties at d* = 0 with dR = 0."""
    S = _flat_S()
    S[0, 6, 3], S[0, 7, 4] = 10, 5
    assert np.array_equal(dp.select_host(S, 0, 0, 1)[0], [0, 0, 0, -16, 0, 0, 48, 64])
    assert np.array_equal(dp.select_host(S, 0, 0, 0)[0], [0, 0, 0, -16, 0, 0, -16, 64])
    assert np.array_equal(dp.select_host(S, 0, 0, -1)[0], [0] * 6 + [48, 64])
    S[0, 7, 4] = 10                                         # a tie in the right view takes the lowest d: dR = 3, and pixel 7 is one off
    assert np.array_equal(dp.select_host(S, 0, 0, 0)[0], [0, 0, 0, -16, 0, 0, 48, -16])
    assert np.array_equal(dp.select_host(S, 0, 0, 1)[0], [0, 0, 0, -16, 0, 0, 48, 64])


# ------------------------------------------------------------------------------------------------ whole images

@pytest.mark.parametrize("value", [0, 93, 255])
def test_constant_images(value):
    """Every S ties: d* = 0, every pixel valid, 16 m everywhere (m = 0)."""
    img = np.full((9, 70), value, np.uint8)
    out = dp.sgm_host(img, img)
    assert out.shape == (9, 70) and out.dtype == np.int16 and not out.any()


def test_batch_is_frame_by_frame():
    rng = np.random.default_rng(3)
    l, r = rng.integers(0, 256, (2, 3, 9, 20), dtype=np.uint8)
    out = dp.sgm_host(l, r, -2, 64, 5, 40, 5, 0)
    assert out.shape == (3, 9, 20)
    for i in range(3):
        assert np.array_equal(out[i], dp.sgm_host(l[i], r[i], -2, 64, 5, 40, 5, 0))


def test_argument_refusals():
    img = np.zeros((8, 8), np.uint8)
    ok = dict(min_disparity=0, num_disparities=64, p1=7, p2=86, uniqueness=10, lr_max_diff=1)
    dp.sgm_host(img, img, **ok)
    dp.sgm_host(img, img, **dict(ok, lr_max_diff=-5))
    dp.sgm_host(np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8))
    for bad in (dict(num_disparities=32), dict(num_disparities=96), dict(num_disparities=512), dict(p1=-1), dict(p1=90),
                dict(p2=256), dict(uniqueness=-1), dict(uniqueness=100), dict(p1=7.5), dict(min_disparity=-2048),
                dict(min_disparity=1984), dict(num_disparities=64.0)):
        with pytest.raises(ValueError):
            dp.sgm_host(img, img, **dict(ok, **bad))
    with pytest.raises(ValueError):
        dp.sgm_host(img.astype(np.int16), img.astype(np.int16))
    with pytest.raises(ValueError):
        dp.sgm_host(img, np.zeros((8, 9), np.uint8))
    with pytest.raises(ValueError):
        dp.sgm_host(np.zeros((0, 8), np.uint8), np.zeros((0, 8), np.uint8))
    with pytest.raises(ValueError):
        dp.sgm_host(np.zeros((1, 2, 8, 8), np.uint8), np.zeros((1, 2, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        dp.disparity_to_points_host(np.zeros((4, 4), np.int16), np.eye(3))
    with pytest.raises(ValueError):
        dp.disparity_to_points_host(np.zeros((4, 4), np.int32), np.eye(4))


def test_host_accuracy_two_planes():
    """A 48 x 160 textured pair, background at disparity 12, a rectangle at 37, at the default parameters.  Measured with this
    definition: 84.9 % of the pixels valid; of the valid ones 98.9 % within 1 px of the truth and 94.8 % within 0.25 px; 98.5 % of the
    pixels that are neither occluded nor off the right frame (x - d < 0) valid.  The gates are those values less two percentage
    points.  Nothing but the occluded and off-frame pixels is left out of any count."""
    left, right, truth, occluded, off_frame = dc.two_plane_scene()
    out = dp.sgm_host(left, right)
    valid = out != -16
    assert (out[valid] >= 0).all()
    err = np.abs(out / 16.0 - truth)
    f_valid = valid.mean()
    f_1px = (err[valid] <= 1.0).mean()
    f_quarter = (err[valid] <= 0.25).mean()
    f_visible = valid[~occluded & ~off_frame].mean()
    print(f"valid {f_valid:.4f}, of those within 1 px {f_1px:.4f}, within 0.25 px {f_quarter:.4f}; visible pixels valid {f_visible:.4f}; "
          f"occluded {occluded.mean():.4f}, off frame {off_frame.mean():.4f}")
    assert f_valid >= 0.829 and f_1px >= 0.969 and f_quarter >= 0.928 and f_visible >= 0.965


# ------------------------------------------------------------------------------------------------ the points

def test_points_against_the_corner_path():
    (K0, d0), (K1, d1) = sx.cam("A"), sx.cam("B")
    R, T = rx.rig_RT("small", "A", "B")
    r = rc.stereo_rectify_host(K0, d0, K1, d1, rx.SIZE, R, T)
    assert r.axis == 0
    rng = np.random.default_rng(11)
    m = -16
    disp = rng.integers(16 * m, 16 * 64, (2, 23, 31)).astype(np.int16)
    disp[0, 0, :5] = 16 * (m - 1)
    disp[1, 3, 4] = 0
    disp[1, 5, 6] = -7
    pts = dp.disparity_to_points_host(disp, r.Q, m)
    assert pts.shape == (2, 23, 31, 3) and pts.dtype == np.float64
    bad = (disp < 16 * m) | (disp == 0)
    assert bad[0, 0, :5].all() and bad[1, 3, 4] and not bad[1, 5, 6]
    assert np.isnan(pts[bad]).all() and np.isfinite(pts[~bad]).all()
    ys, xs = np.mgrid[0:23, 0:31]
    for b in range(2):
        d = disp[b] / 16.0
        xy0 = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
        xy1 = np.stack([xs.ravel() - d.ravel(), ys.ravel()], 1)
        ref = rc.reproject_to_3d(r.Q, xy0, xy1, 0).reshape(23, 31, 3)
        ok = ~bad[b]
        rel = np.linalg.norm(pts[b][ok] - ref[ok], axis=1) / np.linalg.norm(ref[ok], axis=1)
        assert rel.max() <= 1e-12, rel.max()
