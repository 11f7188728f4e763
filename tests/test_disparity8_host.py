"""The eight-path option of the stereo matcher's definition (deepcharuco_amd/disparity.py, ``paths=8``): the recursion against a
scalar restatement that walks every line of every direction, exact identities, a 2 x 2 case by hand, the unchanged default, the
refusals, and the accuracy on a scene whose depth edges run diagonally and on the axis-aligned one."""
import numpy as np
import pytest

import disparity8_cases as d8
import disparity_cases as dc
from deepcharuco_amd import disparity as dp

AXIS = ((0, 1), (0, -1), (1, 0), (-1, 0))
DIAGONAL = ((1, 1), (-1, -1), (1, -1), (-1, 1))
PENALTIES = ((0, 0), (7, 86), (255, 255))


def _restated(C, p1, p2, directions):
    """Step 3 in plain Python: for every direction (dy, dx), every pixel whose predecessor p - (dy, dx) lies outside the frame
    starts a line; the line is walked pixel by pixel, candidate by candidate, and its L added to S."""
    H, W, D = C.shape
    S = np.zeros((H, W, D), np.int64)
    for dy, dx in directions:
        for y0 in range(H):
            for x0 in range(W):
                if 0 <= y0 - dy < H and 0 <= x0 - dx < W:
                    continue
                y, x, prev = y0, x0, None
                while 0 <= y < H and 0 <= x < W:
                    c = [int(v) for v in C[y, x]]
                    if prev is None:
                        cur = c
                    else:
                        M = min(prev)
                        cur = []
                        for d in range(D):
                            terms = [prev[d], M + p2]
                            if d > 0:
                                terms.append(prev[d - 1] + p1)
                            if d < D - 1:
                                terms.append(prev[d + 1] + p1)
                            cur.append(c[d] + min(terms) - M)
                    S[y, x] += cur
                    prev = cur
                    y, x = y + dy, x + dx
    return S


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (2, 2), (5, 7), (7, 5), (4, 4)])
def test_recursion_against_the_scalar_restatement(shape):
    rng = np.random.default_rng([81, *shape])
    C = rng.integers(0, 63, shape + (64,)).astype(np.int32)
    for p1, p2 in PENALTIES:
        S8 = dp.aggregate_host(C, p1, p2, paths=8)
        assert S8.dtype == np.int32 and S8.shape == C.shape
        assert np.array_equal(S8, _restated(C, p1, p2, AXIS + DIAGONAL)), (shape, p1, p2)
        assert np.array_equal(dp.aggregate_host(C, p1, p2, paths=4), _restated(C, p1, p2, AXIS)), (shape, p1, p2)
        assert np.array_equal(dp.aggregate_host(C, p1, p2), dp.aggregate_host(C, p1, p2, paths=4))


def test_exact_identities():
    rng = np.random.default_rng(82)
    for shape in ((1, 9), (9, 1), (1, 1)):                                    # every diagonal of a line has one pixel: L = C
        C = rng.integers(0, 63, shape + (64,)).astype(np.int32)
        assert np.array_equal(dp.aggregate_host(C, 7, 86, paths=8), dp.aggregate_host(C, 7, 86, paths=4) + 4 * C)
    C = rng.integers(0, 63, (6, 11, 64)).astype(np.int32)
    S8 = dp.aggregate_host(C, 7, 86, paths=8)
    Ct = np.ascontiguousarray(C.transpose(1, 0, 2))
    assert np.array_equal(dp.aggregate_host(Ct, 7, 86, paths=8), S8.transpose(1, 0, 2))                 # transposed
    assert np.array_equal(dp.aggregate_host(np.ascontiguousarray(C[:, ::-1]), 7, 86, paths=8), S8[:, ::-1])   # mirrored columns
    assert not np.array_equal(S8, 2 * dp.aggregate_host(C, 7, 86, paths=4))


def test_constant_volumes():
    """One value everywhere: every term of the minimum is at least M, L(q, d) = M is among them, so L = C on every path and
    S = 8 C at any penalties.  A volume that is constant over (y, x) but not over d keeps that only at P1 = P2 = 0 (where
    min(...) = M always): with penalties, c = (0, 20, ...) gives 20 + min(20, 0 + P1, M + P2) - 0 = 20 + P1 at the second pixel.
    All costs 62 at P2 = 255: S = 8 * 62, inside the bound 8 (62 + 255) = 2536, which random costs at the largest penalties
    keep too."""
    for p1, p2 in PENALTIES:
        C = np.full((5, 7, 64), 17, np.int32)
        assert np.array_equal(dp.aggregate_host(C, p1, p2, paths=8), 8 * C)
    c = np.random.default_rng(83).integers(0, 63, 64).astype(np.int32)
    C = np.ascontiguousarray(np.broadcast_to(c, (5, 7, 64)))
    assert np.array_equal(dp.aggregate_host(C, 0, 0, paths=8), 8 * C)
    C = np.full((6, 9, 64), 62, np.int32)
    S = dp.aggregate_host(C, 255, 255, paths=8)
    assert S.max() == 8 * 62 <= 2536
    C = np.random.default_rng(84).integers(0, 63, (9, 12, 64)).astype(np.int32)
    for p1 in (0, 255):
        S = dp.aggregate_host(C, p1, 255, paths=8)
        assert 0 <= S.min() and S.max() <= 2536


def test_two_by_two_by_hand():
    """P1 = 3, P2 = 8, every cost 20 but C(0, 0, d = 5) = C(1, 1, 6) = C(0, 1, 10) = C(1, 0, 30) = 0, so M = 0 at every pixel and
    M + P2 = 8.  A path whose previous pixel is outside the 2 x 2 frame contributes C.

    S(1, 1, 6), C = 0: left -> right from (1, 0) (its zero is far away at d = 30): min(20, 23, 23, 8) = 8; top -> bottom from (0, 1)
    (zero at 10): 8; "\\" (+1, +1) from (0, 0), whose zero sits ONE candidate below, at d = 5: min(20, 0 + 3, 23, 8) = 3, the P1 step;
    the other five start here: 0.  S8 = 8 + 8 + 3 = 19, S4 = 16.
    S(0, 0, 5), C = 0: right -> left from (0, 1): 8; bottom -> top from (1, 0): 8; (-1, -1) from (1, 1), zero one above at d = 6:
    min(20, 23, 0 + 3, 8) = 3.  S8 = 19, S4 = 16.
    S(1, 0, 30), C = 0: right -> left from (1, 1): 8; top -> bottom from (0, 0): 8; "/" (+1, -1) from (0, 1), whose zero is 20
    candidates away: min(20, 23, 23, 0 + 8) = 8, the P2 term.  S8 = 24, S4 = 16.
    S(0, 1, 10), C = 0: left -> right from (0, 0): 8; bottom -> top from (1, 1): 8; (-1, +1) from (1, 0): 8.  S8 = 24, S4 = 16.
    S(1, 1, 0), C = 20, no d - 1 term: the three paths that arrive, from (1, 0), (0, 1) and (0, 0), give 20 + min(20, 23, 8) = 28
    each, the five that start 20 each: S8 = 3 * 28 + 5 * 20 = 184.
    S(1, 1, 5), C = 20: from (1, 0) and (0, 1) 28 each; "\\" from (0, 0) finds L(q, 5) = 0: 20 + 0 = 20; five starts 20 each:
    S8 = 2 * 28 + 6 * 20 = 176."""
    C = np.full((2, 2, 64), 20, np.int32)
    C[0, 0, 5] = C[1, 1, 6] = C[0, 1, 10] = C[1, 0, 30] = 0
    S8, S4 = dp.aggregate_host(C, 3, 8, paths=8), dp.aggregate_host(C, 3, 8, paths=4)
    assert (S8[1, 1, 6], S4[1, 1, 6]) == (19, 16)
    assert (S8[0, 0, 5], S4[0, 0, 5]) == (19, 16)
    assert (S8[1, 0, 30], S4[1, 0, 30]) == (24, 16)
    assert (S8[0, 1, 10], S4[0, 1, 10]) == (24, 16)
    assert S8[1, 1, 0] == 184 and S8[1, 1, 5] == 176


def test_default_is_four_paths():
    left, right = dc.two_plane_scene()[:2]
    plain = dp.sgm_host(left, right)
    assert np.array_equal(plain, dp.sgm_host(left, right, paths=4))
    assert np.array_equal(plain, dp.sgm_host(left, right, 0, 64, 7, 86, 10, 1, 0, 0, 4))             # paths is the last argument
    eight = dp.sgm_host(left, right, paths=8)
    assert eight.shape == plain.shape and eight.dtype == np.int16 and (eight != plain).any()
    assert np.array_equal(eight, dp.sgm_host(left, right, paths=np.int64(8)))
    both = dp.sgm_host(np.stack([left, left[::-1]]), np.stack([right, right[::-1]]), paths=8)          # a batch, frame by frame
    assert np.array_equal(both[0], eight) and np.array_equal(both[1], dp.sgm_host(left[::-1], right[::-1], paths=8))
    assert dp.PATHS == (4, 8)


@pytest.mark.parametrize("paths", [0, 5, 16, True, 8.0])
def test_refusals(paths):
    img = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError):
        dp.sgm_host(img, img, paths=paths)
    with pytest.raises(ValueError):
        dp.aggregate_host(np.zeros((2, 2, 64), np.int32), 7, 86, paths=paths)


def _bad_good(out, truth):
    valid = out != -16
    err = np.abs(out / 16.0 - truth)
    return int((valid & (err > 1.0)).sum()), int((valid & (err <= 1.0)).sum())


@pytest.mark.parametrize("seed", range(8))
def test_band_scene_eight_paths_beat_four(seed):
    """A 48 x 160 pair whose front plane (37 px before 12 px) is a band between two diagonal edges, default parameters: with eight
    paths strictly fewer valid pixels are more than 1 px off and strictly more are within 1 px.  Measured with this definition,
    (bad, good) for four -> eight paths: seed 0 (70, 5876) -> (51, 5938), 1 (49, 5882) -> (18, 5951), 2 (98, 5863) -> (71, 5916),
    3 (88, 5861) -> (68, 5915), 4 (79, 5886) -> (56, 5931), 5 (70, 5892) -> (43, 5936), 6 (82, 5863) -> (68, 5892),
    7 (122, 5846) -> (95, 5898)."""
    left, right, truth = d8.band_scene(seed)
    bad4, good4 = _bad_good(dp.sgm_host(left, right, paths=4), truth)
    bad8, good8 = _bad_good(dp.sgm_host(left, right, paths=8), truth)
    print(f"seed {seed}: four paths {bad4} bad / {good4} good, eight paths {bad8} / {good8}")
    assert bad8 < bad4 and good8 > good4


def test_host_accuracy_two_planes_eight_paths():
    """The axis-aligned scene of tests/test_disparity_host.py with ``paths=8``.  Measured with this definition: 84.6 % of the
    pixels valid; of the valid ones 98.5 % within 1 px of the truth and 94.5 % within 0.25 px; 97.9 % of the pixels that are neither
    occluded nor off the right frame valid (four paths: 84.9, 98.9, 94.8, 98.5: slightly better here, the diagonals cross the
    rectangle's corners).  The gates are those values less two percentage points."""
    left, right, truth, occluded, off_frame = dc.two_plane_scene()
    out = dp.sgm_host(left, right, paths=8)
    valid = out != -16
    assert (out[valid] >= 0).all()
    err = np.abs(out / 16.0 - truth)
    f_valid = valid.mean()
    f_1px = (err[valid] <= 1.0).mean()
    f_quarter = (err[valid] <= 0.25).mean()
    f_visible = valid[~occluded & ~off_frame].mean()
    print(f"valid {f_valid:.4f}, of those within 1 px {f_1px:.4f}, within 0.25 px {f_quarter:.4f}; visible pixels valid {f_visible:.4f}")
    assert f_valid >= 0.826 and f_1px >= 0.965 and f_quarter >= 0.925 and f_visible >= 0.959
