"""The scenes of tests/disparity_limit_cases.py under the host definitions alone (``sgm_host``, ``filter_speckles_host``): each one
is shown to be non-degenerate, so that a device test on it cannot pass on an all-invalid or an all-equal map, and the inputs that a
graph replay swaps in are shown to change the answer.  tests/test_gpu_disparity_limits.py and tests/test_gpu_disparity_graph.py
hold the kernels to the same expectations bit for bit."""
import numpy as np
import pytest

import disparity_limit_cases as lc
from deepcharuco_amd import disparity as dp


def _both(out, invalid=-16):
    return (out == invalid).any() and (out != invalid).any()


# ------------------------------------------------------------------------------------------------ B1, B2

@pytest.mark.parametrize("h,D,paths", [(3, 64, 8), (3, 64, 4), (2, 256, 8), (1, 64, 8)])
def test_wide_pairs_have_valid_and_invalid_pixels(h, D, paths):
    left, right = lc.wide_pair(h)
    assert left.shape == (h, lc.MAX_WIDTH) == (h, dp.MAX_DEVICE_WIDTH)
    out = dp.sgm_host(left, right, num_disparities=D, paths=paths)
    valid = out != -16
    print(f"{h} x 4096, D = {D}, {paths} paths: {valid.mean():.4f} valid")
    assert valid.mean() > 0.99 and not valid.all()
    assert (np.abs(out[valid] - 16 * 9) <= 8).mean() > 0.99                   # the true disparity, to half a pixel


@pytest.mark.parametrize("w", [3, 1])
def test_tall_pairs_have_valid_and_invalid_pixels(w):
    left, right = lc.tall_pair(w)
    assert left.shape == (2100, w)
    out = dp.sgm_host(left, right, paths=8)
    valid = out != -16
    print(f"2100 x {w}: {valid.mean():.3f} valid")
    assert 0.3 < valid.mean() < 0.8
    if w == 1:                                                                # (one column: a pixel is valid where the census words agree)
        third = 2100 // 3
        assert valid[:third].mean() > valid[third:2 * third].mean() + 0.3    # the rows whose right frame is noise are the invalid ones
    else:
        assert (out != dp.sgm_host(left, right, paths=4)).any()               # the diagonals matter in a frame three pixels wide


# ------------------------------------------------------------------------------------------------ B3, B4

def test_the_matcher_period():
    left, right = lc.sgm_period()
    assert left.shape == (lc.SGM_PERIOD,) + lc.SMALL and lc.SGM_CHUNK_CAP % lc.SGM_PERIOD == 4
    out = dp.sgm_host(left, right, paths=8)
    assert _both(out)
    assert len({f.tobytes() for f in out}) == lc.SGM_PERIOD                   # no two frames of the period give the same map
    filtered = dp.sgm_host(left, right, paths=8, **lc.SMALL_SPECKLE)
    assert (filtered != out).any() and (filtered != -16).any()
    assert len({f.tobytes() for f in filtered}) >= 3
    assert np.array_equal(lc.tiled(out, 16)[7:14], out) and np.array_equal(lc.tiled(out, 16)[14:], out[:2])


def test_the_filter_period():
    disp = lc.speckle_period()
    assert disp.shape == (lc.SPECKLE_PERIOD,) + lc.SMALL and lc.SPECKLE_CHUNK_CAP % lc.SPECKLE_PERIOD == 10
    out = dp.filter_speckles_host(disp, *lc.SMALL_FILTER)
    assert (out != disp).any((1, 2)).any() and (out != lc.NV).any()
    assert len({f.tobytes() for f in out}) >= 3
    assert not np.array_equal(out[0], out[lc.SPECKLE_CHUNK_CAP % lc.SPECKLE_PERIOD])      # the tail's frame against frame 0


# ------------------------------------------------------------------------------------------------ B5

@pytest.mark.parametrize("end", ["low", "high"])
def test_edge_scenes(end):
    e = lc.EDGES[end]
    m, D = e["min_disparity"], e["num_disparities"]
    left, right, match = lc.edge_scene(end)
    assert left.shape == (lc.EDGE_H, e["width"]) and 50 <= match.sum() <= 70
    assert e["true"] in (m, m + D - 1)                                        # the candidate range's edge, not its interior
    out = dp.sgm_host(left, right, min_disparity=m, num_disparities=D, paths=8)
    hold = (out[:, match] == 16 * e["true"]).mean()
    gone = (out[:, ~match] == 16 * (m - 1)).mean()
    print(f"{end}: {hold:.3f} of the match columns hold {16 * e['true']}, {gone:.3f} of the others are invalid")
    assert hold >= 0.9 and gone >= 0.95
    assert 16 * e["true"] == (-32752 if end == "low" else 32736) and (end == "high" or 16 * (m - 1) == -32768)


def test_no_candidate_on_the_frame():
    left, right = lc.narrow_pair()
    assert (dp.sgm_host(left, right, min_disparity=-2047, paths=8) == -32768).all()


# ------------------------------------------------------------------------------------------------ A1 - A3, B6, B7

@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("window", [0, 100])
def test_the_swapped_in_frames_change_the_matcher_s_answer(paths, window):
    kw = dict(min_disparity=-3, paths=paths, speckle_window_size=window, speckle_range=2)
    first, second = (dp.sgm_host(*lc.small_batch(s), **kw) for s in (0, 1))
    for a, b in zip(first, second):
        assert (a != b).mean() > 0.5
    assert _both(first, -64) and _both(second, -64)


def test_the_swapped_in_map_changes_the_filter_s_answer():
    first, second = (dp.filter_speckles_host(lc.speckle_batch(s), *lc.FILTER) for s in (7, 8))
    for s, out in ((7, first), (8, second)):
        assert ((out != lc.speckle_batch(s)).sum((1, 2)) >= 50).all() and ((out != lc.NV).sum((1, 2)) >= 50).all()
    for a, b in zip(first, second):
        assert (a != b).mean() > 0.3


def test_the_reordered_two_plane_batch_changes_every_frame():
    kw = dict(min_disparity=-3, paths=8, **lc.SPECKLE)
    first = dp.sgm_host(*lc.two_plane_batch(), **kw)
    second = dp.sgm_host(*lc.two_plane_batch(lc.REORDER), **kw)
    assert np.array_equal(second, first[list(lc.REORDER)])
    for a, b in zip(first, second):
        assert (a != b).mean() > 0.3
    assert (first != dp.sgm_host(*lc.two_plane_batch(), min_disparity=-3, paths=8)).sum() >= 50      # the filter has work to do


def test_the_broadcast_batch():
    left, right = lc.broadcast_batch()
    out = dp.sgm_host(np.broadcast_to(left, right.shape), right)
    assert _both(out)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert (out[a] != out[b]).mean() > 0.5
