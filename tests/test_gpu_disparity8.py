"""The eight-path matcher on the device (the diagonal kernels of csrc/dcx_sgm.hip through ``sgm_device(..., paths=8)``): every case
bit for bit against ``sgm_host(..., paths=8)``.  A wave of the diagonal kernels owns a start column and wraps across the frame
edge, so the shapes are those at which that can go wrong: one row, one column, 2 x 2, square, widths around 64, tall frames that
wrap several times, heights and widths of 64 against 7."""
import numpy as np
import pytest
import torch

import disparity8_cases as d8
import disparity_cases as dc
from deepcharuco_amd import _lib, disparity as dp

pytestmark = pytest.mark.gpu

DEFAULTS = dict(min_disparity=0, num_disparities=64, p1=7, p2=86, uniqueness=10, lr_max_diff=1, paths=8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _mixed_pair(seed, h, w, d_a=9, d_b=3):
    """A textured pair: disparity d_a in the upper half, d_b in the lower, a few columns of noise: valid and invalid pixels, and
    winners that change along every path direction."""
    rng = np.random.default_rng([43, seed, h, w])
    la, ra = dc.shifted_pair(rng, h, w, d_a)
    lb, rb = dc.shifted_pair(rng, h, w, d_b)
    left, right = la.copy(), ra.copy()
    left[h // 2:], right[h // 2:] = lb[h // 2:], rb[h // 2:]
    if w > 8:
        right[:, w // 2:w // 2 + 3] = rng.integers(0, 256, (h, 3), dtype=np.uint8)
    return left, right


def _agree(dev, left, right, **kw):
    """sgm_device against sgm_host on one pair or batch, eight paths unless told otherwise -> the host result."""
    par = dict(DEFAULTS, **kw)
    want = dp.sgm_host(left, right, **par)
    got = dp.sgm_device(torch.from_numpy(np.ascontiguousarray(left)).to(dev), torch.from_numpy(np.ascontiguousarray(right)).to(dev), **par)
    assert got.dtype == torch.int16 and tuple(got.shape) == left.shape and got.is_contiguous()
    got = got.cpu().numpy()
    differ = got != want
    assert not differ.any(), (par, left.shape, int(differ.sum()), np.argwhere(differ)[:5].tolist(), got[differ][:5], want[differ][:5])
    return want


# ------------------------------------------------------------------------------------------------ shapes

@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (23, 1), (2, 2), (9, 9), (9, 63), (9, 64), (9, 65), (9, 131), (23, 5), (64, 7), (7, 64)])
def test_shapes(dev, h, w):
    """(23, 5) and (64, 7): a start-column wave wraps 4 and 9 times and the diagonals' lengths saturate at W; (1, w) and (h, 1):
    every diagonal has one pixel."""
    out = _agree(dev, *_mixed_pair(0, h, w))
    if w >= 63:
        assert (out != -16).any() and (out == -16).any()


@pytest.mark.parametrize("w,D", [(130, 128), (40, 256), (300, 256)])
def test_more_than_one_disparity_to_a_lane(dev, w, D):
    left, right = _mixed_pair(1, 9, w, *((200, 70) if w == 300 else (9, 3)))
    out = _agree(dev, left, right, num_disparities=D)
    if w == 300:
        assert (out[:4, 210:] // 16 == 200).any() and (out[5:, 80:] // 16 == 70).any()     # (both planes win somewhere)


# ------------------------------------------------------------------------------------------------ parameters

@pytest.mark.parametrize("m", [0, 5, -16])
def test_min_disparity(dev, m):
    out = _agree(dev, *_mixed_pair(3, 9, 70), min_disparity=m)
    assert (out != 16 * (m - 1)).any()
    _agree(dev, *_mixed_pair(3, 9, 70, 20, 0), min_disparity=m, num_disparities=128)


@pytest.mark.parametrize("p1,p2", [(0, 0), (7, 86), (255, 255), (0, 255)])
def test_penalties(dev, p1, p2):
    _agree(dev, *_mixed_pair(4, 12, 70), p1=p1, p2=p2)


@pytest.mark.parametrize("uniqueness", [0, 99])
@pytest.mark.parametrize("lr", [-1, 0, 1])
def test_uniqueness_and_left_right_check(dev, uniqueness, lr):
    _agree(dev, *_mixed_pair(5, 12, 70), uniqueness=uniqueness, lr_max_diff=lr)


# ------------------------------------------------------------------------------------------------ content

def test_noise(dev):
    rng = np.random.default_rng(6)
    left, right = rng.integers(0, 256, (2, 23, 131), dtype=np.uint8)
    out = _agree(dev, left, right)
    assert (out == -16).mean() > 0.5
    _agree(dev, left, right, uniqueness=0, lr_max_diff=-1)                   # the same S with every winner kept


@pytest.mark.parametrize("D", [64, 256])
def test_constant_frames_tie_everywhere(dev, D):
    img = np.full((9, 70), 93, np.uint8)
    assert not _agree(dev, img, img, num_disparities=D).any()
    assert (_agree(dev, img, img, num_disparities=D, min_disparity=5)[:, 5:] == 80).all()


def test_band_scene(dev):
    left, right, _ = d8.band_scene(0)
    eight = _agree(dev, np.array(left), np.array(right))
    four = _agree(dev, np.array(left), np.array(right), paths=4)
    assert (eight != four).any()


def test_two_plane_scene(dev):
    left, right, truth, occluded, off_frame = dc.two_plane_scene()
    out = _agree(dev, np.array(left), np.array(right))
    assert (out != -16)[~occluded & ~off_frame].mean() >= 0.959               # (the host test's gate: the case is not degenerate)


# ------------------------------------------------------------------------------------------------ batch and layout

def test_batch_chunks_strides_and_an_odd_address(dev):
    """A batch of 3 in one pass and with a workspace that holds one frame and a half (chunks of one frame); the left frames at pitch
    80 with 33 spare bytes between frames, starting 5 bytes into their buffer; the right frames at pitch 75, 7 spare bytes."""
    h, w, B = 11, 70, 3
    pairs = [_mixed_pair(10 + i, h, w, 9 + i, 2 * i) for i in range(B)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = _agree(dev, left, right)
    _agree(dev, left[:1], right[:1])
    one = dp.sgm_workspace_bytes(1, h, w, 64)
    ws = torch.empty(one + one // 2, dtype=torch.uint8, device=dev)
    got = dp.sgm_device(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), workspace=ws, paths=8)
    assert np.array_equal(got.cpu().numpy(), want)

    def strided(frames, pitch, spare, offset):
        stride = h * pitch + spare
        buf = torch.full((offset + B * stride,), 255, dtype=torch.uint8, device=dev)
        view = torch.as_strided(buf, (B, h, w), (stride, pitch, 1), offset)
        view.copy_(torch.from_numpy(frames).to(dev))
        return view

    ls, rs = strided(left, 80, 33, 5), strided(right, 75, 7, 0)
    assert ls.data_ptr() % 2 == 1
    assert np.array_equal(dp.sgm_device(ls, rs, paths=8).cpu().numpy(), want)
    assert np.array_equal(dp.sgm_device(ls, rs, workspace=ws, paths=8).cpu().numpy(), want)
    assert np.array_equal(dp.sgm_device(ls[1], rs[1], paths=8).cpu().numpy(), want[1])


def test_with_the_speckle_filter(dev):
    left, right = (np.array(a) for a in dc.two_plane_scene()[:2])
    kw = dict(speckle_window_size=100, speckle_range=2)
    want = _agree(dev, left, right, **kw)
    assert (want != dp.sgm_host(left, right, paths=8)).any()                   # (the filter removes something)


def test_two_calls_give_equal_bits_and_nothing_is_allocated(dev):
    rng = np.random.default_rng(8)
    left, right = (torch.from_numpy(a).to(dev) for a in rng.integers(0, 256, (2, 3, 23, 131), dtype=np.uint8))
    out = [torch.empty((3, 23, 131), dtype=torch.int16, device=dev) for _ in range(2)]
    ws = torch.empty(dp.sgm_workspace_bytes(3, 23, 131, 128), dtype=torch.uint8, device=dev)
    dp.sgm_device(left, right, num_disparities=128, out=out[0], workspace=ws, paths=8)   # (the library is loaded by now)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert dp.sgm_device(left, right, num_disparities=128, out=out[1], workspace=ws, paths=8) is out[1]
    assert torch.cuda.memory_allocated(dev) == before
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])
    assert np.array_equal(out[1].cpu().numpy(), dp.sgm_host(left.cpu().numpy(), right.cpu().numpy(), num_disparities=128, paths=8))


# ------------------------------------------------------------------------------------------------ four paths, and the refusals

def _c_call(fn, left, right, out, ws, *tail):
    h, w = left.shape
    return fn(left.data_ptr(), 0, w, right.data_ptr(), 0, w, 1, h, w, 0, 64, 7, 86, 10, 1, *tail, out.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.current_stream())


def test_four_paths_through_the_new_entry_point(dev):
    """``paths=4`` is the old call: sgm_device (which calls dcx_sgm_u8_paths) and both C functions give the same bits."""
    left, right = (torch.from_numpy(a).to(dev) for a in _mixed_pair(0, 9, 131))
    ws = torch.empty(dp.sgm_workspace_bytes(1, 9, 131, 64), dtype=torch.uint8, device=dev)
    old, new = (torch.full((9, 131), 77, dtype=torch.int16, device=dev) for _ in range(2))
    lib = _lib.lib()
    assert _c_call(lib.dcx_sgm_u8, left, right, old, ws) == 0
    assert _c_call(lib.dcx_sgm_u8_paths, left, right, new, ws, 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(old, new)
    assert torch.equal(dp.sgm_device(left, right, paths=4), old) and torch.equal(dp.sgm_device(left, right), old)
    assert np.array_equal(old.cpu().numpy(), dp.sgm_host(left.cpu().numpy(), right.cpu().numpy()))


def test_refusals(dev):
    left, right = (torch.from_numpy(a).to(dev) for a in _mixed_pair(0, 9, 70))
    for bad in (5, 0, 16, True, 8.0):
        with pytest.raises(ValueError):
            dp.sgm_device(left, right, paths=bad)
    ws = torch.empty(dp.sgm_workspace_bytes(1, 9, 70, 64), dtype=torch.uint8, device=dev)
    out = torch.full((9, 70), 77, dtype=torch.int16, device=dev)
    for bad in (5, 0, -8):
        assert _c_call(_lib.lib().dcx_sgm_u8_paths, left, right, out, ws, bad) == -1               # DCX_E_ARG
    torch.cuda.synchronize()
    assert (out == 77).all()                                                  # nothing was launched
