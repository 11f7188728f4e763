"""The device side of the speckle filter (csrc/dcx_speckle.hip through deepcharuco_amd/disparity.py) against its numpy definition:
every case bit for bit against ``filter_speckles_host``; sizes around the kernels' tile, shapes that stress the union-find, in
place and out of place, chunks, repeatability, the no-allocation call, the refusals and the matcher with the filter switched on."""
import numpy as np
import pytest
import torch

import disparity_cases as dc
import speckle_cases as sc
from deepcharuco_amd import _lib, disparity as dp

pytestmark = pytest.mark.gpu

TILE = 32                                    # csrc/dcx_speckle.hip: kTile, the side of the tile that one workgroup labels in LDS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _agree(dev, disp, new_val, size, diff, **kw):
    """filter_speckles_device against filter_speckles_host -> the host result."""
    want = dp.filter_speckles_host(disp, new_val, size, diff)
    src = torch.from_numpy(disp).to(dev)
    got = dp.filter_speckles_device(src, new_val, size, diff, **kw)
    assert got.dtype == torch.int16 and tuple(got.shape) == disp.shape and got.is_contiguous()
    got = got.cpu().numpy()
    differ = got != want
    assert not differ.any(), (disp.shape, new_val, size, diff, int(differ.sum()), np.argwhere(differ)[:5].tolist(), got[differ][:5],
                              want[differ][:5])
    assert np.array_equal(src.cpu().numpy(), disp)                            # out of place: the input is left alone
    return want


# ------------------------------------------------------------------------------------------------ the definition's cases

@pytest.mark.parametrize("case", sc.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(dev, case):
    _, disp, new_val, size, diff, expected = case
    assert np.array_equal(_agree(dev, disp, new_val, size, diff), expected)


# ------------------------------------------------------------------------------------------------ shapes

SIDES = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


@pytest.mark.parametrize("h", SIDES)
@pytest.mark.parametrize("w", SIDES)
def test_sizes_around_the_tile(dev, h, w):
    """Small components (max_diff 16: only equal values join) and ones that reach across tiles (max_diff 40), and the frame as one
    component at both sides of its size."""
    disp = sc.random_map(2, (h, w))
    _agree(dev, disp, sc.NV, 3, 16)
    _agree(dev, disp, sc.NV, 40, 40)
    flat = np.full((h, w), 77, np.int16)
    assert np.array_equal(_agree(dev, flat, sc.NV, h * w - 1, 0), flat)
    assert (_agree(dev, flat, sc.NV, h * w, 0) == sc.NV).all()


H3, W3 = 2 * TILE + 6, 2 * TILE + 3                                           # three tiles each way, the last ones cut


@pytest.mark.parametrize("name", ["serpentine", "serpentine_t", "spiral", "comb"])
def test_one_long_component(dev, name):
    """A one-pixel-wide component of L pixels that crosses the tile borders again and again (the serpentine's rows cross every
    vertical border, its transpose every horizontal one; the serpentine's values are a ramp in steps of max_diff): kept whole at
    max_speckle_size = L - 1, gone at L."""
    if name == "serpentine_t":
        disp, L = sc.serpentine(W3, H3)
        disp = np.ascontiguousarray(disp.T)
    else:
        disp, L = getattr(sc, name)(H3, W3)
    assert L == (disp != sc.NV).sum() > 1000
    assert np.array_equal(_agree(dev, disp, sc.NV, L - 1, 4), disp)
    assert (_agree(dev, disp, sc.NV, L, 4) == sc.NV).all()


def test_checkerboard_every_pixel_its_own_component(dev):
    board = sc.checkerboard(H3, W3)
    assert np.array_equal(_agree(dev, board, sc.NV, 0, 99), board)            # L = 1: kept at L - 1 = 0
    assert (_agree(dev, board, sc.NV, 1, 99) == sc.NV).all()


def test_constant_frame_is_one_component(dev):
    flat = np.full((H3, W3), 320, np.int16)
    assert np.array_equal(_agree(dev, flat, sc.NV, H3 * W3 - 1, 0), flat)
    assert (_agree(dev, flat, sc.NV, H3 * W3, 0) == sc.NV).all()


@pytest.mark.parametrize("shape", [(23, 131), (70, 65), (3, 23, 131)])
@pytest.mark.parametrize("diff,size", [(16, 3), (40, 40)])
def test_random_maps(dev, shape, diff, size):
    disp = sc.random_map(1, shape)
    want = _agree(dev, disp, sc.NV, size, diff)
    assert (want != disp).sum() >= 50 and (want != sc.NV).sum() >= 50         # neither an identity nor an all-new_val kernel passes


# ------------------------------------------------------------------------------------------------ buffers

def test_in_place_and_out_of_place(dev):
    disp = sc.random_map(3, (3, 40, 70))
    want = dp.filter_speckles_host(disp, sc.NV, 3, 16)
    src = torch.from_numpy(disp).to(dev)
    out = torch.full_like(src, 123)
    assert dp.filter_speckles_device(src, sc.NV, 3, 16, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), disp)
    assert dp.filter_speckles_device(src, sc.NV, 3, 16, out=src) is src
    assert np.array_equal(src.cpu().numpy(), want)


def test_batch_in_chunks_through_a_one_frame_workspace(dev):
    B, h, w = 3, 40, 70
    disp = sc.random_map(4, (B, h, w))
    disp[1, -1], disp[2, 0] = 80, 80                                          # frame 1 ends in the row that frame 2 starts with
    one = dp.filter_speckles_workspace_bytes(1, h, w)
    assert one == h * w * 8 and dp.filter_speckles_workspace_bytes(B, h, w) == B * one
    want = _agree(dev, disp, sc.NV, 3, 16)
    src = torch.from_numpy(disp).to(dev)
    for nbytes in (one, one + one // 2, 2 * one, 5 * one):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert np.array_equal(dp.filter_speckles_device(src, sc.NV, 3, 16, workspace=ws).cpu().numpy(), want), nbytes
    ws = torch.empty(one, dtype=torch.uint8, device=dev)
    assert np.array_equal(dp.filter_speckles_device(src, sc.NV, 3, 16, out=src, workspace=ws).cpu().numpy(), want)      # in place, chunked
    with pytest.raises(ValueError):
        dp.filter_speckles_device(src, sc.NV, 3, 16, workspace=ws[:one - 8])


def test_two_calls_give_equal_bits_and_nothing_is_allocated(dev):
    disp = sc.random_map(5, (3, 70, 65))
    src = torch.from_numpy(disp).to(dev)
    out = [torch.empty_like(src) for _ in range(2)]
    ws = torch.empty(dp.filter_speckles_workspace_bytes(3, 70, 65), dtype=torch.uint8, device=dev)
    dp.filter_speckles_device(src, sc.NV, 40, 40, out=out[0], workspace=ws)   # (the library is loaded by now)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert dp.filter_speckles_device(src, sc.NV, 40, 40, out=out[1], workspace=ws) is out[1]
    assert torch.cuda.memory_allocated(dev) == before
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])
    assert np.array_equal(out[1].cpu().numpy(), dp.filter_speckles_host(disp, sc.NV, 40, 40))


def test_device_refusals(dev):
    a = torch.zeros((8, 8), dtype=torch.int16, device=dev)
    dp.filter_speckles_device(a, -32768, 0, 65535)
    for bad in ((40000, 1, 1), (0, -1, 1), (0, 1, -1), (0, 1, 65536), (0, 1.0, 1)):
        with pytest.raises(ValueError):
            dp.filter_speckles_device(a, *bad)
    for t in (a.t(), a[:, :7], a.to(torch.int32), a.cpu(), a[:0], a[None, None]):
        with pytest.raises(ValueError):
            dp.filter_speckles_device(t, 0, 1, 1)
    for out in (torch.empty((8, 8), dtype=torch.int32, device=dev), torch.empty((8, 9), dtype=torch.int16, device=dev),
                torch.empty((8, 16), dtype=torch.int16, device=dev)[:, ::2]):
        with pytest.raises(ValueError):
            dp.filter_speckles_device(a, 0, 1, 1, out=out)
    ws = torch.empty(8 * 8 * 8 + 8, dtype=torch.uint8, device=dev)
    dp.filter_speckles_device(a, 0, 1, 1, workspace=ws)
    for bad_ws in (ws[:8 * 8 * 8 - 8], ws[4:], ws.to(torch.int16)):
        with pytest.raises(ValueError):
            dp.filter_speckles_device(a, 0, 1, 1, workspace=bad_ws)
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1, (1 << 20) + 1), (1, (1 << 15) + 1, 1 << 15)):
        with pytest.raises(ValueError):
            dp.filter_speckles_workspace_bytes(*shape)
    assert dp.filter_speckles_workspace_bytes(2, 1 << 15, 1 << 15) == 1 << 34
    # the C entry point's own codes (each returns before anything is launched)
    f = _lib.lib().dcx_filter_speckles_s16
    p, w, n, s = a.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream()
    E_ARG, E_SHAPE, E_WS = -1, -2, -3
    assert f(None, p, 1, 8, 8, 0, 1, 1, w, n, s) == E_ARG and f(p, None, 1, 8, 8, 0, 1, 1, w, n, s) == E_ARG
    assert f(p, p, 1, 8, 8, 0, 1, 1, None, n, s) == E_ARG and f(p, p, 1, 8, 8, 0, 1, 1, w + 4, n - 4, s) == E_ARG
    assert f(p + 1, p, 1, 8, 7, 0, 1, 1, w, n, s) == E_ARG and f(p, p + 1, 1, 8, 7, 0, 1, 1, w, n, s) == E_ARG
    assert f(p, p, 1, 8, 8, 32768, 1, 1, w, n, s) == E_ARG and f(p, p, 1, 8, 8, -32769, 1, 1, w, n, s) == E_ARG
    assert f(p, p, 1, 8, 8, 0, -1, 1, w, n, s) == E_ARG and f(p, p, 1, 8, 8, 0, 1, 65536, w, n, s) == E_ARG
    assert f(p, p, 0, 8, 8, 0, 1, 1, w, n, s) == E_SHAPE and f(p, p, 1, (1 << 15) + 1, 1 << 15, 0, 1, 1, w, n, s) == E_SHAPE
    assert f(p, p, 1, 8, 8, 0, 1, 1, w, 8 * 8 * 8 - 1, s) == E_WS
    torch.cuda.synchronize()
    assert not a.any()


# ------------------------------------------------------------------------------------------------ behind the matcher

def test_sgm_device_with_the_filter(dev):
    """The two-plane scene, and a batch of three through a workspace that holds one matcher frame and a half: the filter then works
    in the matcher's workspace, in place on its output."""
    left, right = (np.array(x) for x in dc.two_plane_scene()[:2])
    kw = dict(speckle_window_size=100, speckle_range=2)
    want = dp.sgm_host(left, right, **kw)
    plain = dp.sgm_host(left, right)
    assert (want != plain).sum() >= 50                                        # the filter has work to do here
    tl, tr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    assert np.array_equal(dp.sgm_device(tl, tr, **kw).cpu().numpy(), want)

    bl, br = np.stack([left, left[::-1], left[:, ::-1]]), np.stack([right, right[::-1], right[:, ::-1]])
    want3 = dp.sgm_host(bl, br, min_disparity=-3, **kw)
    assert (want3 != dp.sgm_host(bl, br, min_disparity=-3)).sum() >= 50       # (new_val follows min_disparity: -64 here)
    h, w = left.shape
    one = dp.sgm_workspace_bytes(1, h, w, 64)
    ws = torch.empty(one + one // 2, dtype=torch.uint8, device=dev)
    out = torch.empty((3, h, w), dtype=torch.int16, device=dev)
    tl, tr = torch.from_numpy(bl).to(dev), torch.from_numpy(br).to(dev)
    dp.sgm_device(tl, tr, min_disparity=-3, out=out, workspace=ws, **kw)     # (the library is loaded by now)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert dp.sgm_device(tl, tr, min_disparity=-3, out=out, workspace=ws, **kw) is out
    assert torch.cuda.memory_allocated(dev) == before
    assert np.array_equal(out.cpu().numpy(), want3)
    assert np.array_equal(dp.sgm_device(tl, tr, min_disparity=-3, **kw).cpu().numpy(), want3)
    for bad in (dict(speckle_window_size=-1), dict(speckle_range=4096), dict(speckle_window_size=1.5)):
        with pytest.raises(ValueError):
            dp.sgm_device(tl, tr, **bad)


def test_sgm_device_defaults_are_todays_call(dev):
    left, right = (np.array(x) for x in dc.two_plane_scene()[:2])
    tl, tr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    today = dp.sgm_device(tl, tr)
    assert torch.equal(dp.sgm_device(tl, tr, speckle_window_size=0, speckle_range=0), today)
    assert torch.equal(dp.sgm_device(tl, tr, 0, 64, 7, 86, 10, 1, None, None, 0, 7), today)          # the window switches it on, not the range
    assert np.array_equal(today.cpu().numpy(), dp.sgm_host(left, right))
