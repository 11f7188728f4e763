"""resize.resize_device(..., "area_any") (csrc/dcx_resize.hip: dcx_resize_area_u8) against resize.resize_host, bit for bit: every
shape of tests/resize_any_cases.py, gray and BGR, batches of 1, 3 and 9, dense and through pitched, cropped and stepped views;
outputs between guards; repeatability and graph replay beside an "area" call; the refusals; and the detector behind the resize of
a 1080 x 1440 window, the 4:3 window of a 1080p frame."""
import numpy as np
import pytest
import torch

import resize_any_cases as ac
from guarded import Guarded
from deepcharuco_amd import resize as rz

pytestmark = pytest.mark.gpu

MODE = ac.MODE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _source(kind, batch, sh, sw, ch, seed):
    shape = (batch, sh, sw) + ((3,) if ch == 3 else ())
    return ac.noise(shape, seed) if kind == "noise" else ac.extremes(shape, seed)


@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_device_equals_host(dev, shape):
    sh, sw, dh, dw = shape
    for ch in (1, 3):
        for kind in ("noise", "extremes"):
            full = _source(kind, 9, sh, sw, ch, sh * 131 + sw)
            exp = rz.resize_host(full, (dh, dw), MODE)                       # once per layout, shared by the batches
            exp.flags.writeable = False
            for batch in (1, 3, 9):
                got = rz.resize_device(torch.from_numpy(full[:batch]).to(dev), (dh, dw), MODE)
                assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == exp[:batch].shape
                bad = int((got.cpu().numpy() != exp[:batch]).sum())
                assert bad == 0, f"{ac.shape_id(shape)} ch {ch} {kind} batch {batch}: {bad} bytes differ"
    one = torch.from_numpy(full[0]).to(dev)                                  # a single frame without the batch axis: (H, W, 3)
    assert np.array_equal(rz.resize_device(one, (dh, dw), MODE).cpu().numpy(), exp[0])
    gray = torch.from_numpy(np.ascontiguousarray(full[0, :, :, 1])).to(dev)  # (H, W)
    assert np.array_equal(rz.resize_device(gray, (dh, dw), MODE).cpu().numpy(), exp[0, :, :, 1])


@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_pitched_cropped_and_stepped_views(dev, shape):
    """The window big[:, 3:3+sh, 5:5+sw] of larger frames (an odd base address and a pitch beyond the row: once a pitch that is no
    multiple of 16, so every staged row starts at another alignment, once one that is) and stepped batches."""
    sh, sw, dh, dw = shape
    for ch, wide in ((1, sw + 14 + (sw % 16 == 2)), (3, sw + 14 + (sw % 16 == 2)), (1, (sw + 29) // 16 * 16), (3, (sw + 29) // 16 * 16)):
        assert (wide * ch % 16 == 0) == (wide % 16 == 0)
        big = _source("noise", 6, sh + 7, wide, ch, sh * 17 + sw + ch)
        d_big = torch.from_numpy(big).to(dev)
        view = d_big[:, 3:3 + sh, 5:5 + sw]
        assert not view.is_contiguous()
        exp = rz.resize_host(np.ascontiguousarray(big[:, 3:3 + sh, 5:5 + sw]), (dh, dw), MODE)
        assert np.array_equal(rz.resize_device(view, (dh, dw), MODE).cpu().numpy(), exp)
        assert np.array_equal(rz.resize_device(view[::2], (dh, dw), MODE).cpu().numpy(), exp[::2])
        assert np.array_equal(rz.resize_device(view[1::3], (dh, dw), MODE).cpu().numpy(), exp[1::3])
        assert np.array_equal(rz.resize_device(view[4], (dh, dw), MODE).cpu().numpy(), exp[4])
        assert torch.equal(d_big, torch.from_numpy(big).to(dev))             # the source is only read


def test_output_between_guards(dev):
    """``out=`` an exact-size buffer at an odd address between guards: every byte of it is written, none beside it."""
    for sh, sw, dh, dw in ((9, 9, 2, 2), (54, 72, 12, 16), (127, 900, 2, 400), (9, 900, 2, 400), (15, 14, 5, 7)):
        for ch, batch in ((1, 3), (3, 2)):
            src = _source("noise", batch, sh, sw, ch, 7)
            exp = rz.resize_host(src, (dh, dw), MODE)
            for fill in (0xC3, 0x3C):                                        # two fills: a byte left unwritten shows under one
                g = Guarded(dev, exp.shape, torch.uint8, fill, align=16, offset=1)
                got = rz.resize_device(torch.from_numpy(src).to(dev), (dh, dw), MODE, out=g.t)
                assert got is g.t
                assert g.guards_ok() is None, (sh, sw, ch, g.guards_ok())
                assert np.array_equal(g.cpu(), exp)
    with pytest.raises(ValueError):
        rz.resize_device(torch.from_numpy(src).to(dev), (dh, dw), MODE, out=torch.empty((1, dh, dw, 3), dtype=torch.uint8, device=dev))


def test_refusals_on_the_device(dev):
    x = torch.zeros((2, 10, 10), dtype=torch.uint8, device=dev)
    assert tuple(rz.resize_device(x, (3, 3), MODE).shape) == (2, 3, 3)
    with pytest.raises(ValueError):
        rz.resize_device(x, (11, 5), MODE)                                   # area does not enlarge, on either axis
    with pytest.raises(ValueError):
        rz.resize_device(x, (5, 11), MODE)
    with pytest.raises(ValueError):
        rz.resize_device(torch.zeros((1, 129, 4), dtype=torch.uint8, device=dev), (2, 3), MODE)   # 64.5
    with pytest.raises(ValueError):
        rz.resize_device(x.float(), (5, 5), MODE)
    with pytest.raises(ValueError):
        rz.resize_device(x.cpu(), (5, 5), MODE)
    with pytest.raises(ValueError):
        rz.resize_device(x[:, :, ::2], (3, 3), MODE)                         # pixels of a row must be contiguous
    with pytest.raises(ValueError):
        rz.resize_device(x, (3, 3), "area")                                  # the old mode still refuses a fractional factor


def test_two_calls_and_two_replays_give_the_same_bits(dev):
    """No allocation and no synchronisation with ``out`` given: an "area_any" call on a 4.5 x window and an "area" call captured
    in one graph replay to the eager bits, twice, from a pitched BGR view."""
    sh, sw, dh, dw = 54, 72, 12, 16
    big = torch.from_numpy(ac.noise((5, sh + 4, sw + 9, 3), 21)).to(dev)
    view = big[:, 2:2 + sh, 7:7 + sw]
    calls = {"any": (view, MODE), "area": (view[:, :48, :64], "area")}       # 4.5 x; 4 x
    eager = {k: rz.resize_device(v, (dh, dw), m) for k, (v, m) in calls.items()}
    for k, (v, m) in calls.items():
        assert torch.equal(rz.resize_device(v, (dh, dw), m), eager[k])
        assert np.array_equal(eager[k].cpu().numpy(), rz.resize_host(v.cpu().numpy(), (dh, dw), m))
    out = {k: torch.zeros_like(eager[k]) for k in calls}

    def enqueue():
        for k, (v, m) in calls.items():
            rz.resize_device(v, (dh, dw), m, out=out[k])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # warm-up launch outside the capture
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    for _ in range(2):
        for k in calls:
            out[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in calls:
            assert torch.equal(out[k], eager[k]), k


# ------------------------------------------------------------------------------------------------ the detector behind the resize

def test_detector_behind_a_fractional_resize(dev):
    """A golden 240 x 320 frame blown up to 1080 x 1440 with "linear" (which may enlarge): the 4:3 window of a 1080p frame, a factor
    of 4.5.  infer_batch_resized with its default mode returns, row for row, map_points of what infer_batch finds on
    resize_host(big, (240, 320), "area_any"); with "area" the same call still raises."""
    from conftest import GoldenCase
    from deepcharuco_amd.inference import infer_batch
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    case = GoldenCase("board_240x320")
    dc, rn = lModel(dcModel(case.n_ids, case.sd_dc, dev)), lRefineNet(RefineNet(case.sd_rn, dev))
    big = rz.resize_host(case.frame, (1080, 1440), "linear")
    assert big.shape == (1080, 1440) and big.dtype == np.uint8
    small = rz.resize_host(big, (240, 320), MODE)
    assert np.array_equal(rz.resize_device(torch.from_numpy(big).to(dev), (240, 320), MODE).cpu().numpy(), small)
    found = infer_batch(small[None], case.n_ids, dc, rn)[0]
    assert found.ndim == 2 and found.shape[0] > 0 and found.shape[1] == 3
    exp = rz.map_points(found, (1080, 1440), (240, 320))
    got = rz.infer_batch_resized(big[None], (240, 320), case.n_ids, dc, rn)
    assert len(got) == 1 and got[0].dtype == np.float64 and np.array_equal(got[0], exp)
    wide = torch.zeros((2, 1080, 1920), dtype=torch.uint8, device=dev)       # the window read in place from 1080p frames
    wide[:, :, 240:1680] = torch.from_numpy(big).to(dev)
    got = rz.infer_batch_resized(wide[:, :, 240:1680], (240, 320), case.n_ids, dc, rn)
    assert len(got) == 2 and all(np.array_equal(g, exp) for g in got)
    with pytest.raises(ValueError):
        rz.infer_batch_resized(big[None], (240, 320), case.n_ids, dc, rn, interpolation="area")
