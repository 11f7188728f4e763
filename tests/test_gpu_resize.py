"""resize.resize_device (csrc/dcx_resize.hip) against resize.resize_host, bit for bit: every shape of tests/resize_cases.py in every
mode it is defined for, gray and BGR, batches of 1, 3 and 9, dense and through pitched, cropped and stepped views; outputs between
guards; repeatability and graph replay; and the detector behind a resize against the detector on the frame itself."""
import numpy as np
import pytest
import torch

import resize_cases as rc
from guarded import Guarded
from deepcharuco_amd import resize as rz

pytestmark = pytest.mark.gpu

CASES = rc.all_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_host = {}


def _expected(key, frames, size, mode):
    """resize_host, computed once per (case, layout) and shared."""
    if key not in _host:
        _host[key] = rz.resize_host(frames, size, mode)
        _host[key].flags.writeable = False
    return _host[key]


def _source(kind, batch, sh, sw, ch, seed):
    shape = (batch, sh, sw) + ((3,) if ch == 3 else ())
    return rc.noise(shape, seed) if kind == "noise" else rc.extremes(shape, seed)


@pytest.mark.parametrize("case", CASES, ids=rc.case_id)
def test_device_equals_host(dev, case):
    mode, (sh, sw, dh, dw) = case
    for ch in (1, 3):
        for kind in ("noise", "extremes"):
            full = _source(kind, 9, sh, sw, ch, sh * 131 + sw)
            exp = _expected((case, ch, kind), full, (dh, dw), mode)
            for batch in (1, 3, 9):
                got = rz.resize_device(torch.from_numpy(full[:batch]).to(dev), (dh, dw), mode)
                assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == exp[:batch].shape
                bad = int((got.cpu().numpy() != exp[:batch]).sum())
                assert bad == 0, f"{rc.case_id(case)} ch {ch} {kind} batch {batch}: {bad} bytes differ"
    one = torch.from_numpy(full[0]).to(dev)                                  # a single frame without the batch axis: (H, W, 3)
    assert np.array_equal(rz.resize_device(one, (dh, dw), mode).cpu().numpy(), exp[0])
    gray = torch.from_numpy(np.ascontiguousarray(full[0, :, :, 1])).to(dev)  # (H, W)
    assert np.array_equal(rz.resize_device(gray, (dh, dw), mode).cpu().numpy(), exp[0, :, :, 1])


@pytest.mark.parametrize("case", CASES, ids=rc.case_id)
def test_pitched_cropped_and_stepped_views(dev, case):
    """The window big[:, 3:3+sh, 5:5+sw] of larger frames (an odd base address and a pitch beyond the row: once a pitch that is no
    multiple of 16, so every staged row starts at another alignment, once one that is, where "area" takes its row-sum kernel)
    and every second frame of the batch."""
    mode, (sh, sw, dh, dw) = case
    for ch, wide in ((1, sw + 14 + (sw % 16 == 2)), (3, sw + 14 + (sw % 16 == 2)), (1, (sw + 29) // 16 * 16), (3, (sw + 29) // 16 * 16)):
        assert (wide * ch % 16 == 0) == (wide % 16 == 0)
        big = _source("noise", 6, sh + 7, wide, ch, sh * 17 + sw + ch)
        d_big = torch.from_numpy(big).to(dev)
        view = d_big[:, 3:3 + sh, 5:5 + sw]
        assert not view.is_contiguous()
        exp = rz.resize_host(np.ascontiguousarray(big[:, 3:3 + sh, 5:5 + sw]), (dh, dw), mode)
        assert np.array_equal(rz.resize_device(view, (dh, dw), mode).cpu().numpy(), exp)
        assert np.array_equal(rz.resize_device(view[::2], (dh, dw), mode).cpu().numpy(), exp[::2])
        assert np.array_equal(rz.resize_device(view[1::3], (dh, dw), mode).cpu().numpy(), exp[1::3])
        assert np.array_equal(rz.resize_device(view[4], (dh, dw), mode).cpu().numpy(), exp[4])
    assert torch.equal(d_big, torch.from_numpy(big).to(dev))                 # the source is only read


@pytest.mark.parametrize("mode", rc.MODES)
def test_output_between_guards(dev, mode):
    """``out=`` an exact-size buffer at an odd address between guards: every byte of it is written, none beside it."""
    for sh, sw, dh, dw in rc.shapes(mode)[:3] + [rc.COMMON_SHAPE]:
        for ch, batch in ((1, 3), (3, 2)):
            src = _source("noise", batch, sh, sw, ch, 7)
            exp = rz.resize_host(src, (dh, dw), mode)
            for fill in (0xC3, 0x3C):                                        # two fills: a byte left unwritten shows under one
                g = Guarded(dev, exp.shape, torch.uint8, fill, align=16, offset=1)
                got = rz.resize_device(torch.from_numpy(src).to(dev), (dh, dw), mode, out=g.t)
                assert got is g.t
                assert g.guards_ok() is None, (mode, sh, sw, ch, g.guards_ok())
                assert np.array_equal(g.cpu(), exp)
    with pytest.raises(ValueError):
        rz.resize_device(torch.from_numpy(src).to(dev), (dh, dw), mode, out=torch.empty((1, dh, dw, 3), dtype=torch.uint8, device=dev))


def test_refusals_on_the_device(dev):
    x = torch.zeros((2, 10, 10), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        rz.resize_device(x, (3, 3), "area")
    with pytest.raises(ValueError):
        rz.resize_device(x.float(), (5, 5))
    with pytest.raises(ValueError):
        rz.resize_device(x.cpu(), (5, 5))
    with pytest.raises(ValueError):
        rz.resize_device(x[:, :, ::2], (5, 5))                               # pixels of a row must be contiguous
    with pytest.raises(ValueError):
        rz.resize_device(x, (5, 5), "cubic")


def test_two_calls_and_two_replays_give_the_same_bits(dev):
    """No allocation and no synchronisation with ``out`` given: the three modes captured in one graph replay to the eager bits,
    twice, from a pitched BGR view."""
    sh, sw, dh, dw = rc.COMMON_SHAPE
    big = torch.from_numpy(rc.noise((5, sh + 4, sw + 9, 3), 21)).to(dev)
    view = big[:, 2:2 + sh, 7:7 + sw]
    eager = {m: rz.resize_device(view, (dh, dw), m) for m in rc.MODES}
    for m in rc.MODES:
        assert torch.equal(rz.resize_device(view, (dh, dw), m), eager[m])
        assert np.array_equal(eager[m].cpu().numpy(), rz.resize_host(view.cpu().numpy(), (dh, dw), m))
    out = {m: torch.zeros_like(eager[m]) for m in rc.MODES}

    def enqueue():
        for m in rc.MODES:
            rz.resize_device(view, (dh, dw), m, out=out[m])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # warm-up launch outside the capture
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    for _ in range(2):
        for m in rc.MODES:
            out[m].zero_()
        g.replay()
        torch.cuda.synchronize()
        for m in rc.MODES:
            assert torch.equal(out[m], eager[m]), m


# ------------------------------------------------------------------------------------------------ the detector behind a resize

@pytest.mark.parametrize("name", ["board_240x320", "img7412_240x320"])
def test_detector_behind_a_resize(dev, name):
    """A fixture frame blown up 4 x 4 (for the photo: its BGR image) comes back as itself under every mode, so the detector behind
    the resize finds the fixture's corners, and infer_batch_resized returns them in the large frame's pixels: row for row
    map_points of what infer_batch finds on the frame itself."""
    from conftest import GoldenCase
    from deepcharuco_amd.inference import infer_batch
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    case = GoldenCase(name)
    dc, rn = lModel(dcModel(case.n_ids, case.sd_dc, dev)), lRefineNet(RefineNet(case.sd_rn, dev))
    frame = case.bgr if name.startswith("img7412") else case.frame
    ones = np.ones((4, 4, 1) if frame.ndim == 3 else (4, 4), np.uint8)
    big = np.kron(frame, ones)
    assert big.shape[:2] == (960, 1280) and big.dtype == np.uint8
    exps = {}
    for refine in (rn, None):
        small = infer_batch(frame[None], case.n_ids, dc, refine)[0]
        assert small.ndim == 2 and small.shape[0] > 0 and small.shape[1] == 3
        exp = exps[refine is not None] = rz.map_points(small, (960, 1280), (240, 320))
        assert exp.dtype == np.float64 and np.array_equal(exp[:, 2], small[:, 2])
        for m in ("area", "linear", "nearest"):
            got = rz.infer_batch_resized(big[None], (240, 320), case.n_ids, dc, refine, interpolation=m)
            assert len(got) == 1 and got[0].dtype == np.float64 and np.array_equal(got[0], exp), m
    d_big = torch.from_numpy(np.stack([big, big])).to(dev)                   # frames that already lie on the GPU; the default mode
    got = rz.infer_batch_resized(d_big, (240, 320), case.n_ids, dc, rn)
    assert len(got) == 2 and all(np.array_equal(g, exps[True]) for g in got)
