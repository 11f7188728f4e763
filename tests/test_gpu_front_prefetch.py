"""GPU: the two-call form of the batch path (dcx_detector_front + dcx_infer_batch_prefetched) and stream.ResidentStream's use of it
(conv1a of batch i+1 on a side stream beside batch i, two prefetch sets alternating by ticket).

Everything compares by exact equality against the one-call path (dcx_infer_batch / infer_batch_device on a workspace of its own).
Which frame comes first in a batch's corner pool is unspecified and may differ from run to run (include/deepcharuco_amd.h), so
two packed buffers are compared as counts[] plus, per frame, the raw words of its pool slots in the order they were written --
every word of the buffers that is defined, without sorting anything.  Frames are 64x96, batches of 3, kmax 64.
"""
import numpy as np
import pytest
import torch

from deepcharuco_amd import weights as W
from deepcharuco_amd import workload as WL
from deepcharuco_amd.corner_pool import views

pytestmark = pytest.mark.gpu

B, H, WD, KMAX = 3, 64, 96, 64
POOL = B * KMAX


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _canon(packed, b, pool, refined, conf=False):
    """counts and, per frame, the words of its slots of rows / xy / conf, as written (raster order).  Also checks that the
    frames' slot ranges tile [0, sum(counts)) -- the part of starts[] that is specified."""
    packed = np.asarray(packed)
    counts, starts, rows, xy, cf = views(packed, b, pool)
    counts = counts.copy()
    assert int(counts.sum()) <= pool
    spans = sorted((int(s), int(c)) for s, c in zip(starts, counts) if c)
    at = 0
    for s, c in spans:
        assert s == at
        at += c
    parts = [rows]
    if refined:
        parts.append(xy.view(np.int32))
    if conf:
        parts.append(cf.view(np.int32))
    return counts, [[p[s:s + c].copy() for p in parts] for s, c in zip(starts, counts)]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for fa, fb in zip(a[1], b[1]) for x, y in zip(fa, fb))


@pytest.fixture(scope="module")
def case(dev):
    """Models and three different batches: A (3 board frames), B (2 frames: n < batch), C (3 frames in which no cell fires), with
    the one-call result of each from a workspace of its own -- computed once, shared, never written."""
    from deepcharuco_amd._lib import lib
    from deepcharuco_amd.inference import infer_batch_device
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    frames = W.synthetic_frames("board", 6200, 5, H, WD)
    d_all = torch.from_numpy(frames).to(dev)
    sd_dc = WL.calibrate_dustbin(W.synthetic_state_dict("detector", 61), d_all, dev, per_frame=12)
    dc, rn = lModel(dcModel(16, sd_dc, dev)), lRefineNet(RefineNet(W.synthetic_state_dict("refinenet", 62), dev))

    def plain(d, pool=POOL, refine=True):
        n = d.shape[0]
        nb = lib().dcx_pipeline_workspace_bytes(dc.model.handle, rn.model.handle if refine else None, n, H, WD, pool)
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        out = infer_batch_device(d, 16, dc, rn if refine else None, ws=ws, pool=pool)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    quiet = None
    for level in (0, 255, 128, 64, 192):          # a flat frame: the first level at which no cell fires
        d = torch.full((B, H, WD), level, dtype=torch.uint8, device=dev)
        if int(plain(d)[:B].sum()) == 0:
            quiet = d
            break
    assert quiet is not None, "no flat frame is silent under these weights"
    batches = {"A": d_all[:3].contiguous(), "B": d_all[3:5].contiguous(), "C": quiet}
    ref = {k: plain(d) for k, d in batches.items()}
    assert ref["A"][:3].sum() > 10 and ref["B"][:2].sum() > 5
    return {"dc": dc, "rn": rn, "batches": batches, "ref": ref, "plain": plain, "frames": frames}


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("refine,conf", [(True, False), (False, False), (True, True)])
def test_front_plus_prefetched_equals_infer_batch(dev, case, bgr, refine, conf):
    """dcx_detector_front + dcx_infer_batch_prefetched on one stream leave the packed buffer dcx_infer_batch leaves."""
    from deepcharuco_amd._lib import lib
    from deepcharuco_amd.inference import PIXEL_FORMATS, infer_batch_device, launch_front, launch_pipeline, packed_len
    dc, rn = case["dc"], case["rn"] if refine else None
    det, ref = dc.model, rn.model if rn else None
    d = case["batches"]["A"]
    if bgr:       # channels that differ by a few levels: the colour conversion inside the load is part of what is compared
        f = case["frames"][:3].astype(np.int16)
        d = torch.from_numpy(np.stack([np.clip(f + 9, 0, 255), f, np.clip(f - 6, 0, 255)], axis=3).astype(np.uint8)).to(dev).contiguous()
    bpp, pix = (3, PIXEL_FORMATS["opencv4"]) if bgr else (1, PIXEL_FORMATS["gray"])
    L = lib()
    ws = torch.empty((L.dcx_pipeline_workspace_bytes(det.handle, ref.handle if ref else None, B, H, WD, POOL),), dtype=torch.uint8, device=dev)
    exp = infer_batch_device(d, 16, dc, rn, ws=ws, pool=POOL, conf=conf).cpu().numpy()
    nb = L.dcx_front_bytes(det.handle, B, H, WD)
    assert nb >= B * 64 * H * WD * 4 + (64 + B) * 4
    front = torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev)         # dirty control words: the front has to clear them
    ws2 = torch.full_like(ws, 0x5A)
    out = torch.full((packed_len(B, POOL, conf),), -7, dtype=torch.int32, device=dev)
    launch_front(det, d.data_ptr(), B, H, WD, bpp, pix, front)
    launch_pipeline(det, ref, d.data_ptr(), B, H, WD, bpp, pix, 16, POOL, ws2, out.data_ptr(), conf, front=front)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert int(exp[:B].sum()) > 0
    assert _same(_canon(got, B, POOL, refine, conf), _canon(exp, B, POOL, refine, conf))
    # a front set one byte short is refused before anything is launched
    rc = L.dcx_detector_front(det.handle, d.data_ptr(), H * WD * bpp, WD * bpp, pix, B, H, WD, front.data_ptr(), nb - 1, None)
    assert rc == -3


def _unpacked(packed, n, pool=POOL):
    from deepcharuco_amd.inference import unpack_results
    return unpack_results(packed, n, pool, True)[0]


def test_resident_stream_alternating_batches_never_see_a_stale_set(dev, case):
    """A B C A C B ... through one ResidentStream (depth 2, one compute stream), 24 submits: every packed result is that batch's
    one-call result.  A stale activation set or stale control words would come back as another batch's corners or counts."""
    from deepcharuco_amd.stream import ResidentStream
    rs = ResidentStream(16, case["dc"], case["rn"], batch=B, height=H, width=WD, kmax=KMAX, depth=2, raw=True)
    assert rs._front is not None and len(rs._front) == 2
    order = list("ABCACB") * 4
    out = list(rs.run(case["batches"][k] for k in order))
    assert [t for t, _ in out] == list(range(24))
    for (_, pk), k in zip(out, order):
        n = case["batches"][k].shape[0]
        assert _same(_canon(pk, n, POOL, True), _canon(case["ref"][k], n, POOL, True)), k
    assert int(out[2][1][:B].sum()) == 0          # C: nothing fired, between two batches that did


def test_pool_overflow_rerun_beside_a_prefetched_successor(dev, case):
    """kmax 2: batch A fires more cells than its pool holds and is run again (plain path) while its successor's front has
    already run; both come back complete and correct."""
    from deepcharuco_amd.stream import ResidentStream
    rs = ResidentStream(16, case["dc"], case["rn"], batch=B, height=H, width=WD, kmax=2, depth=2)
    assert rs._front is not None
    order = list("ACABA")
    with pytest.warns(UserWarning, match="re-running"):
        out = list(rs.run(case["batches"][k] for k in order))
    assert [t for t, _ in out] == list(range(5))
    for (_, res), k in zip(out, order):
        exp = _unpacked(case["ref"][k], case["batches"][k].shape[0])
        assert len(res) == len(exp) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(res, exp)), k


def test_flush_right_after_submit_and_a_second_stream_object(dev, case):
    """flush() straight after a submit whose front may still be in flight hands out every result; a stream object built afterwards
    on the same model pair gives the same."""
    from deepcharuco_amd.stream import ResidentStream
    got = []
    for _ in range(2):
        rs = ResidentStream(16, case["dc"], case["rn"], batch=B, height=H, width=WD, kmax=KMAX, raw=True)
        assert rs.submit(case["batches"]["A"]) is None
        assert rs.submit(case["batches"]["B"]) is None
        got.append(list(rs.flush()))
        assert list(rs.flush()) == []
    for run in got:
        assert [t for t, _ in run] == [0, 1]
        for (_, pk), k in zip(run, "AB"):
            n = case["batches"][k].shape[0]
            assert _same(_canon(pk, n, POOL, True), _canon(case["ref"][k], n, POOL, True))


def test_two_compute_streams_take_the_plain_path(dev, case):
    from deepcharuco_amd.stream import ResidentStream
    rs = ResidentStream(16, case["dc"], case["rn"], batch=B, height=H, width=WD, kmax=KMAX, compute_streams=2, raw=True)
    assert rs._front is None
    _plain_matches(rs, case)


def _plain_matches(rs, case):
    order = list("ABCACB")
    out = list(rs.run(case["batches"][k] for k in order))
    for (_, pk), k in zip(out, order):
        n = case["batches"][k].shape[0]
        assert _same(_canon(pk, n, POOL, True), _canon(case["ref"][k], n, POOL, True)), k


def test_prefetch_can_be_declined_and_large_sets_are_not_taken_by_default(dev, case, monkeypatch):
    """prefetch=False allocates no set; by default a set above PREFETCH_MAX_BYTES is not allocated either, prefetch=True takes it;
    with several compute streams asking for the prefetch is an error."""
    from deepcharuco_amd.stream import ResidentStream
    kw = dict(batch=B, height=H, width=WD, kmax=KMAX, raw=True)
    rs = ResidentStream(16, case["dc"], case["rn"], prefetch=False, **kw)
    assert rs._front is None
    _plain_matches(rs, case)
    monkeypatch.setattr(ResidentStream, "PREFETCH_MAX_BYTES", 1 << 20)        # a 64x96 set of 3 frames is 4.7 MB
    assert ResidentStream(16, case["dc"], case["rn"], **kw)._front is None
    forced = ResidentStream(16, case["dc"], case["rn"], prefetch=True, **kw)
    assert forced._front is not None
    _plain_matches(forced, case)
    with pytest.raises(ValueError):
        ResidentStream(16, case["dc"], case["rn"], compute_streams=2, prefetch=True, **kw)


def test_failed_set_allocation_warns_once_and_runs_the_plain_path(dev, case, monkeypatch):
    """No memory for the two prefetch sets: one warning at construction, no prefetch, the same results."""
    from deepcharuco_amd import stream as S
    nb = S._lib.lib().dcx_front_bytes(case["dc"].model.handle, B, H, WD)
    real = torch.empty

    def empty(*a, **k):
        if k.get("dtype") == torch.uint8 and a and tuple(a[0]) == (nb,):
            raise torch.cuda.OutOfMemoryError("no memory for a prefetch set (simulated)")
        return real(*a, **k)
    monkeypatch.setattr(torch, "empty", empty)
    with pytest.warns(UserWarning, match="prefetch"):
        rs = S.ResidentStream(16, case["dc"], case["rn"], batch=B, height=H, width=WD, kmax=KMAX, raw=True)
    monkeypatch.undo()
    assert rs._front is None
    _plain_matches(rs, case)
