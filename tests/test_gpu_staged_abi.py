"""The staged chain of the C ABI -- dcx_detector_forward -> dcx_detector_decode -> dcx_build_patch_table -> dcx_extract_patches_u8
-> dcx_refiner_forward with a device-side patch count -- stage by stage through raw pointers, as a binding in another language
would call it.  Everything compares by exact equality, on integers or float32 bit patterns, with

  * the oracle's stage functions (pred_argmax, pred_to_keypoints, extract_patches, pre_bgr_image, speedy_bargmax2d, infer_image),
  * tests/staged_exact.py, the numpy restatement of the header's three index contracts (pinned to the oracle on the CPU by
    tests/test_staged_abi_host.py),
  * the library's already pinned entries where an equality of two paths is the claim (dcx_infer_batch; dcx_refiner_forward
    without a limit, test_gpu_exact_chain.py).

Every output buffer is prefilled with a sentinel and lies between two guard regions (tests/guarded.py) that are checked after the
call.  Every table a test passes stays inside the buffers it allocates: no frame index, slot or total is out of range anywhere in
this file.
Counts per case go to staged_abi_report.json in the suite's report directory (beside test_gpu_parity.py's parity_report.json)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, GoldenCase
from deepcharuco_amd import weights as W
from oracle import deepcharuco_oracle as O
from guarded import Guarded
from staged_exact import SENTINEL, decode_rows, gather_u8, patch_table

pytestmark = pytest.mark.gpu

FSENT = -12345.5                 # float sentinel (no kernel here can produce it: |normalised pixel| <= 0.5, xy >= -4)
E_ARG, E_SHAPE, E_NIDS = -1, -2, -4

REPORT = {}


def _report_dir():
    """The suite's report directory: the ignored ``*_out/`` entry of .gitignore, where the other GPU tests write theirs."""
    with open(os.path.join(REPO, ".gitignore")) as f:
        names = [l.strip().rstrip("/") for l in f if l.strip().endswith("_out/")]
    return os.path.join(REPO, names[0] if names else "reports_out")


def _report(key, value):
    REPORT[key] = value
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "staged_abi_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, default=int)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from deepcharuco_amd import _lib
    return _lib.lib()


def _stream():
    from deepcharuco_amd import _lib
    return _lib.current_stream()


def _ibuf(dev, *shape):
    return Guarded(dev, shape, torch.int32, SENTINEL)


def _fbuf(dev, *shape):
    return Guarded(dev, shape, torch.float32, FSENT)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ok(rc, where):
    assert rc == 0, f"{where} returned {rc}"


# --------------------------------------------------------------------------- models and frames of the decode cases

N_IDS = [8, 16, 40]
SHAPES = [(64, 96), (8, 8), (250, 330), (240, 320), (480, 640)]
BATCHES = [1, 3, 9]
REGIMES = ["plain", "negative", "positive", "tied"]
SHIFT = np.float32(16.0)         # the issue's figure: max |logit| of the fixtures is 11.2; asserted on the returned logits


def _case_frames(h, w):
    """Nine frames; frame 0 is flat gray (the calibration below makes it the frame that fires nothing), then noise and boards."""
    flat = np.full((1, h, w), 128, np.uint8)
    return np.concatenate([flat, W.synthetic_frames("noise", 4200 + h, 4, h, w), W.synthetic_frames("board", 4300 + w, 3, h, w),
                           np.full((1, h, w), 255, np.uint8)])


def _base_sd(n_ids):
    """n_ids = 16: the weights of the tiny_noise_64x96 fixture, whose loc head puts the no-corner class 64 on ~20 % of the cells
    of a noise frame (so the loc == 64 rule decides there); 8 and 40: seeded weights."""
    if n_ids == 16:
        return {k: v.copy() for k, v in GoldenCase("tiny_noise_64x96").sd_dc.items()}
    return W.synthetic_state_dict("detector", 4100 + n_ids, n_ids)


def calibrate_frame0(sd, n_ids, loc_logits, ids_logits):
    """Make frame 0 the frame that fires nothing at dust_bin = n_ids and every cell at a dust bin no cell of it carries: move
    convDb.bias[n_ids] so that the dust logit of every cell of frame 0 ends a quarter above its best id logit, and lower
    convPb.bias[64] (only if needed) until the no-corner class ends a quarter below the best corner class in every cell of
    frame 0.  A construction of the INPUT -- the expected values always come from the logits the run itself returns; the
    quarter is there so that the rounding of the shifted biases cannot undo it."""
    out = {k: v.copy() for k, v in sd.items()}
    m = ids_logits[0, :n_ids].max(axis=0) - ids_logits[0, n_ids]
    out["convDb.bias"][n_ids] += np.float32(m.max() + 0.25)
    g = loc_logits[0, 64] - loc_logits[0, :64].max(axis=0)
    if g.max() > -0.25:
        out["convPb.bias"][64] -= np.float32(g.max() + 0.25)
    return out


def regime_sd(sd, n_ids, regime):
    out = {k: v.copy() for k, v in sd.items()}
    if regime == "negative":         # every logit < 0: a kernel that looked at a zero pad channel would pick it
        out["convPb.bias"] -= SHIFT
        out["convDb.bias"] -= SHIFT
    elif regime == "positive":
        out["convPb.bias"] += SHIFT
        out["convDb.bias"] += SHIFT
    elif regime == "tied":           # zero head weights, equal biases: every class of a head ties, the last loc class included
        out["convPb.weight"][:] = 0
        out["convDb.weight"][:] = 0
        out["convPb.bias"][:] = np.float32(-0.75)
        out["convDb.bias"][:] = np.float32(-0.75)
    return out


class DetRunner:
    """dcx_detector_forward on u8 frames into a workspace this object owns (dcx_detector_decode re-reads it)."""

    def __init__(self, L, n_ids, sd, dev):
        from deepcharuco_amd.models.net import dcModel
        self.L, self.dev, self.n_ids = L, dev, n_ids
        self.model = dcModel(n_ids, sd, dev)
        self.ws = None

    @property
    def handle(self):
        return self.model.handle

    def forward(self, frames, want_logits=True):
        b, h, w = frames.shape
        L, dev = self.L, self.dev
        nbytes = L.dcx_detector_workspace_bytes(self.handle, b, h, w)
        assert nbytes > 0
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.frames_d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        hc, wc = h // 8, w // 8
        loc = _fbuf(dev, b, 65, hc, wc) if want_logits else None
        ids = _fbuf(dev, b, self.n_ids + 1, hc, wc) if want_logits else None
        _ok(L.dcx_detector_forward(self.handle, self.frames_d.data_ptr(), h * w, w, None, b, h, w, self.ws.data_ptr(),
                                   self.ws.numel(), loc.ptr if loc else None, ids.ptr if ids else None, _stream()), "dcx_detector_forward")
        if not want_logits:
            return None, None
        torch.cuda.synchronize()
        assert loc.guard_ok() and ids.guard_ok()
        return loc.cpu(), ids.cpu()


_base_logits = {}
_runners = {}


def _runner(L, dev, n_ids, hw, regime):
    """The detector of a (n_ids, shape, regime): the base weights, calibrated on the logits the base model returns for the nine
    frames of the shape, then put into the regime."""
    key = (n_ids, hw, regime)
    if key not in _runners:
        base = _base_sd(n_ids)
        if (n_ids, hw) not in _base_logits:
            r0 = DetRunner(L, n_ids, base, dev)
            _base_logits[(n_ids, hw)] = r0.forward(_case_frames(*hw))
        sd = regime_sd(calibrate_frame0(base, n_ids, *_base_logits[(n_ids, hw)]), n_ids, regime)
        if len(_runners) >= 2:
            _runners.pop(next(iter(_runners)))
        _runners[key] = DetRunner(L, n_ids, sd, dev)
    return _runners[key]


def run_decode(L, dev, det, b, h, w, dust_bin, kmax, maps=True):
    hc, wc = h // 8, w // 8
    counts, rows = _ibuf(dev, b), _ibuf(dev, b, kmax, 4)
    la = _ibuf(dev, b, hc, wc) if maps else None
    ia = _ibuf(dev, b, hc, wc) if maps else None
    _ok(L.dcx_detector_decode(det.handle, b, h, w, det.ws.data_ptr(), dust_bin, kmax, counts.ptr, rows.ptr,
                              la.ptr if maps else None, ia.ptr if maps else None, _stream()), "dcx_detector_decode")
    torch.cuda.synchronize()
    for g in (counts, rows) + ((la, ia) if maps else ()):
        assert g.guard_ok(), "guard region written"
    return counts.cpu(), rows.cpu(), (la.cpu() if maps else None), (ia.cpu() if maps else None)


def pick_dust_bins(n_ids, raw_ids_argmax0):
    """n_ids, and a class below n_ids that wins no cell of frame 0 (3 if it qualifies): with it frame 0 fires every cell that
    the loc == 64 rule leaves."""
    wins = np.bincount(raw_ids_argmax0.reshape(-1), minlength=n_ids + 1)
    free = [c for c in [3] + list(range(n_ids)) if wins[c] == 0]
    assert free, "every id class wins a cell of frame 0"
    return [n_ids, free[0]]


# --------------------------------------------------------------------------- a. decode from the workspace

@pytest.mark.parametrize("batch", BATCHES)             # (the top decorator varies fastest: one detector serves its three batches)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n_ids", N_IDS)
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_decode_from_workspace(dev, L, hw, batch, n_ids, regime):
    """dcx_detector_decode (dcx_cell_argmax_kernel<true> on the C4 logits + dcx_compact_kernel) == torch's arg-max of the NCHW
    logits the same forward returned -- the same bits (test_layout_roundtrip), so every cell must agree, no margin -- and
    decode_rows of those maps, for two dust bins and for kmax at, one below and far above the busiest frame's count.

    The case cannot pass empty: over its decode calls the expected counts hold a frame at 0, a frame that fires every cell, a
    frame equal to kmax and (where the map has more than one cell) a frame above kmax."""
    h, w = hw
    hc, wc = h // 8, w // 8
    cells = hc * wc
    det = _runner(L, dev, n_ids, hw, regime)
    frames = _case_frames(h, w)[:batch]
    loc, ids = det.forward(frames)
    tl, ti = torch.from_numpy(loc), torch.from_numpy(ids)
    lmax, imax = loc.max(axis=1), ids.max(axis=1)
    n_neg = int(((lmax < 0) & (imax < 0)).sum())
    n_pos = int(((loc.min(axis=1) > 0) & (ids.min(axis=1) > 0)).sum())
    if regime == "negative":
        assert n_neg == batch * cells, (float(lmax.max()), float(imax.max()))
    if regime == "positive":
        assert n_pos == batch * cells, (float(loc.min()), float(ids.min()))
    if regime == "tied":
        assert np.all(loc == loc[:, :1]) and np.all(ids == ids[:, :1]) and n_neg == batch * cells
        dust_bins = [n_ids, 0]                  # index 0 wins both heads: everything fires / nothing fires
    else:
        dust_bins = pick_dust_bins(n_ids, ids[0].argmax(axis=0))
    seen = {"zero": 0, "all": 0, "equal": 0, "above": 0, "below": 0}
    rep = {"cells": cells, "all_negative_cells": n_neg, "all_positive_cells": n_pos, "calls": []}
    for dust_bin in dust_bins:
        ela, eia = O.pred_argmax(tl, ti, dust_bin)
        ela, eia = ela.numpy(), eia.numpy()
        if regime == "tied":
            assert not ela.any() and np.all(eia == 0)
        masked = int(((ela == 64) & (ti.argmax(dim=1).numpy() != dust_bin)).sum())
        c_all, _ = decode_rows(ela, eia, dust_bin, cells)
        cmax = int(c_all.max())
        for kmax in sorted({cells, max(1, cmax), max(1, cmax - 1)}):
            ec, er = decode_rows(ela, eia, dust_bin, kmax)
            counts, rows, la, ia = run_decode(L, dev, det, batch, h, w, dust_bin, kmax)
            assert np.array_equal(la, ela), f"loc arg-max differs on {int((la != ela).sum())} cells"
            assert np.array_equal(ia, eia), f"ids arg-max differs on {int((ia != eia).sum())} cells"
            assert np.array_equal(counts, ec), (counts, ec)
            assert np.array_equal(rows, er), "rows (the sentinel beyond min(count, kmax) included)"
            seen["zero"] += int((ec == 0).sum())
            seen["all"] += int((ec == cells).sum())
            seen["equal"] += int((ec == kmax).sum())
            seen["above"] += int((ec > kmax).sum())
            seen["below"] += int((ec < kmax).sum())
            rep["calls"].append({"dust_bin": dust_bin, "kmax": kmax, "counts": ec.tolist(), "masked_by_loc64": masked,
                                 "above": int((ec > kmax).sum()), "at": int((ec == kmax).sum()), "below": int((ec < kmax).sum())})
        if n_ids == 16 and regime != "tied" and batch >= 3 and cells >= 96 and dust_bin != n_ids:
            assert masked > 0, "no cell where the loc == 64 rule hides a firing id"
    rep["frames"] = seen
    _report(f"decode/{h}x{w}/b{batch}/n{n_ids}/{regime}", rep)
    assert seen["zero"] and seen["all"] and seen["equal"], seen
    assert seen["above"] or cells == 1, seen          # one cell: a count cannot exceed kmax >= 1


def test_decode_kmax_sweep_and_patch_table(dev, L):
    """One dense case (250x330: 1271 cells, three frames, the dust bin that lets nearly every cell fire) over kmax = 1 .. cells:
    the counts never change, the rows are the prefix, row storage beyond min(count, kmax) and the guards are untouched;
    dcx_pred_to_keypoints with the same kmax on the NCHW logits obeys the same law; dcx_build_patch_table on these real rows ==
    patch_table."""
    h, w, b, n_ids = 250, 330, 3, 16
    cells = (h // 8) * (w // 8)
    det = _runner(L, dev, n_ids, (h, w), "plain")
    frames = _case_frames(h, w)[:b]
    loc, ids = det.forward(frames)
    dust_bin = pick_dust_bins(n_ids, ids[0].argmax(axis=0))[1]
    ela, eia = (t.numpy() for t in O.pred_argmax(torch.from_numpy(loc), torch.from_numpy(ids), dust_bin))
    c_inf, r_inf = decode_rows(ela, eia, dust_bin, cells)
    assert c_inf.max() == cells and c_inf.min() > 257
    loc_d, ids_d = torch.from_numpy(loc).to(dev), torch.from_numpy(ids).to(dev)
    for kmax in (1, 63, 64, 65, 255, 256, 257, cells - 1, cells):
        ec, er = decode_rows(ela, eia, dust_bin, kmax)
        assert np.array_equal(ec, c_inf) and all(np.array_equal(er[f, :min(c_inf[f], kmax)], r_inf[f, :min(c_inf[f], kmax)]) for f in range(b))
        counts, rows, _, _ = run_decode(L, dev, det, b, h, w, dust_bin, kmax, maps=False)
        assert np.array_equal(counts, c_inf), (kmax, counts, c_inf)
        assert np.array_equal(rows, er), kmax
        # the caller-logits entry with an explicit kmax (its Python wrappers always pass kmax = cells)
        c2, r2, la2, ia2 = _ibuf(dev, b), _ibuf(dev, b, kmax, 4), _ibuf(dev, b, cells), _ibuf(dev, b, cells)
        _ok(L.dcx_pred_to_keypoints(loc_d.data_ptr(), ids_d.data_ptr(), b, 65, n_ids + 1, h // 8, w // 8, dust_bin, kmax,
                                    c2.ptr, r2.ptr, la2.ptr, ia2.ptr, _stream()), "dcx_pred_to_keypoints")
        torch.cuda.synchronize()
        assert all(g.guard_ok() for g in (c2, r2, la2, ia2))
        assert np.array_equal(c2.cpu(), c_inf) and np.array_equal(r2.cpu(), er), kmax
        assert np.array_equal(la2.cpu().reshape(ela.shape), ela) and np.array_equal(ia2.cpu().reshape(eia.shape), eia)
        # the patch table of these rows
        et, en = patch_table(ec, er, kmax)
        table, total = _ibuf(dev, b * kmax, 4), _ibuf(dev, 1)
        rows_d, counts_d = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
        _ok(L.dcx_build_patch_table(counts_d.data_ptr(), rows_d.data_ptr(), b, kmax, table.ptr, total.ptr, _stream()), "dcx_build_patch_table")
        torch.cuda.synchronize()
        assert table.guard_ok() and total.guard_ok()
        assert int(total.cpu()[0]) == en == int(np.minimum(c_inf, kmax).sum())
        assert np.array_equal(table.cpu()[:en], et) and np.all(table.cpu()[en:] == SENTINEL)
    _report("decode/kmax_sweep", {"cells": cells, "counts": c_inf.tolist(), "dust_bin": dust_bin})


def test_decode_refusals_with_real_buffers(dev, L):
    det = _runner(L, dev, 16, (64, 96), "plain")
    det.forward(_case_frames(64, 96)[:1], want_logits=False)
    torch.cuda.synchronize()
    counts, rows = _ibuf(dev, 1), _ibuf(dev, 96, 4)
    call = lambda hh, dust, kmax: L.dcx_detector_decode(det.handle, 1, hh, 96, det.ws.data_ptr(), dust, kmax, counts.ptr, rows.ptr,
                                                        None, None, _stream())
    assert call(64, 256, 96) == E_NIDS and call(64, -1, 96) == E_NIDS
    assert call(64, 16, 0) == E_SHAPE
    assert call(4, 16, 96) == E_SHAPE
    assert L.dcx_detector_decode(det.handle, 1, 64, 96, det.ws.data_ptr(), 16, 96, None, rows.ptr, None, None, _stream()) == E_ARG
    torch.cuda.synchronize()
    assert np.all(counts.cpu() == SENTINEL) and np.all(rows.cpu() == SENTINEL) and counts.guard_ok() and rows.guard_ok()
    assert call(64, 16, 96) == 0                       # and the same buffers are accepted
    torch.cuda.synchronize()
    assert counts.cpu()[0] >= 0


# --------------------------------------------------------------------------- b. patch table

def _table_inputs(batch, kmax, seed):
    """Counts drawn from {0, 1, kmax-1, kmax, kmax+1, 10 kmax}; zeros at the first frame, at the last frame and in a run across
    every 256-frame chunk boundary the batch has."""
    rng = np.random.default_rng([seed, batch, kmax])
    counts = rng.choice(np.array([0, 1, kmax - 1, kmax, kmax + 1, 10 * kmax]), batch).astype(np.int32)
    if batch > 1:
        counts[0] = counts[-1] = 0
        for edge in range(256, batch, 256):
            counts[edge - 3:min(batch, edge + 4)] = 0
        counts[1 % batch] = 10 * kmax
    if batch > 258:
        counts[255], counts[256] = kmax + 1, 0          # a full frame right before an empty one at the chunk boundary ...
        counts[511 % batch], counts[512 % batch] = 0, kmax   # ... and the other way round
    rows = rng.integers(0, 5000, (batch, kmax, 4)).astype(np.int32)
    return counts, rows


@pytest.mark.parametrize("kmax", [1, 7, 64])
@pytest.mark.parametrize("batch", [1, 255, 256, 257, 600])
def test_patch_table(dev, L, batch, kmax):
    """dcx_build_patch_table on caller counts and rows == patch_table: table[:total], total, and table[total:] untouched, for
    batches on both sides of the kernel's 256-frame chunk (the carry between chunks) and counts above kmax."""
    variants = [_table_inputs(batch, kmax, 1)]
    if batch == 1:
        variants = [(np.array([c], np.int32), variants[0][1]) for c in (0, 1, kmax - 1, kmax, kmax + 1, 10 * kmax)]
    else:
        full = _table_inputs(batch, kmax, 2)
        variants.append((np.full(batch, 10 * kmax, np.int32), full[1]))      # every frame capped: total = batch * kmax
        variants.append((np.zeros(batch, np.int32), full[1]))
    rep = []
    for counts, rows in variants:
        et, en = patch_table(counts, rows, kmax)
        assert en <= batch * kmax
        table, total = _ibuf(dev, batch * kmax, 4), _ibuf(dev, 1)
        counts_d, rows_d = torch.from_numpy(counts).to(dev), torch.from_numpy(rows).to(dev)
        _ok(L.dcx_build_patch_table(counts_d.data_ptr(), rows_d.data_ptr(), batch, kmax, table.ptr, total.ptr, _stream()), "dcx_build_patch_table")
        torch.cuda.synchronize()
        assert table.guard_ok() and total.guard_ok()
        assert int(total.cpu()[0]) == en
        got = table.cpu()
        assert np.array_equal(got[:en], et), f"first differing entry {int(np.argmax((got[:en] != et).any(axis=1)))} of {en}"
        assert np.all(got[en:] == SENTINEL)
        rep.append({"total": en, "above": int((counts > kmax).sum()), "at": int((counts == kmax).sum()),
                    "below": int((counts < kmax).sum()), "zero": int((counts == 0).sum())})
    if batch > 1:
        assert rep[0]["above"] and rep[0]["zero"] >= 2 and rep[0]["total"] > 0
    _report(f"table/b{batch}/k{kmax}", rep)


# --------------------------------------------------------------------------- c. gather

def _keypoints(h, w):
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1),                      # corners
           (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2),          # edge mid-points
           (min(11, w - 1), min(11, h - 1)), (min(12, w - 1), min(12, h - 1)),  # last touching / first fully inside
           (w // 2, h // 2), (w // 3, (2 * h) // 3), (max(0, w - 13), max(0, h - 13)), (max(0, w - 12), max(0, h - 12))]
    return np.array(pts, np.int32)


def _window_buffer(dev, frames, pitch, fstride, offset):
    """The frames as windows of one larger byte buffer whose every other byte is 255."""
    b, h, w = frames.shape
    assert pitch > w and fstride > h * pitch
    big = torch.full((offset + b * fstride + 64,), 255, dtype=torch.uint8, device=dev)
    for i in range(b):
        view = big[offset + i * fstride: offset + i * fstride + h * pitch].view(h, pitch)
        view[:, :w] = torch.from_numpy(frames[i]).to(dev)
    return big


@pytest.mark.parametrize("hw", [(64, 96), (8, 8), (9, 15), (40, 56)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_gather_u8_from_windows(dev, L, hw):
    """dcx_extract_patches_u8 (dcx_gather_kernel on gray DcxPix) on three different frames that are windows of a larger buffer (pitch >
    width, frame stride > height * pitch, a byte offset; the padding holds 255) == gather_u8 == the oracle's extract_patches of
    the normalised frame, for key-points on the corners, the edges, around (11, 11) / (12, 12) and inside; patches at and beyond
    *d_total keep the sentinel; dcx_extract_patches_f32 on the normalised images gives the same bits."""
    h, w = hw
    rng = np.random.default_rng([7, h, w])
    frames = rng.integers(0, 255, (3, h, w), dtype=np.uint8)          # 0..254: a padding byte (255) read by mistake shows
    frames[:, 0, 0] = 0
    pitch, fstride, offset = w + 37, (w + 37) * (h + 3) + 11, 17
    big = _window_buffer(dev, frames, pitch, fstride, offset)
    kp = _keypoints(h, w)
    order = rng.permutation(3 * len(kp))                               # the table visits the frames in a mixed order
    table = np.zeros((3 * len(kp), 4), np.int32)
    table[:, 0] = np.repeat(np.arange(3), len(kp))
    table[:, 1:3] = np.tile(kp, (3, 1))
    table = table[order]
    table[:, 3] = np.arange(len(table))
    P = len(table)
    exp = gather_u8(frames, table)
    for f in range(3):                                                 # ... and the oracle itself, per frame
        sel = table[:, 0] == f
        o = O.extract_patches(torch.from_numpy(O.pre_bgr_image(frames[f])), torch.from_numpy(table[sel, 1:3].astype(np.int64))).numpy()
        assert _bits_equal(exp[sel], o)
    assert (exp == 0).any() and (exp != 0).any()
    table_d = torch.from_numpy(table).to(dev)
    for total in (None, 0, 1, P - 1, P):
        patches = _fbuf(dev, P, 24, 24)
        total_d = None if total is None else torch.tensor([total], dtype=torch.int32, device=dev)
        _ok(L.dcx_extract_patches_u8(big.data_ptr() + offset, fstride, pitch, h, w, table_d.data_ptr(),
                                     None if total is None else total_d.data_ptr(), P, patches.ptr, _stream()), "dcx_extract_patches_u8")
        torch.cuda.synchronize()
        assert patches.guard_ok()
        n = P if total is None else total
        got = patches.cpu()
        bad = [int(i) for i in range(n) if not _bits_equal(got[i], exp[i])]
        assert not bad, f"total={total}: patches {bad[:8]} (table rows {table[bad[:8]].tolist()}) differ"
        assert np.all(got[n:] == np.float32(FSENT)), f"total={total}: a patch beyond the total was written"
    # the f32 entry: one dense normalised image block, so each frame's rows go in with frame index 0
    for f in range(3):
        sel = np.flatnonzero(table[:, 0] == f)
        t0 = table[sel].copy()
        t0[:, 0] = 0
        img = torch.from_numpy(O.pre_bgr_image(frames[f])[0]).to(dev).contiguous()
        t0_d = torch.from_numpy(t0).to(dev)
        for total in (None, len(sel) - 1):
            patches = _fbuf(dev, len(sel), 24, 24)
            total_d = None if total is None else torch.tensor([total], dtype=torch.int32, device=dev)
            _ok(L.dcx_extract_patches_f32(img.data_ptr(), h, w, t0_d.data_ptr(), None if total is None else total_d.data_ptr(),
                                          len(sel), patches.ptr, _stream()), "dcx_extract_patches_f32")
            torch.cuda.synchronize()
            n = len(sel) if total is None else total
            assert patches.guard_ok() and _bits_equal(patches.cpu()[:n], exp[sel][:n])
            assert np.all(patches.cpu()[n:] == np.float32(FSENT))
    _report(f"gather/{h}x{w}", {"patches": P, "zero_padded_patches": int((exp == 0).reshape(P, -1).any(axis=1).sum())})


# --------------------------------------------------------------------------- d. limited refine

@pytest.fixture
def mode(request):
    from deepcharuco_amd.inference import set_deterministic
    os.environ.pop("DCX_FORCE_CFG", None)
    try:
        set_deterministic(request.param)
        yield request.param
    finally:
        set_deterministic(False)


@pytest.mark.parametrize("mode", [False, True], ids=["default", "deterministic"], indirect=True)
def test_refiner_forward_with_a_device_limit(dev, L, mode):
    """dcx_refiner_forward on caller patches with *d_total on the device and a table whose slots are frame*kmax + k (what
    dcx_build_patch_table writes): corners[:total] and heat[:total] are bit-identical to an unlimited call on exactly the first
    `total` patches (pinned by test_gpu_exact_chain.py), xy[slot] = (corner - 32) / 8 + (x, y) in float32 at exactly the table's
    slots, everything else keeps its sentinel.  P = 128 patches, totals around the 16-patch work items and odd ones that cut a
    grouped two-map item."""
    from deepcharuco_amd.models.refinenet import RefineNet
    case = GoldenCase("board_240x320")
    rf = RefineNet(case.sd_rn, dev)
    h, w = case.frame.shape
    nf, kmax, P = 5, 40, 128
    counts = np.array([55, 8, 0, 40, 400], np.int32)                     # kept: 40 + 8 + 0 + 40 + 40 = 128
    rng = np.random.default_rng(41)
    rows = np.zeros((nf, kmax, 4), np.int32)
    rows[..., 0], rows[..., 1] = rng.integers(0, w, (nf, kmax)), rng.integers(0, h, (nf, kmax))
    rows[0, :4, :2] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    table, total_all = patch_table(counts, rows, kmax)
    assert total_all == P and table[:, 3].max() == 4 * kmax + kmax - 1 and len(set(table[:, 3].tolist())) == P
    assert not np.array_equal(table[:, 3], np.arange(P))
    patches = gather_u8([case.frame] * nf, table)
    patches_d, table_d = torch.from_numpy(patches).to(dev), torch.from_numpy(table).to(dev)
    ws = torch.empty(L.dcx_refiner_workspace_bytes(rf.handle, P), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    for total in (0, 1, 2, 15, 16, 17, 113, P):
        corners, xy, heat = _ibuf(dev, P, 2), _fbuf(dev, nf * kmax, 2), _fbuf(dev, P, 64, 64)
        total_d = torch.tensor([total], dtype=torch.int32, device=dev)
        ws.fill_(0xA5)
        _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), P, total_d.data_ptr(), table_d.data_ptr(), ws.data_ptr(),
                                  ws.numel(), corners.ptr, xy.ptr, heat.ptr, _stream()), "dcx_refiner_forward (limited)")
        torch.cuda.synchronize()
        assert corners.guard_ok() and xy.guard_ok() and heat.guard_ok()
        # skipped patches are skipped in EVERY layer, the first one included: the call touches no more of its workspace than a
        # call for `total` patches needs (the header's rule; the first layer's output never reaches an output buffer directly)
        touched = int((ws != 0xA5).sum().item())
        assert touched <= L.dcx_refiner_workspace_bytes(rf.handle, total), \
            f"total={total}: {touched} workspace bytes written, {L.dcx_refiner_workspace_bytes(rf.handle, total)} serve {total} patches"
        gc, gxy, gh = corners.cpu(), xy.cpu(), heat.cpu()
        assert np.all(gc[total:] == SENTINEL), f"total={total}: corners beyond the total written"
        untouched_heat = int((gh[total:] != np.float32(FSENT)).sum())
        assert untouched_heat == 0, f"total={total}: {untouched_heat} heat values beyond the total written"
        exy = np.full((nf * kmax, 2), FSENT, np.float32)
        if total:
            c0, h0 = _ibuf(dev, total, 2), _fbuf(dev, total, 64, 64)
            ws0 = torch.empty(L.dcx_refiner_workspace_bytes(rf.handle, total), dtype=torch.uint8, device=dev)
            _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), total, None, None, ws0.data_ptr(), ws0.numel(),
                                      c0.ptr, None, h0.ptr, _stream()), "dcx_refiner_forward (unlimited)")
            torch.cuda.synchronize()
            assert c0.guard_ok() and h0.guard_ok()
            assert _bits_equal(gh[:total], h0.cpu()), f"total={total}: heat differs from the unlimited call"
            assert np.array_equal(gc[:total], c0.cpu()), f"total={total}: corners differ from the unlimited call"
            flat = torch.from_numpy(h0.cpu())
            assert np.array_equal(gc[:total], O.speedy_bargmax2d(flat).numpy())           # = the first flat maximum of that heat
            t = table[:total]
            exy[t[:, 3]] = (gc[:total] - 32).astype(np.float32) / np.float32(8) + t[:, 1:3].astype(np.float32)
        assert _bits_equal(gxy, exy), f"total={total}: xy differs at slots {np.flatnonzero((gxy != exy).any(axis=1))[:8].tolist()}"
    _report(f"refine_limited/{'deterministic' if mode else 'default'}", {"patches": P, "slots": nf * kmax, "counts": counts.tolist()})


# --------------------------------------------------------------------------- e. the whole chain

class Chain:
    """The five staged calls on the current stream into fixed buffers, no host synchronisation between them."""

    def __init__(self, L, dev, det, rf, frames, dust_bin, kmax):
        self.L, self.det, self.rf, self.dust_bin, self.kmax = L, det, rf, dust_bin, kmax
        self.b, self.h, self.w = frames.shape
        b, P = self.b, self.b * kmax
        self.P = P
        self.frames_d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        self.ws_det = torch.empty(L.dcx_detector_workspace_bytes(det.handle, b, self.h, self.w), dtype=torch.uint8, device=dev)
        self.ws_ref = torch.empty(L.dcx_refiner_workspace_bytes(rf.handle, P), dtype=torch.uint8, device=dev)
        self.counts, self.rows = _ibuf(dev, b), _ibuf(dev, b, kmax, 4)
        self.table, self.total = _ibuf(dev, P, 4), _ibuf(dev, 1)
        self.patches, self.corners, self.xy = _fbuf(dev, P, 24, 24), _ibuf(dev, P, 2), _fbuf(dev, P, 2)
        self.outputs = (self.counts, self.rows, self.table, self.total, self.patches, self.corners, self.xy)

    def refill(self):
        for g in self.outputs:
            g.refill()

    def enqueue(self):
        L, s, b, h, w = self.L, _stream(), self.b, self.h, self.w
        _ok(L.dcx_detector_forward(self.det.handle, self.frames_d.data_ptr(), h * w, w, None, b, h, w, self.ws_det.data_ptr(),
                                   self.ws_det.numel(), None, None, s), "dcx_detector_forward")
        _ok(L.dcx_detector_decode(self.det.handle, b, h, w, self.ws_det.data_ptr(), self.dust_bin, self.kmax, self.counts.ptr,
                                  self.rows.ptr, None, None, s), "dcx_detector_decode")
        _ok(L.dcx_build_patch_table(self.counts.ptr, self.rows.ptr, b, self.kmax, self.table.ptr, self.total.ptr, s), "dcx_build_patch_table")
        _ok(L.dcx_extract_patches_u8(self.frames_d.data_ptr(), h * w, w, h, w, self.table.ptr, self.total.ptr, self.P,
                                     self.patches.ptr, s), "dcx_extract_patches_u8")
        _ok(L.dcx_refiner_forward(self.rf.handle, self.patches.ptr, self.P, self.total.ptr, self.table.ptr, self.ws_ref.data_ptr(),
                                  self.ws_ref.numel(), self.corners.ptr, self.xy.ptr, None, s), "dcx_refiner_forward")

    def results(self):
        torch.cuda.synchronize()
        assert all(g.guard_ok() for g in self.outputs), "guard region written"
        return {k: getattr(self, k).cpu().copy() for k in ("counts", "rows", "table", "total", "patches", "corners", "xy")}


def _fused(L, dev, det, rf, frames, dust_bin, pool):
    b, h, w = frames.shape
    ws = torch.empty(L.dcx_pipeline_workspace_bytes(det.handle, rf.handle, b, h, w, pool), dtype=torch.uint8, device=dev)
    frames_d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    counts, starts, rows, xy = _ibuf(dev, b), _ibuf(dev, b), _ibuf(dev, pool, 4), _fbuf(dev, pool, 2)
    _ok(L.dcx_infer_batch(det.handle, rf.handle, frames_d.data_ptr(), h * w, w, 0, b, h, w, dust_bin, pool, ws.data_ptr(), ws.numel(),
                          counts.ptr, starts.ptr, rows.ptr, xy.ptr, None, _stream()), "dcx_infer_batch")
    torch.cuda.synchronize()
    assert all(g.guard_ok() for g in (counts, starts, rows, xy))
    return counts.cpu(), starts.cpu(), rows.cpu(), xy.cpu()


def _oracle_rows(rows, xy):
    """(rows [K][4], xy [K][2] float32) -> what infer_image returns: [x, y, id] float64 sorted by id (stable); np.array([])
    when nothing fires."""
    if rows.shape[0] == 0:
        return np.array([])
    out = np.empty((rows.shape[0], 3), np.float64)
    out[:, :2], out[:, 2] = xy, rows[:, 2]
    return out[np.argsort(rows[:, 2], kind="stable")]


def _chain_case(name):
    """(sd_dc, sd_rn, n_ids, nine frames: the case's own frame first, a frame that fires nothing among them)."""
    if name == "synthetic_250x330":
        h, w = 250, 330
        frames = np.concatenate([W.synthetic_frames("noise", 9100 + h, 5, h, w), W.synthetic_frames("board", 9200 + w, 3, h, w),
                                 np.full((1, h, w), 128, np.uint8)])
        sd = W.synthetic_state_dict("detector", 700 + h + w, 16)
        # dust bias: ~10 corners per frame, set in the middle of a gap of the oracle's margins (as the suite's other seeded
        # detectors are calibrated)
        x = torch.from_numpy(np.stack([O.pre_bgr_image(f) for f in frames]))
        loc, ids = O.detector_forward(O.to_torch_state_dict(sd), x)
        m = ids[:, :16].max(1).values - ids[:, 16]
        m = torch.where(loc.argmax(1) == 64, torch.tensor(-1e30), m).flatten().sort(descending=True).values
        sd["convDb.bias"][16] += np.float32((m[10 * len(frames) - 1] + m[10 * len(frames)]) / 2)
        return sd, W.synthetic_state_dict("refinenet", 701 + h), 16, frames
    c = GoldenCase(name)
    h, w = c.frame.shape
    frames = np.concatenate([c.frame[None], W.synthetic_frames("noise", 6100 + h, 4, h, w), W.synthetic_frames("board", 6200 + h, 2, h, w),
                             np.full((1, h, w), 128, np.uint8), np.full((1, h, w), 255, np.uint8)])
    return c.sd_dc, c.sd_rn, c.n_ids, frames


CHAIN_CASES = ["tiny_noise_64x96", "board_240x320", "diverse_ids_240x320", "synthetic_250x330"]


@pytest.mark.parametrize("regime", ["plain", "negative"])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_staged_chain_equals_fused_path_and_oracle(dev, L, name, regime):
    """The five stages on one stream without a host round trip, batch 9 and batch 1: per frame the rows equal the rows
    dcx_infer_batch puts in its corner pool, xy[frame*kmax + k] equals its xy bit for bit, and both are what the oracle's
    infer_image returns.  In the all-negative regime (every head bias - 16) the fused tail's padded MFMA rows face the pad-channel
    question too; the expectation is still the oracle's on the shifted weights."""
    from deepcharuco_amd.models.refinenet import RefineNet
    sd_dc, sd_rn, n_ids, frames = _chain_case(name)
    sd_dc = regime_sd(sd_dc, n_ids, regime)
    det, rf = DetRunner(L, n_ids, sd_dc, dev), RefineNet(sd_rn, dev)
    t_dc, t_rn = O.to_torch_state_dict(sd_dc), O.to_torch_state_dict(sd_rn)
    kmax = 64
    exp = [O.infer_image(None, n_ids, t_dc, t_rn, gray=f) for f in frames]
    n_exp = [e.shape[0] if e.ndim == 2 else 0 for e in exp]
    assert min(n_exp) == 0 and max(n_exp) >= 4 and max(n_exp) <= kmax, n_exp
    if regime == "negative":
        loc, ids = det.forward(frames)
        assert loc.max() < 0 and ids.max() < 0
    rep = {"oracle_counts": n_exp}
    for sel in (list(range(9)), [0], [int(np.argmin(n_exp))]):
        fr = np.ascontiguousarray(frames[sel])
        b = len(sel)
        chain = Chain(L, dev, det, rf, fr, n_ids, kmax)
        chain.enqueue()
        got = chain.results()
        fc, fs, frows, fxy = _fused(L, dev, det, rf, fr, n_ids, b * kmax)
        assert np.array_equal(got["counts"], fc), (got["counts"], fc)
        assert int(got["total"][0]) == int(fc.sum())
        et, en = patch_table(got["counts"], got["rows"], kmax)
        assert en == int(got["total"][0]) and np.array_equal(got["table"][:en], et) and np.all(got["table"][en:] == SENTINEL)
        assert _bits_equal(got["patches"][:en], gather_u8(fr, et)) and np.all(got["patches"][en:] == np.float32(FSENT))
        live = np.zeros(b * kmax, bool)
        for i, f in enumerate(sel):
            c, s = int(fc[i]), int(fs[i])
            assert c == n_exp[f], (name, f, c, n_exp[f])
            rows_i = got["rows"][i, :c]
            assert np.array_equal(rows_i, frows[s:s + c]), f"frame {f}: rows differ from the fused path's"
            assert np.all(got["rows"][i, c:] == SENTINEL)
            xy_i = got["xy"][i * kmax:i * kmax + c]
            assert _bits_equal(xy_i, fxy[s:s + c]), f"frame {f}: xy differs from the fused path's"
            live[i * kmax:i * kmax + c] = True
            for tag, r in (("staged", _oracle_rows(rows_i, xy_i)), ("fused", _oracle_rows(frows[s:s + c], fxy[s:s + c]))):
                assert r.shape == exp[f].shape and np.array_equal(r, exp[f]), f"frame {f}: {tag} result differs from the oracle's"
        assert np.all(got["xy"][~live] == np.float32(FSENT)), "an xy slot of no live row was written"
        rep[f"b{b}_frames_{sel[0]}"] = {"counts": fc.tolist(), "total": en}
    _report(f"chain/{name}/{regime}", rep)


def test_staged_chain_in_a_captured_graph(dev, L):
    """The five calls recorded into one captured graph (a single serial chain), replayed twice: the outputs equal the eager
    run's.  None of the entries needs K on the host."""
    from deepcharuco_amd.models.refinenet import RefineNet
    sd_dc, sd_rn, n_ids, frames = _chain_case("tiny_noise_64x96")
    det, rf = DetRunner(L, n_ids, sd_dc, dev), RefineNet(sd_rn, dev)
    kmax = 32
    eager = Chain(L, dev, det, rf, frames, n_ids, kmax)
    eager.enqueue()
    want = eager.results()
    assert int(want["total"][0]) > 0 and want["counts"].min() == 0
    chain = Chain(L, dev, det, rf, frames, n_ids, kmax)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        chain.enqueue()                                   # eager warm-up on the capture stream (lazy module loading)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain.enqueue()
    for _ in range(2):
        chain.refill()
        torch.cuda.synchronize()
        graph.replay()
        got = chain.results()
        for k in want:
            assert np.array_equal(got[k].view(np.int32) if got[k].dtype == np.float32 else got[k],
                                  want[k].view(np.int32) if want[k].dtype == np.float32 else want[k]), f"replay differs in {k}"
    del graph


# --------------------------------------------------------------------------- f. non-finite inputs on caller data

NONFINITE = {
    "all_neg_inf": lambda x, n: x.fill(-np.inf),
    "all_pos_inf": lambda x, n: x.fill(np.inf),
    "pos_inf_tied_at_two": lambda x, n: x.__setitem__([n // 3, n - 2], np.inf),
    "neg_inf_but_one": lambda x, n: (x.fill(-np.inf), x.__setitem__(n // 2, -3.0)),
    "nan_at_0": lambda x, n: x.__setitem__(0, np.nan),
    "nan_in_the_middle": lambda x, n: x.__setitem__(n // 2, np.nan),
    "nan_at_two": lambda x, n: x.__setitem__([n // 3, n - 1], np.nan),
    "nan_after_pos_inf": lambda x, n: (x.__setitem__(n // 3, np.inf), x.__setitem__(n // 3 + 1, np.nan)),
    "nan_before_pos_inf": lambda x, n: (x.__setitem__(n // 3, np.nan), x.__setitem__(n // 3 + 1, np.inf)),
    "nan_last": lambda x, n: x.__setitem__(n - 1, np.nan),
}


@pytest.mark.parametrize("kind", list(NONFINITE))
def test_argmax_on_non_finite_input_follows_torch(dev, L, kind):
    """dcx_pred_to_keypoints (pred_argmax) and dcx_argmax2d (speedy_bargmax2d) take caller data and mirror torch.argmax /
    torch.max: +-inf order like numbers, a NaN is the maximum and the first NaN wins.  One cell / one map per pattern position;
    the other cells stay finite."""
    rng = np.random.default_rng(len(kind))
    # pred_to_keypoints: [B=2][C][3][5] logits, the pattern planted in the channel vector of some cells of both heads
    hc, wc, n_ids = 3, 5, 16
    loc = rng.standard_normal((2, 65, hc, wc)).astype(np.float32)
    ids = rng.standard_normal((2, n_ids + 1, hc, wc)).astype(np.float32)
    for (b, cy, cx) in ((0, 0, 0), (0, 1, 3), (1, 2, 4)):
        v = loc[b, :, cy, cx].copy(); NONFINITE[kind](v, 65); loc[b, :, cy, cx] = v
    for (b, cy, cx) in ((0, 0, 1), (0, 1, 3), (1, 2, 0)):
        v = ids[b, :, cy, cx].copy(); NONFINITE[kind](v, n_ids + 1); ids[b, :, cy, cx] = v
    for dust_bin in (n_ids, 3):
        ela, eia = (t.numpy() for t in O.pred_argmax(torch.from_numpy(loc), torch.from_numpy(ids), dust_bin))
        ec, er = decode_rows(ela, eia, dust_bin, hc * wc)
        kp, idf = O.pred_to_keypoints(torch.from_numpy(loc), torch.from_numpy(ids), dust_bin)
        cat = np.concatenate([er[f, :ec[f]] for f in range(2)])
        assert np.array_equal(cat[:, :2], kp.numpy()) and np.array_equal(cat[:, 2], idf.numpy())
        loc_d, ids_d = torch.from_numpy(loc).to(dev), torch.from_numpy(ids).to(dev)
        counts, rows, la, ia = _ibuf(dev, 2), _ibuf(dev, 2, hc * wc, 4), _ibuf(dev, 2, hc, wc), _ibuf(dev, 2, hc, wc)
        _ok(L.dcx_pred_to_keypoints(loc_d.data_ptr(), ids_d.data_ptr(), 2, 65, n_ids + 1, hc, wc, dust_bin, hc * wc, counts.ptr,
                                    rows.ptr, la.ptr, ia.ptr, _stream()), "dcx_pred_to_keypoints")
        torch.cuda.synchronize()
        assert all(g.guard_ok() for g in (counts, rows, la, ia))
        print(f"{kind} dust {dust_bin}: loc arg-max got {la.cpu()[0, 0, 0]} / {la.cpu()[0, 1, 3]} torch {ela[0, 0, 0]} / {ela[0, 1, 3]}")
        assert np.array_equal(la.cpu(), ela), (kind, la.cpu().tolist(), ela.tolist())
        assert np.array_equal(ia.cpu(), eia), (kind, ia.cpu().tolist(), eia.tolist())
        assert np.array_equal(counts.cpu(), ec) and np.array_equal(rows.cpu(), er)
    # argmax2d: maps below, at and above one 256-thread stride, and the RefineNet's 64x64
    for (hh, ww) in ((1, 1), (3, 5), (16, 16), (17, 23), (64, 64)):
        n = hh * ww
        x = rng.standard_normal((4, n)).astype(np.float32)
        if n >= 6 or kind.startswith("all_"):             # (a single element has no room for the other patterns)
            for k in (0, 2, 3):
                v = x[k].copy(); NONFINITE[kind](v, n); x[k] = v
        x = x.reshape(4, hh, ww)
        e = O.speedy_bargmax2d(torch.from_numpy(x)).numpy()
        out = _ibuf(dev, 4, 2)
        x_d = torch.from_numpy(x).to(dev)
        _ok(L.dcx_argmax2d(x_d.data_ptr(), 4, hh, ww, out.ptr, _stream()), "dcx_argmax2d")
        torch.cuda.synchronize()
        assert out.guard_ok()
        assert np.array_equal(out.cpu(), e), (kind, (hh, ww), out.cpu().tolist(), e.tolist())
