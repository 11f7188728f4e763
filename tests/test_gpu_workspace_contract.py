"""The memory contract of the C ABI, entry by entry: "the contents of a workspace at entry do not matter; the call writes nothing
outside [d_ws, d_ws + *_workspace_bytes()) and its output buffers" (include/deepcharuco_amd.h).

Every workspace, prefetch set and device output of a call lies in an arena of tests/guarded.py: exactly the reported size, a
4 KiB guard on either side, outputs prefilled with a sentinel no kernel can produce.  Each call is made once per workspace
content, mildest first -- zeros; what a previous, different call through the same bytes left; 0x7F bytes (finite and huge: fp32
3.4e38, fp64 1.4e306); 0xFF bytes (fp32 / fp64 NaN, int32 -1, non-zero control words and tickets) -- and the first content that
fails ends the entry's test.  After every call:
  1. every guard of every arena is intact, and so are the bytes of a larger arena behind the part that is the workspace;
  2. the specified results equal, bit for bit, those of the same call on a roomy torch.empty workspace (the suite's habit);
  3. one result is held to the definition the entry's own device-versus-host test uses (its comparison function, imported);
  4. words the header calls unwritten keep their sentinel, words it calls zero are zero;
  5. the call changed some workspace bytes and left some as they were: else the content tested nothing.  The exemptions are
     stated per case (a refiner call for no patch writes nothing; the matcher and the filter rewrite every byte of theirs).
Counts per case go to workspace_contract_report.json in the suite's report directory.

The words some kernel uses as an index, a count or a ticket, and the launch that writes each before any launch reads it (read
from the code; a word that were read first would be a wild index under 0xFF):

  word                                     where                                   written first by                          read by
  ---------------------------------------  --------------------------------------  ----------------------------------------  ----------------
  pool cursor ctrl[0]                      pipe_layout.ctrl / front_layout.ctrl    conv1a of the detector (dcx_zero_words,   tail's atomicAdd;
                                                                                   dcx_first_dev.h: workgroup (0,0,0)        RefineNet's n_limit
                                                                                   clears ctrl_words) --
                                                                                   dcx_detector_front for a prefetch set
  frame tickets ctrl[64 .. 64+B)           the same words                          the same launch                           tail's last-item test
  codes [B][cells] (packed arg-max)        det_layout.codes                        tail kernel's items (agent-scope stores)  tail's last item of
                                                                                   / dcx_cell_argmax_kernel in decode        the frame / compact
  conf_cells [B][cells][2]                 det_layout.conf                         tail kernel's items, with d_conf only     the same last item
  patch table [pool][4] (frame,x,y,slot)   pipe_layout.table                       tail's last item, slots < pool            conv1a of RefineNet
                                                                                                                             and finalize, p <
                                                                                                                             min(cursor, pool)
  part_val / part_idx [P][tiles]           ref_layout.pval / pidx                  RefineNet head kernel, patches < total    finalize, the same
  inlier index list int32 [pool]           behind poses and scores                 select kernel, list[0 .. count) of the    solve() of the same
                                           (dcx_solve_pnp_ransac_workspace_bytes)  frame's own slots                         wave, [0, count)
  scores int32 [B][iterations]             dcx_pnp_ransac.hip / calib_ransac       hypotheses / consensus kernel, every h    select, OK frames
                                                                                   of every OK frame                         only
  head[kOverlap], head[kChanged]           dcx_calib_ransac.hip, dcx_stereo.hip    hipMemsetAsync at entry; changed_sum      host copies
  LmState::code, lg, iters, attempts       Ws<M>::st of dcx_calib_dev.h (both      calib_init_reduce_kernel (dcx_calib.hip)  every later launch,
                                           calibrations), Ws::st of dcx_stereo.hip / the stereo init writer (lm_reset +      lm_run on the host
                                                                                   code) -- before the first kernel that
                                                                                   tests code
  counts' starts' vstat winner changed     RWs of dcx_calib_ransac.hip             select_compact kernel, every view         inner solve, merge
  filtered rows / xy / mask                the same                                keep_rows / exclude_view, a view's slots  inner solve, remask
  pair, count[2B], idx0 / idx1, ident      Ws of dcx_stereo.hip                    init_views (count, idx), ident kernel,    every later launch
                                                                                   pairs kernel
  labels, sizes [B][H][W]                  dcx_speckle.hip                         tile-label launch, every pixel            union / size / rewrite
"""
import ctypes
import json
import os
import time

import numpy as np
import pytest
import torch

import disparity_limit_cases as lc
import pool_cases
import rectify_exact as rx
import stereo_exact as sx
from conftest import GoldenCase
from deepcharuco_amd import _lib, calib, corner_pool, disparity as dp, pnp, rectify as rc, stereo
from deepcharuco_amd import weights as W
from guarded import Arena, Guarded
from oracle import deepcharuco_oracle as O
from staged_exact import SENTINEL, decode_rows, gather_u8, patch_table

pytestmark = pytest.mark.gpu

FSENT = -12345.5                 # float sentinel of the staged tests: |normalised pixel| <= 0.5, xy >= -4, poses and rms are not it
USENT = 0x5B                     # uint8 sentinel: a mask byte is 0 or 1
PATTERNS = (("zeros", b"\x00"), ("leftovers", None), ("0x7f", b"\x7f"), ("0xff", b"\xff"))
I32, F32, F64, U8, I16 = torch.int32, torch.float32, torch.float64, torch.uint8, torch.int16

REPORT = {"seconds": {}}


def _write_report():
    from test_gpu_staged_abi import _report_dir
    out = _report_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "workspace_contract_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, default=int)


def _report(key, value):
    REPORT[key] = value
    _write_report()


@pytest.fixture(autouse=True)
def _timed(request):
    """The wall time of every test of this file, in the report (their sum is the file's)."""
    t0 = time.time()
    yield
    REPORT["seconds"][request.node.name] = round(time.time() - t0, 2)
    REPORT["seconds"]["whole file"] = round(sum(v for k, v in REPORT["seconds"].items() if k != "whole file"), 2)
    _write_report()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _stream():
    return _lib.current_stream()


def _gpu(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)                              # (a copy: the scenes are read-only)


# --------------------------------------------------------------------------- the harness

class Roomy:
    """The suite's habit: a torch.empty tensor with room behind the bytes asked for."""

    def __init__(self, nbytes, dev, align=256, offset=0):
        self.nbytes = nbytes
        self.full = torch.empty(nbytes + 4096 + align, dtype=U8, device=dev)
        self.start = (offset - self.full.data_ptr()) % align
        self.body = self.full[self.start:self.start + nbytes]

    @property
    def ptr(self):
        return self.full.data_ptr() + self.start


class Bufs:
    """The buffers of one call.  guarded: workspaces in exact-size arenas; else roomy torch.empty ones.  The outputs are guarded
    either way.  ``room``: the arena is made large enough for the larger call that leaves its contents behind; the workspace is
    its first ``nbytes`` bytes and the rest is checked like a guard."""

    def __init__(self, dev, guarded):
        self.dev, self.guarded, self.ws, self.need, self.out = dev, guarded, {}, {}, {}

    def workspace(self, name, nbytes, room=0, align=256, offset=0):
        self.need[name] = nbytes
        self.ws[name] = (Arena(max(nbytes, room), self.dev, align=align, offset=offset) if self.guarded
                         else Roomy(nbytes, self.dev, align, offset))
        return self.ws[name]

    def output(self, name, shape, dtype, fill, align=256, offset=0):
        self.out[name] = Guarded(self.dev, shape, dtype, fill, align=align, offset=offset)
        return self.out[name]

    def refill_outputs(self):
        for g in self.out.values():
            g.refill()

    def damage(self):
        every = list(self.out.items()) + (list(self.ws.items()) if self.guarded else [])
        return {n: a.guards_ok() for n, a in every if a.guards_ok() is not None}


def _same(got, want, where):
    assert got.keys() == want.keys(), where
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))
            raise AssertionError(f"{where}: {k} differs in {bad.size} bytes, the first at byte {int(bad[0])}")


def drive(key, dev, setup, left, want=None, same=_same, writes_nothing=(), rewritten=(), after=None, patterns=PATTERNS):
    """``setup(bufs)`` creates the call's buffers in ``bufs`` and returns ``run()``, which makes the call, waits for it and
    returns the specified results as a dict of arrays.  ``left(bufs)`` makes the previous, different call through the same
    workspace bytes.  ``patterns``: (name, fill) with fill a byte pattern, None (the leftovers) or a dict per workspace.
    ``writes_nothing`` / ``rewritten``: workspaces exempt from the first / second half of rule 5, by the caller's stated reason.
    ``after(bufs, got)``: the entry's own checks (untouched words), -> notes for the report.  -> (want, report)."""
    if want is None:
        want = setup(Bufs(dev, False))()
    g = Bufs(dev, True)
    run = setup(g)
    rep = {}
    for name, fill in patterns:
        where = f"{key}, workspace content {name}"
        if fill is None:
            left(g)
            torch.cuda.synchronize()
        else:
            for n, a in g.ws.items():
                a.fill_body(fill[n] if isinstance(fill, dict) else fill)
        g.refill_outputs()
        snaps = {n: a.body.clone() for n, a in g.ws.items()}
        got = run()
        torch.cuda.synchronize()
        assert not g.damage(), f"{where}: guard damaged at offset (relative to the buffer) {g.damage()}"
        rep[name] = {}
        for n, a in g.ws.items():
            need = g.need[n]
            diff = a.body != snaps[n]
            past = torch.nonzero(diff[need:])
            assert past.numel() == 0, f"{where}: {n} written at byte {need + int(past[0, 0]) if past.numel() else 0} of {need}"
            changed = int(diff[:need].sum())
            rep[name][n] = {"bytes": need, "changed": changed, "kept": need - changed}
            assert changed > 0 or n in writes_nothing, f"{where}: the call changed nothing of {n}"
            assert need - changed > 0 or n in rewritten, f"{where}: nothing of {n} kept its content"
        same(got, want, where)
        if after is not None:
            rep[name]["notes"] = after(g, got)
    _report(key, rep)
    return want, rep


# --------------------------------------------------------------------------- the pipeline: dcx_infer_batch (+ the prefetched form)

def _pool_frames(o, b, pool):
    """The pool restricted to counts / starts: counts and, per frame, the words of its slots below ``pool``."""
    counts, starts = o["counts"], o["starts"]
    out = {"counts": counts.copy()}
    for i in range(b):
        s = min(int(starts[i]), pool)
        e = min(s + int(counts[i]), pool)
        for k in ("rows", "xy", "conf"):
            if k in o:
                out[f"{k}[{i}]"] = np.ascontiguousarray(o[k][s:e]).view(np.int32)
    return out


def _pool_same(got, full, where):
    """``got`` against the whole pool of the roomy call: the counts, and every frame's slots below the pool as the prefix of that
    frame's slots there (which frame a short pool cuts is unspecified; what a frame's slots hold is not)."""
    assert np.array_equal(got["counts"], full["counts"]), (where, got["counts"], full["counts"])
    for k in got:
        if k != "counts":
            n = len(got[k])
            assert n <= len(full[k]) and np.array_equal(got[k], full[k][:n]), f"{where}: {k} differs"


class PipeCase:
    """Models, frames and the oracle's answer of one (shape, batch, n_ids)."""

    def __init__(self, dev, L, h, w, b, n_ids):
        from deepcharuco_amd.models.net import dcModel
        from deepcharuco_amd.models.refinenet import RefineNet
        from test_gpu_parity import _calibrated
        self.h, self.w, self.b, self.n_ids = h, w, b, n_ids
        frames = np.concatenate([W.synthetic_frames("noise", 9100 + h, 5, h, w), W.synthetic_frames("board", 9200 + w, 4, h, w)])
        cells = (h // 8) * (w // 8)
        self.sd_dc = _calibrated(700 + h + w + n_ids - 16, frames, n_ids=n_ids, target_per_frame=max(1, min(10, cells // 3)))
        self.sd_rn = W.synthetic_state_dict("refinenet", 701 + h)
        self.det, self.rf = dcModel(n_ids, self.sd_dc, dev), RefineNet(self.sd_rn, dev)
        # the b frames that fire most (the device's own counts; the oracle below is the judge of them)
        counts = self._counts(dev, L, _gpu(dev, frames))
        pick = np.sort(np.argsort(-counts, kind="stable")[:b])
        self.frames = np.ascontiguousarray(frames[pick])
        self.frames_d = _gpu(dev, self.frames)
        t_dc, t_rn = O.to_torch_state_dict(self.sd_dc), O.to_torch_state_dict(self.sd_rn)
        self.exp = [O.infer_image(None, n_ids, t_dc, t_rn, gray=f) for f in self.frames]
        self.total = sum(e.shape[0] if e.ndim == 2 else 0 for e in self.exp)

    def _counts(self, dev, L, frames_d):
        n = frames_d.shape[0]
        ws = torch.empty(L.dcx_pipeline_workspace_bytes(self.det.handle, None, n, self.h, self.w, 1), dtype=U8, device=dev)
        c, s, r = (torch.zeros(k, dtype=I32, device=dev) for k in (n, n, 4))
        assert L.dcx_infer_batch(self.det.handle, None, frames_d.data_ptr(), self.h * self.w, self.w, 0, n, self.h, self.w, self.n_ids, 1,
                                 ws.data_ptr(), ws.numel(), c.data_ptr(), s.data_ptr(), r.data_ptr(), None, None, _stream()) == 0
        torch.cuda.synchronize()
        return c.cpu().numpy()

    def need(self, L, rf, pool):
        return L.dcx_pipeline_workspace_bytes(self.det.handle, self.rf.handle if rf else None, self.b, self.h, self.w, pool)

    def setup(self, L, rf, conf, pool, room=0, front=False, front_room=0):
        """-> setup(bufs) for drive(): dcx_infer_batch, or with ``front`` dcx_detector_front + dcx_infer_batch_prefetched."""
        b, h, w = self.b, self.h, self.w
        need = self.need(L, rf, pool)
        rfh = self.rf.handle if rf else None
        fneed = L.dcx_front_bytes(self.det.handle, b, h, w)
        assert need > 0 and fneed >= b * 64 * h * w * 4 + (64 + b) * 4

        def setup(bufs):
            ws = bufs.workspace("ws", need, room)
            fs = bufs.workspace("front", fneed, front_room) if front else None
            o = {"counts": bufs.output("counts", (b,), I32, SENTINEL), "starts": bufs.output("starts", (b,), I32, SENTINEL),
                 "rows": bufs.output("rows", (pool, 4), I32, SENTINEL)}
            if rf:
                o["xy"] = bufs.output("xy", (pool, 2), F32, FSENT)
            if conf:
                o["conf"] = bufs.output("conf", (pool, 2), F32, FSENT)
            head = (self.frames_d.data_ptr(), h * w, w, 0, b, h, w)
            tail = (o["counts"].ptr, o["starts"].ptr, o["rows"].ptr, o["xy"].ptr if rf else None, o["conf"].ptr if conf else None)

            def run():
                if front:
                    assert L.dcx_detector_front(self.det.handle, *head, fs.ptr, fneed, _stream()) == 0
                    torch.cuda.synchronize()
                    act = fs.body[:b * 64 * h * w * 4].clone()
                    assert L.dcx_infer_batch_prefetched(self.det.handle, rfh, *head, self.n_ids, pool, ws.ptr, need, fs.ptr, fneed,
                                                        *tail, None, _stream()) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(fs.body[:b * 64 * h * w * 4], act), "the prefetched call wrote the set's activations"
                else:
                    assert L.dcx_infer_batch(self.det.handle, rfh, *head, self.n_ids, pool, ws.ptr, need, *tail, _stream()) == 0
                    torch.cuda.synchronize()
                return _pool_frames({k: g.cpu() for k, g in o.items()}, b, pool)
            return run
        return setup

    def leftovers(self, L, other, rf, pool=64, front=False):
        """-> left(bufs): ``other``'s call (another shape and batch) through the first bytes of the same arenas."""
        need = other.need(L, rf, pool)
        fneed = L.dcx_front_bytes(other.det.handle, other.b, other.h, other.w)

        def left(bufs):
            assert need <= bufs.ws["ws"].nbytes and (not front or fneed <= bufs.ws["front"].nbytes)
            n = corner_pool.packed_len(other.b, pool, True)
            out = torch.zeros(n, dtype=I32, device=bufs.dev)
            p = corner_pool.ptrs(out.data_ptr(), other.b, pool)
            head = (other.frames_d.data_ptr(), other.h * other.w, other.w, 0, other.b, other.h, other.w)
            rfh = other.rf.handle if rf else None
            if front:
                assert L.dcx_detector_front(other.det.handle, *head, bufs.ws["front"].ptr, fneed, _stream()) == 0
                assert L.dcx_infer_batch_prefetched(other.det.handle, rfh, *head, other.n_ids, pool, bufs.ws["ws"].ptr, need,
                                                    bufs.ws["front"].ptr, fneed, *p[:3], p[3] if rf else None, None, None, _stream()) == 0
            else:
                assert L.dcx_infer_batch(other.det.handle, rfh, *head, other.n_ids, pool, bufs.ws["ws"].ptr, need, *p[:3],
                                         p[3] if rf else None, None, _stream()) == 0
            torch.cuda.synchronize()
            assert int(out[:other.b].sum()) > 0, "the call that leaves its contents behind found nothing"
        return left, need, fneed


_pipe_cases = {}


def _pipe_case(dev, L, h, w, b, n_ids=16):
    key = (h, w, b, n_ids)
    if key not in _pipe_cases:
        _pipe_cases[key] = PipeCase(dev, L, h, w, b, n_ids)
    return _pipe_cases[key]


@pytest.fixture
def direct_mode():
    """-> set(enabled); the default family is restored afterwards."""
    from deepcharuco_amd.inference import set_deterministic
    os.environ.pop("DCX_FORCE_CFG", None)
    try:
        yield set_deterministic
    finally:
        set_deterministic(False)


def _oracle_agrees(case, full, where):
    from test_gpu_staged_abi import _oracle_rows
    for i, e in enumerate(case.exp):
        r = _oracle_rows(full[f"rows[{i}]"], full[f"xy[{i}]"].view(np.float32))
        assert r.shape == e.shape and np.array_equal(r, e), f"{where}: frame {i} differs from the oracle"


PIPE_SHAPES = [(64, 96, 3, 16), (64, 96, 1, 16), (67, 101, 2, 16), (9, 15, 1, 16), (250, 330, 1, 16), (64, 96, 2, 40)]


@pytest.mark.parametrize("h,w,b,n_ids", PIPE_SHAPES, ids=[f"{h}x{w}-b{b}-n{n}" for h, w, b, n in PIPE_SHAPES])
def test_infer_batch(dev, L, direct_mode, h, w, b, n_ids):
    """dcx_infer_batch with and without RefineNet, with and without d_conf, in the default and the direct kernel family, at pools
    of exactly sum(counts), one more and one fewer.  In the short pool the counts stay true, a frame's slots below the pool are
    the prefix of its slots in the whole pool, and nothing is stored at or behind slot ``pool`` of rows / xy / conf.  The contents
    left behind are those of the 64x96 batch of three (of the 67x101 batch of two for that batch itself): a larger batch and then
    a smaller one of the same shape, and another shape, through the same bytes."""
    case = _pipe_case(dev, L, h, w, b, n_ids)
    other = _pipe_case(dev, L, 67, 101, 2) if (h, w, b, n_ids) == (64, 96, 3, 16) else _pipe_case(dev, L, 64, 96, 3)
    S = case.total
    assert S >= 1, "no cell fires"
    for direct in (False, True):
        direct_mode(direct)
        for rf in (True, False):
            for conf in (False, True):
                tag = f"infer_batch/{h}x{w}/b{b}/n{n_ids}/{'direct' if direct else 'default'}/{'refine' if rf else 'detect'}{'+conf' if conf else ''}"
                full = case.setup(L, rf, conf, S)(Bufs(dev, False))()           # the roomy call on the whole pool
                assert int(full["counts"].sum()) == S and all(len(full[f"rows[{i}]"]) == full["counts"][i] for i in range(b)), tag
                if rf and not direct:
                    _oracle_agrees(case, full, tag)
                left, lneed, _ = case.leftovers(L, other, rf)
                for pool in sorted({S, S + 1, max(1, S - 1)}):
                    def after(g, got, pool=pool):
                        free = slice(min(S, pool), pool)                          # the header is silent about these slots
                        kept = {k: bool(g.out[k].untouched(free, torch.int64)) for k in ("xy", "conf") if k in g.out}
                        kept["rows"] = bool((g.out["rows"].t[free] == SENTINEL).all())
                        return {"slots_between_sum_counts_and_pool": pool - min(S, pool), "of_them_untouched": kept}
                    drive(f"{tag}/pool{pool}", dev, case.setup(L, rf, conf, pool, room=lneed), left, want=full, same=_pool_same, after=after)


def test_infer_batch_prefetched(dev, L):
    """dcx_detector_front + dcx_infer_batch_prefetched at 64x96, B = 3: the prefetch set in an arena of exactly dcx_front_bytes,
    the four contents on the set and on the workspace independently (sixteen pairs; the leftovers of a set are those of another
    batch's front), and the set's activation part is the same bytes after the prefetched call as before it."""
    case, other = _pipe_case(dev, L, 64, 96, 3), _pipe_case(dev, L, 67, 101, 2)
    S = case.total
    full = case.setup(L, True, True, S)(Bufs(dev, False))()
    _oracle_agrees(case, full, "prefetched")
    left, lneed, lfneed = case.leftovers(L, other, True, front=True)
    fills = dict(PATTERNS)
    # independent contents: a pattern on one and the leftovers on the other are made by filling after the other call has run
    for pf, pw in [(a, c) for a, _ in PATTERNS for c, _ in PATTERNS]:
        def left_then_fill(bufs, pf=pf, pw=pw):
            left(bufs)
            if fills[pf] is not None:
                bufs.ws["front"].fill_body(fills[pf])
            if fills[pw] is not None:
                bufs.ws["ws"].fill_body(fills[pw])
        pattern = (f"front {pf}, ws {pw}", None if None in (fills[pf], fills[pw]) else {"front": fills[pf], "ws": fills[pw]})
        drive(f"infer_batch_prefetched/64x96/b3/front_{pf}/ws_{pw}", dev,
              case.setup(L, True, True, S, room=lneed, front=True, front_room=lfneed), left_then_fill, want=full, same=_pool_same,
              patterns=(pattern,))


# --------------------------------------------------------------------------- dcx_detector_forward -> dcx_detector_decode

@pytest.mark.parametrize("h,w,b", [(64, 96, 3), (9, 15, 1)], ids=["64x96-b3", "9x15-b1"])
def test_detector_forward_and_decode(dev, L, h, w, b):
    """Raw calls, as a binding makes them: the NCHW logits and the decode outputs are the same bits whatever the workspace held,
    and the decode is torch's arg-max of those logits (the staged tests' definition).  The C4 logit buffers carry pad channels
    (68 for 65, ids_quads * 4 for n_ids + 1) that the head kernels do not own; under 0xFF they hold NaN, which an arg-max that
    looked at them would prefer."""
    case = _pipe_case(dev, L, h, w, b)
    other = _pipe_case(dev, L, 67, 101, 2) if b == 3 else _pipe_case(dev, L, 64, 96, 3)
    hc, wc, n1 = h // 8, w // 8, case.n_ids + 1
    cells = hc * wc
    need = L.dcx_detector_workspace_bytes(case.det.handle, b, h, w)
    lneed = L.dcx_detector_workspace_bytes(other.det.handle, other.b, other.h, other.w)

    def setup(bufs):
        ws = bufs.workspace("ws", need, lneed)
        o = {"loc": bufs.output("loc", (b, 65, hc, wc), F32, FSENT), "ids": bufs.output("ids", (b, n1, hc, wc), F32, FSENT),
             "counts": bufs.output("counts", (b,), I32, SENTINEL), "rows": bufs.output("rows", (b, cells, 4), I32, SENTINEL),
             "loc_argmax": bufs.output("loc_argmax", (b, hc, wc), I32, SENTINEL),
             "ids_argmax": bufs.output("ids_argmax", (b, hc, wc), I32, SENTINEL)}

        def run():
            assert L.dcx_detector_forward(case.det.handle, case.frames_d.data_ptr(), h * w, w, None, b, h, w, ws.ptr, need,
                                          o["loc"].ptr, o["ids"].ptr, _stream()) == 0
            assert L.dcx_detector_decode(case.det.handle, b, h, w, ws.ptr, case.n_ids, cells, o["counts"].ptr, o["rows"].ptr,
                                         o["loc_argmax"].ptr, o["ids_argmax"].ptr, _stream()) == 0
            torch.cuda.synchronize()
            return {k: g.cpu().copy() for k, g in o.items()}
        return run

    def left(bufs):
        assert L.dcx_detector_forward(other.det.handle, other.frames_d.data_ptr(), other.h * other.w, other.w, None, other.b, other.h,
                                      other.w, bufs.ws["ws"].ptr, lneed, None, None, _stream()) == 0

    want, _ = drive(f"detector_forward+decode/{h}x{w}/b{b}", dev, setup, left)
    ela, eia = (t.numpy() for t in O.pred_argmax(torch.from_numpy(want["loc"]), torch.from_numpy(want["ids"]), case.n_ids))
    ec, er = decode_rows(ela, eia, case.n_ids, cells)
    assert np.array_equal(want["loc_argmax"], ela) and np.array_equal(want["ids_argmax"], eia)
    assert np.array_equal(want["counts"], ec) and np.array_equal(want["rows"], er) and ec.sum() > 0


# --------------------------------------------------------------------------- dcx_refiner_forward with a device-side limit

REFINE_P, REFINE_KMAX, REFINE_COUNTS = 33, 16, (16, 1, 40)          # kept: 16 + 1 + 16 = 33 of 48 slots


@pytest.mark.parametrize("total", [0, 1, 17, 32, 33])
def test_refiner_forward_limited(dev, L, total):
    """The staged test's limited call at P = 33 patches: the odd totals cut a two-map item, and an exact-size workspace lies
    between guards.  corners[:total] and heat[:total] are the same bits whatever the workspace held, corners are the first flat
    maximum of that heat and xy the staged test's formula at the table's slots; everything else keeps its sentinel.
    Exemptions from rule 5, by the header: a call for total = 0 writes none of its workspace; at total = P the layers rewrite
    their buffers wholly."""
    from deepcharuco_amd.models.refinenet import RefineNet
    case = GoldenCase("board_240x320")
    rf = RefineNet(case.sd_rn, dev)
    h, w = case.frame.shape
    nf, kmax, P = len(REFINE_COUNTS), REFINE_KMAX, REFINE_P
    rng = np.random.default_rng(43)
    rows = np.zeros((nf, kmax, 4), np.int32)
    rows[..., 0], rows[..., 1] = rng.integers(0, w, (nf, kmax)), rng.integers(0, h, (nf, kmax))
    rows[0, :4, :2] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    table, n_all = patch_table(np.array(REFINE_COUNTS, np.int32), rows, kmax)
    assert n_all == P and len(set(table[:, 3].tolist())) == P and table[:, 3].max() == nf * kmax - 1
    patches = gather_u8([case.frame] * nf, table)
    patches_d, table_d = _gpu(dev, patches), _gpu(dev, table)
    other_d = _gpu(dev, patches[::-1] * np.float32(0.5))
    total_d = torch.tensor([total], dtype=I32, device=dev)
    need = L.dcx_refiner_workspace_bytes(rf.handle, P)
    live = np.zeros(nf * kmax, bool)
    live[table[:total, 3]] = True

    def setup(bufs):
        ws = bufs.workspace("ws", need)
        corners, xy, heat = (bufs.output("corners", (P, 2), I32, SENTINEL), bufs.output("xy", (nf * kmax, 2), F32, FSENT),
                             bufs.output("heat", (P, 64, 64), F32, FSENT))

        def run():
            assert L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), P, total_d.data_ptr(), table_d.data_ptr(), ws.ptr, need,
                                         corners.ptr, xy.ptr, heat.ptr, _stream()) == 0
            torch.cuda.synchronize()
            return {"corners": corners.cpu()[:total].copy(), "heat": heat.cpu()[:total].copy(), "xy": xy.cpu()[live].copy()}
        return run

    def left(bufs):                                   # an unlimited call on other patches through the same bytes
        assert L.dcx_refiner_forward(rf.handle, other_d.data_ptr(), P, None, None, bufs.ws["ws"].ptr, need, None, None, None, _stream()) == 0

    def after(g, got):
        assert g.out["corners"].untouched(slice(total, None), torch.int64), "corners beyond the total written"
        assert g.out["heat"].untouched(slice(total * 4096, None), F32), "heat beyond the total written"
        assert g.out["xy"].untouched(~live, torch.int64), "an xy slot of no live table row written"
        return {"xy_slots_untouched": int((~live).sum())}

    want, _ = drive(f"refiner_forward/P{P}/total{total}", dev, setup, left, after=after,
                    writes_nothing=("ws",) if total == 0 else (), rewritten=("ws",) if total == P else ())
    if total:
        assert np.array_equal(want["corners"], O.speedy_bargmax2d(torch.from_numpy(want["heat"])).numpy())
        t = table[:total]
        exy = np.full((nf * kmax, 2), FSENT, np.float32)
        exy[t[:, 3]] = (want["corners"] - 32).astype(np.float32) / np.float32(8) + t[:, 1:3].astype(np.float32)
        assert np.array_equal(want["xy"].view(np.uint32), exy[live].view(np.uint32))


# --------------------------------------------------------------------------- dcx_solve_pnp_ransac_pool

PNP_BOARD = (20, 20, 0.002)


def ransac_frames(seed=77):
    """Six frames of test_gpu_pnp_ransac's hand-built pool, one per status -> (frames, expected status at 100 iterations)."""
    from test_gpu_pnp import _board_frame
    rng = np.random.default_rng(seed)
    frames = [
        _board_frame(rng, np.arange(16) * 7, PNP_BOARD, 0.0),                  # 0: OK
        _board_frame(rng, np.array([3, 50, 200]), PNP_BOARD, 0.0),             # 1: TOO_FEW
        _board_frame(rng, np.arange(10) * 13, PNP_BOARD, 0.0),                 # 2: TRUNCATED (last in the pool, cut)
        _board_frame(rng, np.arange(12) * 5, PNP_BOARD, 0.3),                  # 3: BAD_ID (one id = 361)
        _board_frame(rng, np.arange(19) * 19, PNP_BOARD, 0.0),                 # 4: DEGENERATE (a column of the board: no sample)
        _board_frame(rng, np.arange(12) * 23, PNP_BOARD, 0.0),                 # 5: NO_CONSENSUS (every corner moved by many px)
    ]
    frames[3][4, 2] = 361
    frames[5][:, :2] += rng.uniform(-40, 40, size=(12, 2)).astype(np.float32)
    return frames, [pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_TRUNCATED, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE, pnp.PNP_NO_CONSENSUS]


def ransac_pool(frames, order, gap):
    pool = sum(len(f) for f in frames) + gap * (len(frames) - 1) - 3          # the last frame in the pool is cut by three rows
    return pool_cases.lay_frames(frames, pool, order, gap=gap, cell=-7) + (pool,)


@pytest.mark.parametrize("iterations", [1, 63, 64, 65, 100])
def test_solve_pnp_ransac_pool(dev, L, iterations):
    """A pool of six frames with gaps between their slot ranges, one frame per status; the workspace 8-byte but not 16-byte
    aligned and exactly dcx_solve_pnp_ransac_workspace_bytes; d_inliers NULL and guarded.  Slots of no frame keep the mask's
    sentinel, d_pose is zeros unless OK, and at 100 iterations the frames are test_gpu_pnp_ransac's _check_frame away from
    solve_pnp_ransac_host_full."""
    from test_gpu_pnp_ransac import _check_frame
    from test_pnp_host import DIST5, K
    frames, expect = ransac_frames()
    B = len(frames)
    packed, owned, pool = ransac_pool(frames, [5, 0, 4, 1, 3, 2], 3)
    other, _, pool2 = ransac_pool(frames[::-1], [3, 1, 5, 0, 2, 4], 3)        # other scenes at the frames' places, the same sizes
    assert pool2 == pool and (~owned).sum() >= 15
    kw = dict(reproj_error=8.0, min_inliers=6, seed=1234)
    cam, dist, n_dist = pnp._camera_args(K, DIST5)
    need = L.dcx_solve_pnp_ransac_workspace_bytes(B, pool, iterations)
    d, d2 = _gpu(dev, packed), _gpu(dev, other)

    def call(p, ws_ptr, st, pose, info, inl, seed):
        assert L.dcx_solve_pnp_ransac_pool(*corner_pool.ptrs(p.data_ptr(), B, pool)[:4], B, pool, *PNP_BOARD, cam, dist, n_dist, iterations,
                                           kw["reproj_error"], kw["min_inliers"], seed, ws_ptr, need, st, pose, info, inl, _stream()) == 0

    for with_mask in (False, True):
        def setup(bufs):
            ws = bufs.workspace("ws", need, align=16, offset=8)
            assert ws.ptr % 16 == 8
            o = {"status": bufs.output("status", (B,), I32, SENTINEL), "pose": bufs.output("pose", (B, 8), F64, FSENT),
                 "info": bufs.output("info", (B, 2), I32, SENTINEL)}
            if with_mask:
                o["inliers"] = bufs.output("inliers", (pool,), U8, USENT)

            def run():
                call(d, ws.ptr, o["status"].ptr, o["pose"].ptr, o["info"].ptr, o["inliers"].ptr if with_mask else None, kw["seed"])
                torch.cuda.synchronize()
                got = {k: g.cpu().copy() for k, g in o.items()}
                if with_mask:
                    got["inliers"] = got["inliers"][owned]
                return got
            return run

        def left(bufs):
            tmp = torch.zeros(B * 11 + pool, dtype=F64, device=bufs.dev)      # outputs of its own
            call(d2, bufs.ws["ws"].ptr, tmp.data_ptr(), tmp[B:].data_ptr(), tmp[9 * B:].data_ptr(), None, kw["seed"] + 1)

        def after(g, got):
            if with_mask:
                assert g.out["inliers"].untouched(~owned), "a mask slot of no frame written"
            ok = got["status"] == pnp.PNP_OK
            assert not got["pose"][~ok].any(), "d_pose of a frame without a pose is not zeros"
            return {"status": got["status"].tolist(), "mask_slots_of_no_frame": int((~owned).sum())}

        want, _ = drive(f"solve_pnp_ransac_pool/it{iterations}/{'mask' if with_mask else 'no_mask'}", dev, setup, left, after=after)
    if iterations == 100:
        assert want["status"].tolist() == expect
        mask = np.zeros(pool, np.uint8)
        mask[owned] = want["inliers"]
        tally = [0, 0, 0]
        for b in (0, 5):
            s0, n = int(packed[B + b]), int(packed[b])
            _check_frame((int(want["status"][b]), want["pose"][b], mask[s0:s0 + n].astype(bool), int(want["info"][b, 1])), frames[b],
                         PNP_BOARD, K, DIST5, dict(kw, iterations=100), tally, f"frame {b}", pool_order=True)


# --------------------------------------------------------------------------- the three calibrations

def calib_views(seed, n_ok, sigma=0.0):
    """n_ok views that stand, then three that fail three different checks: three rows, an id outside the board, and a view that
    goes last into the pool and is cut by its end."""
    from test_calib_host import make_views
    _, imgs, ids_l, _ = make_views(seed, n_ok + 1, sigma=sigma)
    kps = [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]
    bad = kps[1].copy()
    bad[1, 2] = 49
    views = kps[:n_ok] + [kps[0][:3].copy(), bad, kps[n_ok].copy()]
    return views, [pnp.PNP_OK] * n_ok + [pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_TRUNCATED]


def calib_pool(views, seed, gap=3, cut=4):
    B = len(views)
    order = list(np.random.default_rng(seed).permutation(B - 1)) + [B - 1]
    pool = sum(len(v) + gap for v in views) - gap - cut
    return pool_cases.lay_frames(views, pool, order, gap=gap, filler=-9) + (pool,)


def _calib_result(res, st, pose):
    return calib.CalibResult(*calib._common_fields(res, st, pose))


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned_by_4"])
def test_calibrate_pool(dev, L, misaligned):
    """dcx_calibrate_pool, raw: eight views of which three fail three different checks, so every reduction runs over views that
    wrote nothing; the contents left behind are those of a 16-view call on other scenes.  Also at a workspace address that is 4
    modulo 8, which the entry accepts."""
    from test_calib_host import BOARD, SIZE
    from test_gpu_calib import _check
    views, expect = calib_views(7, 5)
    packed, owned, pool = calib_pool(views, 7)
    B = len(views)
    big, _ = calib_views(8, 13)
    packed2, _, pool2 = calib_pool(big, 8)
    d, d2 = _gpu(dev, packed), _gpu(dev, packed2)
    need, need2 = L.dcx_calibrate_workspace_bytes(B), L.dcx_calibrate_workspace_bytes(len(big))
    res = (ctypes.c_double * 16)()

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=8, offset=4 if misaligned else 0)
        st, pose = bufs.output("view_status", (B,), I32, SENTINEL), bufs.output("pose", (B, 8), F64, FSENT)

        def run():
            assert L.dcx_calibrate_pool(*corner_pool.ptrs(d.data_ptr(), B, pool)[:4], B, pool, *BOARD, *SIZE, ws.ptr, need, st.ptr,
                                        pose.ptr, res, _stream()) == 0
            return {"view_status": st.cpu().copy(), "pose": pose.cpu().copy(), "result": np.array(res[:], np.float64)}
        return run

    def left(bufs):
        tmp = torch.zeros(len(big) * 9, dtype=F64, device=bufs.dev)
        r2 = (ctypes.c_double * 16)()
        assert L.dcx_calibrate_pool(*corner_pool.ptrs(d2.data_ptr(), len(big), pool2)[:4], len(big), pool2, *BOARD, *SIZE,
                                    bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[len(big):].data_ptr(), r2, _stream()) == 0
        assert int(r2[12]) == 13                      # thirteen views stood

    def after(g, got):
        out = got["view_status"] != pnp.PNP_OK
        assert not got["pose"][out, :7].any() and got["pose"][:, 7].tolist() == [len(v) for v in views]
        return {"view_status": got["view_status"].tolist()}

    want, _ = drive(f"calibrate_pool/{'misaligned_by_4' if misaligned else 'aligned'}", dev, setup, left, after=after)
    assert want["view_status"].tolist() == expect
    dres = _calib_result(want["result"], want["view_status"], want["pose"])
    use = [b for b in range(B) if expect[b] in (pnp.PNP_OK, pnp.PNP_TOO_FEW)]                 # what the host can take
    h = calib.calibrate_camera_host_full([pnp.object_points(views[b][:, 2], *BOARD) for b in use],
                                         [views[b][:, :2].astype(np.float32) for b in use], SIZE)
    sel = np.array(use)
    _check(dres._replace(view_status=dres.view_status[sel], rvecs=dres.rvecs[sel], tvecs=dres.tvecs[sel], view_rms=dres.view_rms[sel],
                         view_points=dres.view_points[sel]), h, "calibrate_pool on guarded buffers", rms_floor=1e-12)   # (noise-free views)


def ransac_views(seed, n_ok):
    """calib_views with a planted wrong id in the first view, so that the consensus step has something to drop."""
    views, expect = calib_views(seed, n_ok)
    v = views[0]
    far = np.argmax(np.abs(v[:, 2] - v[0, 2]))
    v[0, 2], v[far, 2] = v[far, 2], v[0, 2]          # two ids swapped: both rows are wrong, the ids stay distinct
    views[0] = v[np.argsort(v[:, 2], kind="stable")]
    return views, expect


def test_calibrate_ransac_pool(dev, L):
    """dcx_calibrate_ransac_pool, raw, on calib_views' eight views with two swapped ids planted; 16 other views leave their
    contents.  The discrete outputs equal calibrate_camera_ransac_host_full's (whose margin is asserted first) and the
    continuous ones are, bit for bit, the plain device solve over the rows the host kept: test_gpu_calib_ransac's hand-built
    comparison.  d_inliers keeps its sentinel at slots of no view."""
    from test_calib_host import BOARD, SIZE
    from test_gpu_calib_ransac import MARGIN, _bits_equal, _same_discrete
    views, expect = ransac_views(7, 5)
    packed, owned, pool = calib_pool(views, 7)
    B = len(views)
    big, _ = ransac_views(8, 13)
    packed2, _, pool2 = calib_pool(big, 8)
    d, d2 = _gpu(dev, packed), _gpu(dev, packed2)
    it, args = 100, (100, 8.0, 3.0, 6, 2, 0)                                # iterations, consensus, reproj, min_inliers, rounds, seed
    need, need2 = L.dcx_calibrate_ransac_workspace_bytes(B, pool, it), L.dcx_calibrate_ransac_workspace_bytes(len(big), pool2, it)
    res = (ctypes.c_double * 16)()

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=16, offset=8)
        o = {"view_status": bufs.output("view_status", (B,), I32, SENTINEL), "pose": bufs.output("pose", (B, 8), F64, FSENT),
             "info": bufs.output("info", (B, 2), I32, SENTINEL), "inliers": bufs.output("inliers", (pool,), U8, USENT)}

        def run():
            assert L.dcx_calibrate_ransac_pool(*corner_pool.ptrs(d.data_ptr(), B, pool)[:4], B, pool, *BOARD, *SIZE, *args, ws.ptr, need,
                                               o["view_status"].ptr, o["pose"].ptr, o["info"].ptr, o["inliers"].ptr, res, _stream()) == 0
            got = {k: g.cpu().copy() for k, g in o.items()}
            got["inliers"] = got["inliers"][owned]
            got["result"] = np.array(res[:], np.float64)
            return got
        return run

    def left(bufs):
        n2 = len(big)
        tmp = torch.zeros(n2 * 10 + pool2, dtype=F64, device=bufs.dev)
        r2 = (ctypes.c_double * 16)()
        assert L.dcx_calibrate_ransac_pool(*corner_pool.ptrs(d2.data_ptr(), n2, pool2)[:4], n2, pool2, *BOARD, *SIZE, *args,
                                           bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[n2:].data_ptr(), tmp[9 * n2:].data_ptr(), None,
                                           r2, _stream()) == 0
        assert int(r2[12]) >= 12

    def after(g, got):
        assert g.out["inliers"].untouched(~owned), "a mask slot of no view written"
        out = got["view_status"] != pnp.PNP_OK
        assert not got["pose"][out, :7].any()
        return {"view_status": got["view_status"].tolist(), "inliers": got["info"][:, 0].tolist()}

    want, _ = drive("calibrate_ransac_pool", dev, setup, left, after=after)
    assert want["view_status"].tolist() == expect
    h, margin = calib.calibrate_camera_ransac_host_full(views[:-1], *BOARD, SIZE, with_margin=True, pool_order=True)
    assert margin >= MARGIN, margin
    mask = np.zeros(pool, bool)
    mask[owned] = want["inliers"].astype(bool)
    inl = [mask[int(packed[B + b]):int(packed[B + b]) + len(views[b])] for b in range(B - 1)]
    solves = int(want["result"][15])
    dres = calib.RobustCalibResult(*calib._common_fields(want["result"], want["view_status"][:-1], want["pose"][:-1]), inl,
                                   want["info"][:-1, 0].astype(np.int64), want["info"][:-1, 1].astype(np.int32), solves % 16, solves >= 16)
    _same_discrete(dres, h, "calibrate_ransac_pool on guarded buffers")
    assert (h.inliers[0] == False).sum() == 2                              # noqa: E712  (the two planted rows are out)
    kept = [v[m] if st == pnp.PNP_OK else v[:0] for v, m, st in zip(views[:-1], h.inliers, h.view_status)] + [views[-1][:0]]
    p = calib.calibrate_charuco_pool(*corner_pool.pack_keypoints(kept, dev), True, *BOARD, SIZE)
    _bits_equal([dres.rms, dres.camera_matrix, dres.dist_coeffs, dres.rvecs, dres.tvecs, dres.view_rms, dres.iterations, dres.attempts],
                [p.rms, p.camera_matrix, p.dist_coeffs, p.rvecs[:-1], p.tvecs[:-1], p.view_rms[:-1], p.iterations, p.attempts])


def stereo_views(seed, n, board=sx.BOARD_S):
    """n timestamps of which three lose a view to three different checks: camera 0's view of timestamp n-3 keeps three rows,
    camera 1's view of timestamp 1 carries an id outside the board, camera 0's view of the last timestamp goes last into its
    pool and is cut."""
    s = sx.scene(seed, n, "toe90", board, "A", "B", sigma=0.3, rows=[(30, 11)] * (n // 2) + [(8, 60)] * (n - n // 2))
    kps0, kps1 = [k.copy() for k in s.kps0], [k.copy() for k in s.kps1]
    kps0[n - 3] = kps0[n - 3][:3]
    kps1[1][2, 2] = (board[0] - 1) * (board[1] - 1)
    return s, kps0, kps1


def stereo_pools(kps0, kps1, seed):
    n = len(kps0)
    order = list(np.random.default_rng(seed).permutation(n - 1)) + [n - 1]
    pool0 = 2 + sum(len(k) + 3 for k in kps0) - 3 - 4                       # the last view of pool 0 loses four rows
    pool1 = 2 + sum(len(k) + 3 for k in kps1) + 5
    p0, _ = pool_cases.lay_frames(kps0, pool0, order, gap=3, first=2, filler=-9, id_sorted=True)
    p1, _ = pool_cases.lay_frames(kps1, pool1, order[::-1], gap=3, first=2, filler=-9, id_sorted=True)
    return p0, p1, pool0, pool1


def test_stereo_calibrate_pool(dev, L):
    """dcx_stereo_calibrate_pool, raw: eight timestamps of which three lose a view to three different checks (TOO_FEW, BAD_ID,
    TRUNCATED), so five pairs stand and the reductions run over timestamps that wrote nothing; 16 other timestamps leave their
    contents.  Against stereo_calibrate_host_full by test_gpu_stereo's _agree (the cut view is an empty view to the host)."""
    from test_gpu_stereo import _agree
    s, kps0, kps1 = stereo_views(61, 8)
    p0, p1, pool0, pool1 = stereo_pools(kps0, kps1, 1)
    B = 8
    s2, big0, big1 = stereo_views(62, 16)
    q0, q1, qpool0, qpool1 = stereo_pools(big0, big1, 2)
    d0, d1, e0, e1 = (_gpu(dev, a) for a in (p0, p1, q0, q1))
    cams = pnp._camera_args(*sx.cam_args(s)[:2]) + pnp._camera_args(*sx.cam_args(s)[2:])
    need, need2 = L.dcx_stereo_calibrate_workspace_bytes(B, pool0, pool1), L.dcx_stereo_calibrate_workspace_bytes(16, qpool0, qpool1)
    res = (ctypes.c_double * 16)()

    def call(a0, a1, n, pl0, pl1, ws_ptr, nbytes, st, pose, info, r):
        assert L.dcx_stereo_calibrate_pool(*corner_pool.ptrs(a0.data_ptr(), n, pl0)[:4], None, *corner_pool.ptrs(a1.data_ptr(), n, pl1)[:4],
                                           None, n, pl0, pl1, *s.board, *cams, ws_ptr, nbytes, st, pose, info, r, _stream()) == 0

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=16, offset=8)
        o = {"view_status": bufs.output("view_status", (B, 2), I32, SENTINEL), "pose": bufs.output("pose", (B, 8), F64, FSENT),
             "view_info": bufs.output("view_info", (B, 2, 2), F64, FSENT)}

        def run():
            call(d0, d1, B, pool0, pool1, ws.ptr, need, o["view_status"].ptr, o["pose"].ptr, o["view_info"].ptr, res)
            got = {k: g.cpu().copy() for k, g in o.items()}
            got["result"] = np.array(res[:], np.float64)
            return got
        return run

    def left(bufs):
        tmp = torch.zeros(16 * 14, dtype=F64, device=bufs.dev)
        r2 = (ctypes.c_double * 16)()
        call(e0, e1, 16, qpool0, qpool1, bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[16:].data_ptr(), tmp[16 * 9:].data_ptr(), r2)
        assert int(r2[9]) == 13                       # thirteen pairs stood

    def after(g, got):
        pair = (got["view_status"] == pnp.PNP_OK).all(1)
        assert not got["pose"][~pair].any() and not got["view_info"][~pair, :, 0].any()
        return {"view_status": got["view_status"].tolist()}

    want, _ = drive("stereo_calibrate_pool", dev, setup, left, after=after)
    OKs, FEW, BAD, CUT = pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_TRUNCATED
    exp = [[OKs, OKs] for _ in range(B)]
    exp[5][0], exp[1][1], exp[7][0] = FEW, BAD, CUT
    assert want["view_status"].tolist() == exp
    r = want["result"]
    assert int(r[11]) == stereo.STEREO_OK and int(r[9]) == 5
    R = pnp._rodrigues(r[0:3])
    E, F = stereo.essential_fundamental(R, r[3:6], *(pnp._camera(c) for c in sx.cam_args(s)[::2]))
    pose, info = want["pose"], want["view_info"]
    dres = stereo.StereoResult(0, float(r[6]), R, r[3:6].copy(), r[0:3].copy(), E, F, want["view_status"], pose[:, 0:3].copy(),
                               pose[:, 3:6].copy(), pose[:, 6].copy(), pose[:, 7].astype(np.int64), info[:, :, 0].copy(),
                               info[:, :, 1].astype(np.int64), int(r[7]), int(r[8]), int(r[9]), int(r[10]))
    host0 = kps0[:7] + [np.zeros((0, 3))]
    h = stereo.stereo_calibrate_host_full(host0, kps1, *s.board, *sx.cam_args(s))
    assert h.view_status[7, 0] == FEW
    _agree(dres._replace(view_status=h.view_status), h, "stereo_calibrate_pool on guarded buffers")


# --------------------------------------------------------------------------- entries whose workspace contents the suite already varies

@pytest.mark.parametrize("frames_of_room", [3, 1], ids=["whole_batch", "one_frame_chunks"])
@pytest.mark.parametrize("paths", [4, 8])
def test_sgm_and_speckle_filter(dev, L, paths, frames_of_room):
    """dcx_sgm_u8_paths (D = 64) and dcx_filter_speckles_s16 on the limits test's 11 x 70 batch of three: exact-size workspaces
    (the whole batch's, and one frame's so that the batch is chunked) and the disparities between guards on both sides.  Both
    kernels rewrite every byte of their workspace (census words and S; a label and a size per pixel): exempt from the second
    half of rule 5."""
    h, w, D = 11, 70, 64
    left_np, right_np = lc.small_batch(0)
    kw = dict(min_disparity=-3, num_disparities=D, paths=paths)
    want_sgm = dp.sgm_host(left_np, right_np, **kw)
    want_flt = dp.filter_speckles_host(want_sgm, 16 * (-3 - 1), 100, 32)
    tl, tr = _gpu(dev, left_np), _gpu(dev, right_np)
    oth = tuple(_gpu(dev, a) for a in lc.broadcast_batch())
    need_s, need_f = dp.sgm_workspace_bytes(frames_of_room, h, w, D), dp.filter_speckles_workspace_bytes(frames_of_room, h, w)

    def setup(bufs):
        ws_s, ws_f = bufs.workspace("sgm_ws", need_s, align=16, offset=8), bufs.workspace("filter_ws", need_f, align=16, offset=8)
        disp, flt = bufs.output("disp16", (3, h, w), I16, 77), bufs.output("filtered", (3, h, w), I16, 77)

        def run():
            dp.sgm_device(tl, tr, out=disp.t, workspace=ws_s.body, **kw)
            dp.filter_speckles_device(disp.t, 16 * (-3 - 1), 100, 32, out=flt.t, workspace=ws_f.body)
            torch.cuda.synchronize()
            return {"disp16": disp.cpu().copy(), "filtered": flt.cpu().copy()}
        return run

    def left(bufs):
        dp.sgm_device(oth[0], oth[1][0], num_disparities=64, workspace=bufs.ws["sgm_ws"].body, paths=12 - paths)
        dp.filter_speckles_device(_gpu(dev, lc.speckle_batch(8)[0, :9, :65]), lc.NV, 40, 40, workspace=bufs.ws["filter_ws"].body)

    want, _ = drive(f"sgm_u8_paths+filter_speckles/paths{paths}/room{frames_of_room}", dev, setup, left, rewritten=("sgm_ws", "filter_ws"))
    assert np.array_equal(want["disp16"], want_sgm) and np.array_equal(want["filtered"], want_flt)
    assert (want_flt != want_sgm).any() and (want_sgm != 16 * (-3 - 1)).any()


def _guards_only(key, bufs, notes=None):
    assert not bufs.damage(), f"{key}: guard damaged at offset (relative to the buffer) {bufs.damage()}"
    _report(key, dict(notes or {}, outputs={n: g.nbytes for n, g in bufs.out.items()}, guards="intact on both sides"))


def test_disparity_to_points(dev):
    """dcx_disparity_to_points: the xyz points between guards, against disparity_to_points_host cast to float32 as
    test_gpu_disparity compares them (equal NaN positions, equal or one ulp)."""
    from test_gpu_disparity import _ulps
    h, w = 11, 70
    disp = dp.sgm_host(*lc.small_batch(0), min_disparity=-3)
    Q = np.array([[1.0, 0, 0, -35.0], [0, 1.0, 0, -5.5], [0, 0, 0, 80.0], [0, 0, 12.5, 0.25]])
    want = dp.disparity_to_points_host(disp, Q, -3).astype(np.float32)
    bufs = Bufs(dev, True)
    xyz = bufs.output("xyz", (3, h, w, 3), F32, FSENT)
    dp.disparity_to_points_device(_gpu(dev, disp), Q, -3, out=xyz.t)
    torch.cuda.synchronize()
    got, nan = xyz.cpu(), np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.any() and not nan.all()
    assert _ulps(got[~nan], want[~nan]).max() <= 1
    _guards_only("disparity_to_points/11x70/b3", bufs)


def test_remap_map_and_rectified_points(dev):
    """dcx_undistort_rectify_map (37 x 19), dcx_remap_u8 at 19 x 37 with B = F + 1 (the byte-store path, whose last thread holds
    fewer than kPix pixels; gray and BGR) and dcx_rectify_points_pool at pools of 1, 63, 64 and 65 slots: every output between
    guards, against the host definitions by test_gpu_rectify's own comparisons."""
    from test_gpu_rectify import F, _map_agrees, _points_agree, _pool, _random_map, _rectify, _strided_source
    r = _rectify("verge15", "B", "C")
    K, d = sx.cam("B")
    bufs = Bufs(dev, True)
    Ks, Ps = K.copy(), r.P1.copy()
    Ks[:2] *= 41.0 / rx.SIZE[0]
    Ps[:2] *= 37.0 / rx.SIZE[0]
    m = bufs.output("map", (19, 37, 2), I32, SENTINEL)
    _map_agrees(dev, Ks, d, r.R1, Ps, 37, 19, "37x19 of 41x23 into a guarded map", out=m.t)
    rng = np.random.default_rng([61, 19, 37])
    mp = _random_map(rng, 19, 37)
    md = _gpu(dev, mp)
    for ch in (1, 3):
        src, host_src = _strided_source(dev, rng, F + 1, ch)
        out = bufs.output(f"remap{ch}", (F + 1, 19, 37) + ((3,) if ch == 3 else ()), U8, 0xA7)
        rc.remap_device(src, md, 7, out=out.t)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu(), rc.remap_host(host_src, mp, 7)), ch
    for n in (1, 63, 64, 65):
        xy = np.stack([rng.uniform(-20, rx.SIZE[0] + 20, n), rng.uniform(-20, rx.SIZE[1] + 20, n)], 1).astype(np.float32)
        pts = bufs.output(f"points{n}", (n, 2), F64, FSENT)
        rc.rectify_points_pool(_pool(dev, xy), 1, n, True, K, d, r.R1, r.P1, out=pts.t)
        torch.cuda.synchronize()
        _points_agree(pts.t, rc.rectify_points_host(xy.astype(np.float64), K, d, r.R1, r.P1), f"guarded points, n = {n}")
    _guards_only("undistort_rectify_map+remap_u8+rectify_points_pool", bufs)


def test_solve_pnp_pool(dev):
    """dcx_solve_pnp_pool on the six-frame pool of the consensus test: status and pose between guards, every frame held to
    solve_pnp_host_full by test_gpu_pnp's _agree (d_pose zeros unless OK)."""
    from test_gpu_pnp import _agree
    from test_pnp_host import DIST5, K
    frames, _ = ransac_frames()
    packed, _, pool = ransac_pool(frames, [5, 0, 4, 1, 3, 2], 3)
    B = len(frames)
    bufs = Bufs(dev, True)
    st, pose = bufs.output("status", (B,), I32, SENTINEL), bufs.output("pose", (B, 8), F64, FSENT)
    pnp.solve_pnp_pool(_gpu(dev, packed), B, pool, True, *PNP_BOARD, K, DIST5, out=(st.t, pose.t))
    torch.cuda.synchronize()
    got_st, got_pose = st.cpu(), pose.cpu()
    tally = [0, 0, 0]
    for b, f in enumerate(frames):
        hs, hp = {2: (pnp.PNP_TRUNCATED, None), 3: (pnp.PNP_BAD_ID, None)}.get(b) or pnp.solve_pnp_host_full(f, *PNP_BOARD, K, DIST5)
        assert got_st[b] == hs, (b, got_st[b], hs)                 # (the host raises on the bad id and never sees a pool's end)
        if hs == pnp.PNP_OK:
            _agree(got_pose[b], hp, tally)
        else:
            assert not got_pose[b].any()
    assert got_st[0] == pnp.PNP_OK and sum(tally) >= 2 and len(set(got_st.tolist())) == 5
    _guards_only("solve_pnp_pool/6_frames", bufs, {"status": got_st.tolist()})
