"""The instrument every recorded performance figure passes through, run on the GPU: the per-launch profile hooks of
csrc/dcx_conv_mfma.hip (records, filter, sampling, the clock probes workgroup 0 of every conv kernel stores while profiling is on),
the stage timers of csrc/dcx_api.hip, the XCD shares' getter and dcx_stream_synchronize.

What is compared with what:
  * records of a call  -- the list tests/instrument_cases.py derives from the ORACLE's layers and the header (never from the library);
  * kernels under probing -- oracle/conv_exact.c of the kernel's family, by bits; the fused heads, the whole pipeline and one launch
    chosen for its length -- the same call with profiling off, by bits;
  * event times -- the host's wall clock around the call (an upper bound: brackets on one stream are disjoint);
  * clocks -- the device's maximum shader clock as the runtime reports it.

Frames are 64x96 (the tiny_noise_64x96 fixture and its weights), batches 1 and 3; conv layers come from test_gpu_parity.CONV_CASES.
The hooks are process-global: every test runs inside ``hooks(L)``, which puts them back in a ``finally`` -- profile off, filter -1,
sample 1, timing off, equal XCD shares -- and the last test of the file checks that graphs are usable again.
Figures measured on the way go to instrument_report.json in the suite's report directory."""
import contextlib
import ctypes as C
import json
import math
import os
import time
import zlib

import numpy as np
import pytest
import torch

import instrument_cases as IC
from conftest import REPO
from deepcharuco_amd import weights as W
from test_gpu_parity import CONV_CASES, _conv_layer, _family

pytestmark = pytest.mark.gpu

H, WD, KMAX = 64, 96, 64
REPORT = {}


def _report(key, value):
    REPORT[key] = value
    with open(os.path.join(REPO, ".gitignore")) as f:
        names = [l.strip().rstrip("/") for l in f if l.strip().endswith("_out/")]
    out = os.path.join(REPO, names[0] if names else "reports_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "instrument_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, default=float)
    print(f"[instrument] {key}: {value}")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from deepcharuco_amd import _lib
    return _lib.lib()


def _ok(rc, where):
    assert rc == 0, f"{where} returned {rc}"


def _restore(L):
    L.dcx_profile_enable(0)
    L.dcx_profile_filter(-1)
    L.dcx_profile_sample(1)
    L.dcx_set_timing(0)
    w = (C.c_float * 8)()
    if L.dcx_get_xcd_weights(w) != 0 or list(w) != [1.0] * 8:     # (every set takes one of the 256 device tables: only when needed)
        L.dcx_set_xcd_weights(None)


@contextlib.contextmanager
def hooks(L):
    """The process-global hooks are put back whatever happens inside, a failed assertion included."""
    try:
        yield
    finally:
        torch.cuda.synchronize()
        _restore(L)


def _session(L, kernel_filter=-1, every=1):
    """Starts a profile session the way bench.py does: filter, sample, then enable."""
    _ok(L.dcx_profile_filter(kernel_filter), "dcx_profile_filter")
    _ok(L.dcx_profile_sample(every), "dcx_profile_sample")
    _ok(L.dcx_profile_enable(1), "dcx_profile_enable")
    assert L.dcx_profile_count() == 0


def _fetch(L, max_records=None):
    n = L.dcx_profile_count()
    m = n if max_records is None else max_records
    k = max(m, 1)
    ids, nimg, lim, fl, ms = (C.c_int * k)(), (C.c_int * k)(), (C.c_int * k)(), (C.c_double * k)(), (C.c_float * k)()
    got = L.dcx_profile_fetch(ids, nimg, lim, fl, ms, m)
    assert got == min(n, m)
    return [dict(id=ids[i], n=nimg[i], limited=lim[i], flops=fl[i], ms=ms[i]) for i in range(got)]


def _clocks(L, n):
    ghz = (C.c_float * max(n, 1))()
    assert L.dcx_profile_clocks(ghz, n) == min(n, L.dcx_profile_count())
    return [float(v) for v in ghz[:n]]


def _words(L, record):
    out = (C.c_ulonglong * IC.CLK_WORDS)()
    _ok(L.dcx_profile_probe_words(record, out), f"dcx_profile_probe_words({record})")
    return np.array(out[:], dtype=np.uint64)


def _names(L):
    names = []
    while L.dcx_profile_kernel_name(len(names)) != b"?":
        names.append(L.dcx_profile_kernel_name(len(names)).decode())
    return names


def _check_own_probes(w, what):
    assert all(int(v) != 0 for v in w[:4]), f"{what}: start / end probes not written: {w[:4]}"
    assert int(w[2]) >= int(w[0]) and int(w[3]) >= int(w[1]), f"{what}: a clock ran backwards: {w[:4]}"


def _device_max_khz(dev):
    """The device's maximum shader clock in kHz as the runtime reports it: torch's device properties where they carry it, else
    hipDeviceGetAttribute(hipDeviceAttributeClockRate) of the HIP runtime this process has loaded.  0 if neither can be had (the
    attribute's number is checked on one whose value torch does report, the CU count)."""
    props = torch.cuda.get_device_properties(dev)
    if getattr(props, "clock_rate", 0):
        return int(props.clock_rate)
    with open("/proc/self/maps") as f:
        paths = sorted({l.split()[-1] for l in f if "libamdhip64" in l})
    if len(paths) != 1:
        return 0
    hip = C.CDLL(paths[0])
    v = C.c_int(0)
    clock_rate, cu_count = 5, 63          # hipDeviceAttributeClockRate, hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    if hip.hipDeviceGetAttribute(C.byref(v), cu_count, dev.index) != 0 or v.value != props.multi_processor_count:
        return 0
    if hip.hipDeviceGetAttribute(C.byref(v), clock_rate, dev.index) != 0:
        return 0
    return int(v.value)


def _case_tensors(case, salt):
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000 + salt)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    bn = None
    if has_bn:
        bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1,
              torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5)
    return x, wt, b, bn


def _case_exact(case, tensors, family):
    from oracle.conv_exact import conv_exact
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    x, wt, b, bn = tensors
    return conv_exact(x.numpy(), wt.numpy(), b.numpy(), None if bn is None else [t.numpy() for t in bn],
                      pad=pad, ups=bool(ups), pool=bool(pool), family=family)


def _case_pick(L, case):
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    ho, wo = (h << ups) + 2 * pad - (ks - 1), (w << ups) + 2 * pad - (ks - 1)
    return L.dcx_conv_pick_name_ups(n, cin, ho, wo, cout, ks, int(pool), 0 if has_bn else 1, int(ups)).decode()


def _case_work(case):
    name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
    return n * cin * cout * ks * ks * (h << ups) * (w << ups)


def _case(name):
    return next(c for c in CONV_CASES if c[0] == name)


SMALLEST = min((c for c in CONV_CASES if c[9] == 3), key=_case_work)      # the smallest 3x3 layer of the list


class RawConv:
    """dcx_conv_layer on buffers made once: many launches of one layer without a conversion or an allocation of the test's between
    them (dcx_conv_layer itself synchronises the stream before it returns)."""

    def __init__(self, L, dev, case, salt=7):
        name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = case
        self.L, self.case = L, case
        x, wt, b, bn = _case_tensors(case, salt)
        ho, wo = (h << ups) + 2 * pad - (ks - 1), (w << ups) + 2 * pad - (ks - 1)
        self.flops = 2 * cout * cin * ks * ks * ho * wo
        hs, ws_ = (ho // 2, wo // 2) if pool else (ho, wo)
        xd = x.to(dev).contiguous()
        self.c4 = torch.empty((n, cin // 4, h, w, 4), device=dev)
        _ok(L.dcx_nchw_to_c4(xd.data_ptr(), n, cin, h, w, self.c4.data_ptr(), None), "to_c4")
        self.out4 = torch.zeros((n, (cout + 3) // 4, hs, ws_, 4), device=dev)
        self.host = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (wt, b) + tuple(bn or ())]
        self.args = [a.ctypes.data for a in self.host] + [None] * (6 - len(self.host))
        torch.cuda.synchronize()

    def launch(self):
        name, n, cin, cout, h, w, pad, ups, pool, ks, has_bn = self.case
        _ok(self.L.dcx_conv_layer(self.c4.data_ptr(), n, cin, h, w, *self.args, cout, ks, pad, ups, int(pool), int(has_bn),
                                  self.out4.data_ptr(), None), "dcx_conv_layer")


@pytest.fixture(scope="module")
def table(L, dev):
    """The probe table exists from the first profiled conv launch of the process on: make that launch, so that every test may
    read slots before its own first launch."""
    with hooks(L):
        _session(L)
        RawConv(L, dev, SMALLEST).launch()
        assert L.dcx_profile_count() == 1
    return True


class Tiny:
    """The tiny fixture's models, three 64x96 frames (the fixture's and two more noise frames) and what the pipeline returns for
    them with every hook off."""

    def __init__(self, dev):
        from conftest import GoldenCase
        from deepcharuco_amd.models.net import dcModel, lModel
        from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
        self.case = GoldenCase("tiny_noise_64x96")
        self.dev = dev
        self.dc = lModel(dcModel(self.case.n_ids, self.case.sd_dc, dev))
        self.rn = lRefineNet(RefineNet(self.case.sd_rn, dev))
        frames = np.concatenate([self.case.frame[None]] + [W.synthetic_frames("noise", 50 + i, 1, H, WD) for i in range(2)])
        self.frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        self.plain = {b: self.run(b) for b in (1, 3)}
        assert self.plain[3][1].tolist()[0] == self.case.fx["final_rn"].shape[0] and int(self.plain[3][1].sum()) >= 8

    def run(self, b, sync=True):
        from deepcharuco_amd.inference import infer_batch_device
        packed = infer_batch_device(self.frames[:b], self.case.n_ids, self.dc, self.rn, kmax=KMAX)
        if not sync:
            return packed
        torch.cuda.synchronize()
        return self.unpack(packed, b)

    def unpack(self, packed, b):
        from deepcharuco_amd.inference import unpack_results
        return unpack_results(packed.cpu().numpy(), b, b * KMAX, True)


def _same_results(a, b):
    return (np.array_equal(a[1], b[1]) and len(a[0]) == len(b[0])
            and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[0], b[0])))


@pytest.fixture(scope="module")
def tiny(dev):
    return Tiny(dev)


def _check_records(L, recs, expected, names, what):
    """Records against the expected list: ids of the brackets, the instantiation the cost model names for each conv shape, n,
    limited and flops exactly, every event time positive."""
    assert len(recs) == len(expected), f"{what}: {len(recs)} records, {len(expected)} expected: {[r['id'] for r in recs]}"
    for i, (r, e) in enumerate(zip(recs, expected)):
        where = f"{what}, record {i} ({'+'.join(e.layers) or 'finalize'})"
        if e.kernel_id is not None:
            assert r["id"] == e.kernel_id, f"{where}: id {r['id']}"
        else:
            want = L.dcx_conv_pick_name_ups(*e.pick).decode()
            assert 0 <= r["id"] < len(names) and names[r["id"]] == want, f"{where}: {L.dcx_profile_kernel_name(r['id'])} != {want}"
        assert (r["n"], r["limited"]) == (e.n, e.limited), f"{where}: n, limited = {r['n']}, {r['limited']}"
        assert r["flops"] == float(e.flops), f"{where}: flops_per_image {r['flops']} != {e.flops}"
        assert r["ms"] > 0, f"{where}: ms = {r['ms']}"


# --------------------------------------------------------------------------- a. probing changes no bits and stays in its slot

def _heat_run(L, dev, rf, patches_d):
    p = patches_d.shape[0]
    ws = torch.empty(L.dcx_refiner_workspace_bytes(rf.handle, p), dtype=torch.uint8, device=dev)
    corners = torch.full((p, 2), -7, dtype=torch.int32, device=dev)
    heat = torch.full((p, 64, 64), float("nan"), device=dev)
    _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), p, None, None, ws.data_ptr(), ws.numel(), corners.data_ptr(), None,
                              heat.data_ptr(), None), "dcx_refiner_forward")
    torch.cuda.synchronize()
    return corners.cpu().numpy(), heat.cpu().numpy()


# One launch chosen so that workgroup 0 runs MORE than the 20 units the probe window holds (a unit = 16 input channels of one work
# item): 1,152 items of 8 units each on at most 512 workgroups give workgroup 0 three items = 24 units on a 256-CU device.  None of
# CONV_CASES gets there (its two XCD-walk cases give workgroup 0 three and two items of four units: 12 and 8 stamped units on an
# MI355X, instrument_report.json), so this one shape is the file's own.
WINDOW_CASE = ("window_24_units", 6, 128, 128, 96, 128, 1, 0, 0, 3, True)


def test_probing_changes_no_bits_and_stays_in_its_slot(dev, L, tiny, table, monkeypatch):
    """With profiling on every recorded conv launch gets a clk_probe pointer and workgroup 0 takes another path.  Every non-HEAT
    instantiation runs once under DCX_FORCE_CFG on the smallest CONV_CASES entry it accepts and must equal conv_exact of its family by
    bits; both W2H_600_items_xcd_walk* cases run on the cost model's own choice; the two HEAT instantiations run through
    dcx_refiner_forward and WINDOW_CASE once more on the default choice, both against the same call with profiling off.  After each
    launch: the record's own words 0-3 are written and ordered, and the 64 words of the NEXT slot are what they were before."""
    from deepcharuco_amd.models.refinenet import RefineNet
    names = _names(L)
    heat_cfgs = [n_ for n_ in names if "HEAT" in n_]
    assert len(heat_cfgs) == 2
    rf = RefineNet(tiny.case.sd_rn, dev)
    g = torch.Generator().manual_seed(77)
    patches_d = (torch.rand(18, 24, 24, generator=g) - 0.5).to(dev)
    win_t = _case_tensors(WINDOW_CASE, 5)
    plain_heat = {}
    for cfg in heat_cfgs:
        monkeypatch.setenv("DCX_FORCE_CFG", cfg)
        plain_heat[cfg] = _heat_run(L, dev, rf, patches_d)
    monkeypatch.delenv("DCX_FORCE_CFG")
    plain_win = _conv_layer(win_t[0].to(dev), *win_t[1:], WINDOW_CASE[6], WINDOW_CASE[7], WINDOW_CASE[8]).cpu().numpy()
    ran, units = {}, {}
    with hooks(L):
        _session(L)
        rec = 0

        def conv_checked(case, tensors, ref, what):
            nonlocal rec
            nxt = _words(L, rec + 1)
            got = _conv_layer(tensors[0].to(dev), tensors[1], tensors[2], tensors[3], case[6], case[7], case[8], case[9]).cpu().numpy()
            assert L.dcx_profile_count() == rec + 1, f"{what}: not exactly one record"
            own = _words(L, rec)
            _check_own_probes(own, what)
            assert np.array_equal(_words(L, rec + 1), nxt), f"{what}: the next slot's words changed"
            nbad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
            assert nbad == 0, f"{what}: {nbad} of {got.size} elements differ under probing"
            rec += 1
            return own

        by_size = sorted(CONV_CASES, key=_case_work)
        refs = {}
        for cfg in names:
            if cfg in heat_cfgs:
                continue
            monkeypatch.setenv("DCX_FORCE_CFG", cfg)
            case = next((c for c in by_size if _case_pick(L, c) == cfg), None)
            assert case is not None, f"{cfg} accepts no CONV_CASES entry"
            key = (case[0], _family(cfg))
            if key not in refs:
                refs[key] = _case_exact(case, _case_tensors(case, 3), key[1])
            conv_checked(case, _case_tensors(case, 3), refs[key], f"{cfg} on {case[0]}")
            assert _fetch(L)[-1]["id"] == names.index(cfg)
            ran[cfg] = case[0]
        monkeypatch.delenv("DCX_FORCE_CFG")
        for nm in ("W2H_600_items_xcd_walk", "W2H_600_items_xcd_walk_pool"):
            case = _case(nm)
            cfg = _case_pick(L, case)
            t = _case_tensors(case, 3)
            own = conv_checked(case, t, _case_exact(case, t, _family(cfg)), f"{nm} on its own choice {cfg}")
            units[nm] = int(np.count_nonzero(own[4:])) // 3
        own = conv_checked(WINDOW_CASE, win_t, plain_win, "WINDOW_CASE")
        units[WINDOW_CASE[0]] = int(np.count_nonzero(own[4:])) // 3
        # the window is full and ends with the slot: all of words 4..63 written, the next slot untouched (checked above)
        assert np.count_nonzero(own[4:]) == 60, f"per-unit window of WINDOW_CASE: {np.count_nonzero(own[4:])} of 60 words written"
        for cfg in heat_cfgs:       # one dcx_refiner_forward = 12 records; the head is the 11th, the finalize bracket the slot behind it
            monkeypatch.setenv("DCX_FORCE_CFG", cfg)
            nxt = _words(L, rec + 11)
            corners, heat = _heat_run(L, dev, rf, patches_d)
            assert L.dcx_profile_count() == rec + 12
            assert _fetch(L)[rec + 10]["id"] == names.index(cfg)
            _check_own_probes(_words(L, rec + 10), cfg)
            assert np.array_equal(_words(L, rec + 11), nxt) and not nxt.any(), f"{cfg}: the slot behind the head changed"
            assert not _words(L, rec).any(), "the conv1a bracket's slot holds probes"
            assert np.array_equal(corners, plain_heat[cfg][0]), f"{cfg}: corners differ under probing"
            assert np.array_equal(heat.view(np.uint32), plain_heat[cfg][1].view(np.uint32)), f"{cfg}: heat-map bits differ under probing"
            rec += 12
            ran[cfg] = "dcx_refiner_forward, 18 patches"
        monkeypatch.delenv("DCX_FORCE_CFG")
    assert sorted(ran) == sorted(names)
    _report("probed_instantiations", ran)
    _report("units_stamped_by_workgroup_0", units)


# --------------------------------------------------------------------------- b. the records of a whole call

def test_records_of_a_whole_call(dev, L, tiny, table):
    """dcx_infer_batch on three tiny frames, unfiltered: exactly the expected list in launch order, every event time positive and
    their sum within the host's wall time around the call, the corners those of the same call with profiling off."""
    names = _names(L)
    b = 3
    expected = IC.expected_infer_batch(b, H, WD, b * KMAX, tiny.case.n_ids)
    with hooks(L):
        _session(L)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed = tiny.run(b, sync=False)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        recs = _fetch(L)
        _check_records(L, recs, expected, names, "dcx_infer_batch")
        assert [r["id"] for r in recs if r["id"] >= 100] == [100, 102, 101, 103]
        assert all(r["flops"] == 0.0 for r in recs if r["id"] >= 100) and all(r["flops"] > 0 for r in recs if r["id"] < 100)
        total_ms = sum(r["ms"] for r in recs)
        _report("infer_batch_3x64x96", dict(sum_of_brackets_ms=total_ms, host_wall_ms=wall_ms))
        assert total_ms <= wall_ms, f"brackets sum to {total_ms} ms inside {wall_ms} ms of wall time"
        assert _same_results(tiny.unpack(packed, b), tiny.plain[b]), "corners differ with profiling on"
        clocks = _clocks(L, len(recs))
        assert all(c == 0.0 for c, r in zip(clocks, recs) if r["id"] >= 100), "a bracket without probes reports a clock"
        assert all(math.isfinite(c) and c >= 0.0 for c in clocks)


def test_records_of_the_staged_chain(dev, L, tiny, table):
    """dcx_detector_forward, then dcx_refiner_forward with and without a device-side patch count: the expected lists, and
    limited = 1 exactly on the launches that take the count."""
    from deepcharuco_amd.models.refinenet import RefineNet
    names = _names(L)
    b, p = 3, 18
    det, rf = tiny.dc.model, RefineNet(tiny.case.sd_rn, dev)
    ws = torch.empty(L.dcx_detector_workspace_bytes(det.handle, b, H, WD), dtype=torch.uint8, device=dev)
    loc = torch.empty((b, 65, H // 8, WD // 8), device=dev)
    ids = torch.empty((b, tiny.case.n_ids + 1, H // 8, WD // 8), device=dev)
    g = torch.Generator().manual_seed(78)
    patches_d = (torch.rand(p, 24, 24, generator=g) - 0.5).to(dev)
    table_d = torch.tensor([[0, 40 + i, 30, i] for i in range(p)], dtype=torch.int32, device=dev)       # {frame, x, y, slot}
    total_d = torch.tensor([p - 5], dtype=torch.int32, device=dev)
    ws_r = torch.empty(L.dcx_refiner_workspace_bytes(rf.handle, p), dtype=torch.uint8, device=dev)
    corners = torch.zeros((p, 2), dtype=torch.int32, device=dev)
    xy = torch.zeros((p, 2), device=dev)
    with hooks(L):
        _session(L)
        _ok(L.dcx_detector_forward(det.handle, tiny.frames.data_ptr(), H * WD, WD, None, b, H, WD, ws.data_ptr(), ws.numel(),
                                   loc.data_ptr(), ids.data_ptr(), None), "dcx_detector_forward")
        _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), p, total_d.data_ptr(), table_d.data_ptr(), ws_r.data_ptr(),
                                  ws_r.numel(), corners.data_ptr(), xy.data_ptr(), None, None), "dcx_refiner_forward (limited)")
        _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), p, None, None, ws_r.data_ptr(), ws_r.numel(),
                                  corners.data_ptr(), None, None, None), "dcx_refiner_forward (unlimited)")
        torch.cuda.synchronize()
        expected = (IC.expected_detector_forward(b, H, WD, tiny.case.n_ids) + IC.expected_refiner_forward(p, True)
                    + IC.expected_refiner_forward(p, False))
        recs = _fetch(L)
        _check_records(L, recs, expected, names, "staged chain")
        assert [r["limited"] for r in recs] == [0] * 11 + [1] * 12 + [0] * 12


# --------------------------------------------------------------------------- c. filter and sampling

def test_filter_selects_one_instantiation(dev, L, tiny, table):
    names = _names(L)
    b = 3
    expected = IC.expected_infer_batch(b, H, WD, b * KMAX, tiny.case.n_ids)
    want = [L.dcx_conv_pick_name_ups(*e.pick).decode() for e in expected if e.pick]
    cfg = max(set(want), key=want.count)
    k = want.count(cfg)
    assert k >= 2, f"no instantiation occurs twice in the call: {want}"
    with hooks(L):
        _session(L, kernel_filter=names.index(cfg))
        tiny.run(b)
        recs = _fetch(L)
        assert len(recs) == k and {r["id"] for r in recs} == {names.index(cfg)}, [r["id"] for r in recs]
        assert [(r["n"], r["limited"], r["flops"]) for r in recs] == \
               [(e.n, e.limited, float(e.flops)) for e in expected if e.pick and L.dcx_conv_pick_name_ups(*e.pick).decode() == cfg]
        # fewer than recorded: that many, the oldest first
        assert _fetch(L, max_records=k - 1) == recs[:k - 1]
        assert _fetch(L, max_records=0) == []
    _report("filtered_instantiation", dict(kernel=cfg, records=k))


def test_sampling_counts_matching_launches(dev, L, table):
    """dcx_profile_sample(5) before dcx_profile_enable(1), as bench.py sets them: 20 matching launches give exactly 4 records, and a
    launch of another instantiation in between neither counts nor is recorded.  The header's rule for the count: only
    dcx_profile_sample restarts it -- a new session continues where the last one stopped."""
    names = _names(L)
    kid = names.index(_case_pick(L, SMALLEST))
    small = RawConv(L, dev, SMALLEST)
    other = RawConv(L, dev, next(c for c in sorted(CONV_CASES, key=_case_work) if names.index(_case_pick(L, c)) != kid))
    with hooks(L):
        _session(L, kernel_filter=kid, every=5)
        for i in range(20):
            small.launch()
            if i == 7:
                other.launch()
        recs = _fetch(L)
        assert len(recs) == 4 and all(r["id"] == kid and r["flops"] == float(small.flops) and r["ms"] > 0 for r in recs)
        # the count restarts with dcx_profile_sample alone
        _session(L, kernel_filter=kid, every=5)          # count = 0
        for _ in range(3):
            small.launch()                               # launches 0 (recorded), 1, 2
        assert L.dcx_profile_count() == 1
        _ok(L.dcx_profile_enable(1), "dcx_profile_enable")           # a new session: the list is cleared, the count goes on at 3
        assert L.dcx_profile_count() == 0
        for _ in range(2):
            small.launch()                               # launches 3, 4: not recorded (a restarted count would record the first)
        assert L.dcx_profile_count() == 0
        small.launch()                                   # launch 5
        assert L.dcx_profile_count() == 1
        # 0 and negative values are 1: every launch
        for every in (0, -3):
            _session(L, kernel_filter=kid, every=every)
            for _ in range(3):
                small.launch()
            assert L.dcx_profile_count() == 3, every


# --------------------------------------------------------------------------- d. clocks

def test_clock_of_a_long_launch_and_no_stale_clock(dev, L, tiny, table):
    """W2H_600_items_xcd_walk (measured on an MI355X: the launch 0.037 ms between its events, workgroup 0 alone 3,044 ticks of the
    100 MHz clock and 62,464 shader cycles = 2.05 GHz, so one tick is 0.03 %; the test asserts at least 100 ticks): its clock is
    finite, positive and not above the device's maximum shader clock (hipDeviceAttributeClockRate: 2.4 GHz).  The margin is the tick
    granularity of this very launch: both real-time reads are floored to a tick, so the true span is below ticks + 1.
    Then sessions that write no probes into slots an earlier session used: a lone conv1a bracket in slot 0, and a RefineNet call
    whose device-side patch count is 0 (workgroup 0 of every conv returns before its first probe) must report clock 0."""
    from deepcharuco_amd.models.refinenet import RefineNet
    long_conv = RawConv(L, dev, _case("W2H_600_items_xcd_walk"))
    det, rf = tiny.dc.model, RefineNet(tiny.case.sd_rn, dev)
    p = 18
    g = torch.Generator().manual_seed(79)
    patches_d = (torch.rand(p, 24, 24, generator=g) - 0.5).to(dev)
    ws_r = torch.empty(L.dcx_refiner_workspace_bytes(rf.handle, p), dtype=torch.uint8, device=dev)
    corners = torch.zeros((p, 2), dtype=torch.int32, device=dev)
    zero_d = torch.zeros(1, dtype=torch.int32, device=dev)
    front = torch.empty(L.dcx_front_bytes(det.handle, 1, H, WD), dtype=torch.uint8, device=dev)
    assert front.numel() > 0
    with hooks(L):
        _session(L)
        long_conv.launch()                               # warm
        long_conv.launch()
        recs, w = _fetch(L), _words(L, 1)
        ghz = _clocks(L, 2)[1]
        ticks, cycles = int(w[3]) - int(w[1]), int(w[2]) - int(w[0])
        max_khz = _device_max_khz(dev)
        _report("clock_of_W2H_600", dict(launch_ms=recs[1]["ms"], workgroup0_ticks=ticks, workgroup0_cycles=cycles, ghz=ghz,
                                         device_max_ghz=max_khz / 1e6))
        assert ticks >= 100, f"workgroup 0 ran {ticks} ticks: one tick is not below 1 %"
        assert math.isfinite(ghz) and ghz > 0.0
        assert abs(ghz - cycles / ticks * 0.1) <= 1e-6 * ghz
        if max_khz > 0:
            assert ghz <= max_khz / 1e6 * (ticks + 1) / ticks, f"{ghz} GHz above the device's {max_khz / 1e6} GHz"
        # a session of the RefineNet chain: slots 1..10 now hold probes
        _session(L)
        _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), p, None, None, ws_r.data_ptr(), ws_r.numel(),
                                  corners.data_ptr(), None, None, None), "dcx_refiner_forward")
        torch.cuda.synchronize()
        assert all(c > 0.0 for c in _clocks(L, 12)[1:11])
        # second session: only a non-conv bracket, in slot 0
        _session(L)
        _ok(L.dcx_detector_front(det.handle, tiny.frames.data_ptr(), H * WD, WD, 0, 1, H, WD, front.data_ptr(), front.numel(), None),
            "dcx_detector_front")
        torch.cuda.synchronize()
        recs = _fetch(L)
        assert [(r["id"], r["n"], r["flops"]) for r in recs] == [(IC.PROF_CONV1A, 1, 0.0)] and recs[0]["ms"] > 0
        assert _clocks(L, 1) == [0.0], "a record that wrote no probes reports an earlier session's clock"
        assert not _words(L, 0).any() and not _words(L, 5).any()
        # third: conv launches whose workgroup 0 has no item
        _session(L)
        _ok(L.dcx_refiner_forward(rf.handle, patches_d.data_ptr(), p, zero_d.data_ptr(), None, ws_r.data_ptr(), ws_r.numel(),
                                  corners.data_ptr(), None, None, None), "dcx_refiner_forward (count 0)")
        torch.cuda.synchronize()
        recs = _fetch(L)
        assert len(recs) == 12 and all(r["limited"] == 1 for r in recs)
        assert _clocks(L, 12) == [0.0] * 12, "conv launches without work report an earlier session's clocks"


# --------------------------------------------------------------------------- e. past the last slot

def test_records_past_the_last_probe_slot(dev, L, table):
    """1,030 launches of the smallest conv layer in one session: every record is complete, the first 1,024 own a slot, the later
    ones report clock 0 and write nowhere: the last slot's and the first slot's words are the same before the 1,025th launch and
    after the 1,030th."""
    names = _names(L)
    conv = RawConv(L, dev, SMALLEST)
    kid = names.index(_case_pick(L, SMALLEST))
    total = IC.CLK_SLOTS + 6
    with hooks(L):
        _session(L)
        for _ in range(IC.CLK_SLOTS):
            conv.launch()
        first, last = _words(L, 0), _words(L, IC.CLK_SLOTS - 1)
        _check_own_probes(first, "slot 0")
        _check_own_probes(last, "slot 1023")
        for _ in range(total - IC.CLK_SLOTS):
            conv.launch()
        assert L.dcx_profile_count() == total
        recs = _fetch(L)
        assert all((r["id"], r["n"], r["limited"], r["flops"]) == (kid, SMALLEST[1], 0, float(conv.flops)) and r["ms"] > 0 for r in recs)
        clocks = _clocks(L, total)
        assert clocks[IC.CLK_SLOTS:] == [0.0] * (total - IC.CLK_SLOTS)
        assert all(math.isfinite(c) and c >= 0.0 for c in clocks[:IC.CLK_SLOTS])
        assert np.array_equal(_words(L, 0), first) and np.array_equal(_words(L, IC.CLK_SLOTS - 1), last)
        words = (C.c_ulonglong * IC.CLK_WORDS)()
        assert L.dcx_profile_probe_words(IC.CLK_SLOTS, words) == IC.E_ARG and L.dcx_profile_probe_words(-1, words) == IC.E_ARG
        assert L.dcx_profile_probe_words(0, None) == IC.E_ARG
        _report("past_the_last_slot", dict(records=total, clocked=sum(c > 0 for c in clocks)))


# --------------------------------------------------------------------------- f. stage timers

EVENT_TICK_MS = 1e-3      # hipEventElapsedTime: "Time is computed in ms, with a resolution of approximately 1 us" (hip_runtime_api.h)


def test_stage_timers(dev, L, tiny):
    """One eager dcx_infer_batch with dcx_set_timing(1): four values >= 0, the total >= each part and <= the host's wall time
    around the call, and the three parts add up to the total within three ticks of the event timer -- 1 us, the resolution the HIP
    runtime's own header states for hipEventElapsedTime (the parts share their inner events, so nothing else can separate them)."""
    b = 3
    t4 = (C.c_float * 4)()
    with hooks(L):
        _ok(L.dcx_set_timing(1), "dcx_set_timing")
        assert L.dcx_get_timing() == 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed = tiny.run(b, sync=False)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        _ok(L.dcx_last_timings(t4), "dcx_last_timings")
        t = [float(v) for v in t4]
        _report("stage_timers_3x64x96", dict(detector_ms=t[0], tail_ms=t[1], refinenet_ms=t[2], total_ms=t[3], host_wall_ms=wall_ms))
        assert all(v >= 0.0 for v in t) and all(t[3] >= v for v in t[:3])
        assert abs(t[0] + t[1] + t[2] - t[3]) <= 3 * EVENT_TICK_MS
        assert t[3] <= wall_ms
        assert _same_results(tiny.unpack(packed, b), tiny.plain[b])


def test_profiling_switches_graphs_off(dev, L, tiny, golden_tiny):
    """As with timing (test_graph_cache_threads_modes_and_lifetime): while profiling is on the one-frame path launches eagerly --
    the fixture's corners, and no graph captured."""
    from deepcharuco_amd import graph as G
    from deepcharuco_amd.inference import infer_image
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    dc = lModel(dcModel(golden_tiny.n_ids, golden_tiny.sd_dc, dev))
    rn = lRefineNet(RefineNet(golden_tiny.sd_rn, dev))
    live = len(G._live)
    with hooks(L):
        _session(L)
        assert not G.graphs_usable()
        kp, _ = infer_image(golden_tiny.bgr, golden_tiny.n_ids, dc, rn, device="cuda")
        assert kp.shape == golden_tiny.fx["final_rn"].shape and np.array_equal(kp, golden_tiny.fx["final_rn"])
        assert not getattr(dc.model, "_graph_cache", None) and len(G._live) == live
        assert L.dcx_profile_count() == len(IC.expected_infer_batch(1, H, WD, KMAX))
    assert G.graphs_usable()


# --------------------------------------------------------------------------- XCD shares (they live in a device table)

def test_xcd_shares_round_trip(dev, L):
    """dcx_set_xcd_weights -> dcx_get_xcd_weights: eight values of mean 1.0 in the proportions set (each share is one division in
    double rounded to float32 and one exact multiplication by 8: 2^-23 covers two such values' ratio), NULL gives eight exact
    ones, a refused set leaves the previous shares in place."""
    rel = [1.0, 1.1, 0.9, 1.05, 0.95, 1.2, 0.8, 1.0]
    got, again = (C.c_float * 8)(), (C.c_float * 8)()
    with hooks(L):
        sent = (C.c_float * 8)(*[3.7 * v for v in rel])
        _ok(L.dcx_set_xcd_weights(sent), "dcx_set_xcd_weights")
        _ok(L.dcx_get_xcd_weights(got), "dcx_get_xcd_weights")
        s = sum(float(v) for v in sent)
        assert abs(sum(got) / 8 - 1.0) <= 8 * 2.0 ** -24
        assert all(abs(float(g_) - 8.0 * float(v) / s) <= 2.0 ** -23 * float(g_) for g_, v in zip(got, sent))
        for bad in ([2.0] + [1.0] * 7, [1.0] * 7 + [0.5], [0.0] + [1.0] * 7, [-1.0] + [1.0] * 7):
            assert L.dcx_set_xcd_weights((C.c_float * 8)(*bad)) == IC.E_ARG, bad
            _ok(L.dcx_get_xcd_weights(again), "dcx_get_xcd_weights")
            assert list(again) == list(got), f"a refused set changed the shares: {bad}"
        _ok(L.dcx_set_xcd_weights(None), "dcx_set_xcd_weights(NULL)")
        _ok(L.dcx_get_xcd_weights(got), "dcx_get_xcd_weights")
        assert list(got) == [1.0] * 8
    _ok(L.dcx_get_xcd_weights(got), "dcx_get_xcd_weights")
    assert list(got) == [1.0] * 8


# --------------------------------------------------------------------------- g. dcx_stream_synchronize

@pytest.mark.parametrize("which", ["default", "side"])
def test_stream_synchronize_waits_for_the_stream(dev, L, tiny, which):
    """What graph.py's one-frame path relies on before it reads the pinned result: after dcx_stream_synchronize(raw handle) an
    event recorded behind ~20 queued pipeline calls has completed, and the last call's result is the separately synchronised one."""
    b = 3
    stream = torch.cuda.default_stream(dev) if which == "default" else torch.cuda.Stream(dev)
    with hooks(L):
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            try:
                raw = torch._C._cuda_getCurrentRawStream(dev.index)       # what graph._sync_current_stream passes
            except AttributeError:
                raw = torch.cuda.current_stream(dev).cuda_stream
            assert raw == stream.cuda_stream and (raw == 0) == (which == "default")
            for _ in range(20):
                packed = tiny.run(b, sync=False)
            ev = torch.cuda.Event()
            ev.record(stream)
            rc = L.dcx_stream_synchronize(raw)
            done = ev.query()
        assert rc == 0
        assert done, "dcx_stream_synchronize returned before the stream's work had finished"
        assert _same_results(tiny.unpack(packed, b), tiny.plain[b])


# --------------------------------------------------------------------------- last: the process is as the file found it

def test_hooks_are_back_to_their_defaults(dev, L):
    from deepcharuco_amd import graph as G
    w = (C.c_float * 8)()
    assert L.dcx_profile_enabled() == 0 and L.dcx_get_timing() == 0
    _ok(L.dcx_get_xcd_weights(w), "dcx_get_xcd_weights")
    assert list(w) == [1.0] * 8
    assert "DCX_FORCE_CFG" not in os.environ
    assert G.graphs_usable()
