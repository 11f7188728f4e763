"""The profile and timing hooks of the C ABI, as far as they can be held to their header without a GPU: the expected-record table of
tests/instrument_cases.py against the project's recorded 26.816 GFLOP per frame, argument checks, idle behaviour, the kernel-name
table.  What needs a device -- the XCD shares' round trip among it: dcx_set_xcd_weights / dcx_get_xcd_weights write a device table
-- is in tests/test_gpu_instrument.py.  Every test leaves the process-global hooks as it found them (profile off, filter -1,
sample 1, timing off)."""
import ctypes as C

import pytest

import instrument_cases as IC


@pytest.fixture(scope="module")
def L():
    from deepcharuco_amd import _lib
    return _lib.lib()


def _restore(L):
    L.dcx_profile_enable(0)
    L.dcx_profile_filter(-1)
    L.dcx_profile_sample(1)
    L.dcx_set_timing(0)


# --------------------------------------------------------------------------- the expected records

def test_layer_table_reproduces_the_recorded_gflop_per_frame():
    """DESIGN.md 5 states 26.816 GFLOP for a 320x240 frame with 16 corners; bench.py divides every end-to-end fraction by it.  The
    oracle's own conv2d calls, with Ho x Wo = each convolution's own output (before a pooling, after an up-sampling), sum to it."""
    assert round(IC.gflop_per_frame(240, 320, 16), 3) == IC.DESIGN_GFLOP_PER_FRAME
    det = {l.name: l for l in IC.trace_layers("detector", 240, 320)}
    ref = {l.name: l for l in IC.trace_layers("refinenet", 24, 24)}
    # the conventions the figure rests on, layer by layer where they matter
    assert (det["conv1b"].pool, det["conv1b"].ho, det["conv1b"].wo) == (1, 240, 320)          # pooled: counted at its own 240x320
    assert (det["conv2a"].hin, det["conv2a"].win) == (120, 160)
    assert (ref["conv2b"].pool, ref["conv2b"].ho, ref["conv3a"].hin) == (1, 16, 8)
    assert (ref["conv4a"].ups, ref["conv4a"].ho) == (1, 16) and (ref["conv5a"].ups, ref["conv5a"].ho) == (1, 32)
    assert (ref["convPa"].ups, ref["convPa"].ho, ref["convPa"].wo) == (1, 64, 64)              # up-sampled: counted at 64x64
    assert [l.name for l in det.values() if l.ups] == [] and [l.name for l in det.values() if l.pool] == ["conv1b", "conv2b", "conv3b"]
    assert sum(l.flops for l in det.values()) == 2 * 6_439_526_400 and sum(l.flops for l in ref.values()) == 2 * 435_536_128


def test_expected_records_of_a_320x240_batch():
    """The records of dcx_infer_batch for 32 frames of 320x240 and a pool of 32 x 64: launch order, fused launches, brackets, and the
    flops the records carry -- everything but the two conv1a, the detector's 1x1 heads and RefineNet's convPb, which run inside the
    flops-0 brackets (100, 102, 101) or a head's epilogue: 0.156 of the 26.816 GFLOP, as the header says."""
    b, pool = 32, 32 * 64
    recs = IC.expected_infer_batch(b, 240, 320, pool)
    assert [r.kernel_id for r in recs] == [100] + [None] * 8 + [102, 101] + [None] * 10 + [103]
    assert [r.n for r in recs] == [b] * 10 + [pool] * 12
    assert [r.limited for r in recs] == [0] * 10 + [1] * 12
    assert all((r.flops == 0) == (r.kernel_id is not None) for r in recs)
    assert recs[8].layers == ("convPa", "convDa") and recs[8].pick[4] == 512 and recs[8].flops == 2 * 2 * 256 * 128 * 9 * 30 * 40
    assert recs[-2].layers == ("convPa", "convPb") and recs[-2].pick[0] == IC.HEAT_PICK_N and recs[-2].pick[7] == IC.EPI_HEAT
    assert all(r.pick[0] == 512 for r in recs[11:20])                   # tiles for the expected 16 corners per frame, not for the pool
    per_frame = sum(r.flops for r in recs[:10]) + 16 * sum(r.flops for r in recs[10:])
    missing = IC.unrecorded_flops(240, 320, 16)
    assert per_frame + missing == round(IC.gflop_per_frame(240, 320, 16) * 1e9)
    assert round(missing / 1e9, 3) == 0.156
    # the staged chain: the heads become two 1x1 launches on the flattened cell list, the refiner's limit is the caller's choice
    staged = IC.expected_detector_forward(b, 240, 320)
    assert [r.kernel_id for r in staged] == [100] + [None] * 10 and staged[:9] == recs[:9]
    assert [r.pick[1:8] for r in staged[9:]] == [(256, 1, 1200, 65, 1, 0, IC.EPI_RAW), (256, 1, 1200, 17, 1, 0, IC.EPI_RAW)]
    assert [r.flops for r in staged[9:]] == [2 * 65 * 256 * 1200, 2 * 17 * 256 * 1200]
    for with_total in (False, True):
        rf = IC.expected_refiner_forward(40, with_total)
        assert [r.kernel_id for r in rf] == [101] + [None] * 10 + [103]
        assert {r.limited for r in rf} == {int(with_total)} and {r.n for r in rf} == {40}
        assert [r.flops for r in rf] == [r.flops for r in recs[10:]]


def test_expected_kernels_exist_for_every_record(L):
    """Every expected convolution record names a shape the library's cost model has an instantiation for (host call, no GPU)."""
    for recs in (IC.expected_infer_batch(3, 64, 96, 192), IC.expected_detector_forward(1, 64, 96), IC.expected_refiner_forward(18, True),
                 IC.expected_infer_batch(32, 240, 320, 2048)):
        for r in recs:
            if r.pick is not None:
                assert L.dcx_conv_pick_name_ups(*r.pick).decode().startswith("dcx_conv_"), r


# --------------------------------------------------------------------------- argument checks and idle behaviour

def test_null_arguments_are_refused(L):
    n = 4
    ids, nimg, lim = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    fl, ms, ghz = (C.c_double * n)(), (C.c_float * n)(), (C.c_float * n)()
    full = [ids, nimg, lim, fl, ms]
    try:
        for i in range(5):
            args = list(full)
            args[i] = None
            assert L.dcx_profile_fetch(*args, n) == IC.E_ARG, f"dcx_profile_fetch with argument {i} NULL"
        assert L.dcx_profile_clocks(None, n) == IC.E_ARG
        words = (C.c_ulonglong * IC.CLK_WORDS)()
        assert L.dcx_profile_probe_words(0, None) == IC.E_ARG
        for record in (-1, IC.CLK_SLOTS, IC.CLK_SLOTS + 1, -(2 ** 31), 2 ** 31 - 1):
            assert L.dcx_profile_probe_words(record, words) == IC.E_ARG, record
        assert L.dcx_last_timings(None) == IC.E_ARG
        t4 = (C.c_float * 4)(-7.0, -7.0, -7.0, -7.0)
        L.dcx_set_timing(1)                       # switched on, but no call has been timed in this process (there is no device)
        assert L.dcx_last_timings(t4) == IC.E_ARG and list(t4) == [-7.0] * 4
    finally:
        _restore(L)


def test_idle_hooks_follow_their_setters(L):
    n = 4
    ids, nimg, lim = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    fl, ms, ghz = (C.c_double * n)(), (C.c_float * n)(), (C.c_float * n)()
    try:
        assert L.dcx_profile_enabled() == 0 and L.dcx_get_timing() == 0
        for every in (0, -3, 1):                  # 0 and negative values behave as 1: nothing but a 0 return to see without a launch
            assert L.dcx_profile_sample(every) == 0
        assert L.dcx_profile_enable(1) == 0
        assert L.dcx_profile_enabled() == 1 and L.dcx_profile_count() == 0
        assert L.dcx_profile_fetch(ids, nimg, lim, fl, ms, n) == 0 and L.dcx_profile_clocks(ghz, n) == 0
        assert L.dcx_profile_enable(7) == 0 and L.dcx_profile_enabled() == 1      # any non-zero value is "on"
        assert L.dcx_profile_enable(0) == 0 and L.dcx_profile_enabled() == 0 and L.dcx_profile_count() == 0
        for v, want in ((1, 1), (0, 0), (5, 1), (0, 0)):
            assert L.dcx_set_timing(v) == 0 and L.dcx_get_timing() == want
        assert L.dcx_profile_enabled() == 0       # the two switches are independent
    finally:
        _restore(L)
    assert L.dcx_profile_enabled() == 0 and L.dcx_get_timing() == 0


def test_kernel_names(L):
    names = []
    while len(names) < 99 and L.dcx_profile_kernel_name(len(names)) != b"?":
        names.append(L.dcx_profile_kernel_name(len(names)).decode())
    table = len(names)
    assert 14 <= table < 99
    named = names + [L.dcx_profile_kernel_name(i).decode() for i in IC.BRACKET_IDS]
    assert all(nm and nm != "?" for nm in named) and len(set(named)) == len(named)
    for i in (-1, table, 99, 104, 2 ** 31 - 1, -(2 ** 31)):
        assert L.dcx_profile_kernel_name(i) == b"?", i
    # what the other tests look up by name: every instantiation the cost model can answer with is in the table
    for recs in (IC.expected_infer_batch(3, 64, 96, 192), IC.expected_infer_batch(32, 240, 320, 2048)):
        assert all(L.dcx_conv_pick_name_ups(*r.pick).decode() in names for r in recs if r.pick)


def test_xcd_shares_refused_without_touching_a_device(L):
    """The refusals of dcx_set_xcd_weights are decided on the host, before any device call: a share more than 25 % from equal, a
    zero, a negative value, a NaN.  (The round trip is a GPU test.)"""
    rest = [1.0] * 7
    # first share = 8 w0 / sum(w): 2.0 -> 1.78, 1.4 -> 1.33, 0.5 -> 0.53 of an equal one
    for w0 in (2.0, 1.4, 0.5, 0.0, -1.0, float("nan"), float("inf")):
        for at in (0, 7):
            bad = rest[:at] + [w0] + rest[at:]
            assert L.dcx_set_xcd_weights((C.c_float * 8)(*bad)) == IC.E_ARG, bad
    assert L.dcx_get_xcd_weights(None) == IC.E_ARG
