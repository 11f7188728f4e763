"""The stereo kernels (csrc/dcx_sgm.hip, csrc/dcx_speckle.hip) at the launch limits that their own constants state, as ACCEPTED
shapes: frames 4096 wide, lines of 2100 pixels, one frame more than a chunk may hold (16384 for the matcher, 32768 for the filter),
``min_disparity`` at both ends of the int16 range, a frame stride of 0 and a workspace that holds anything; and the refusals of
the C entry points themselves, which the Python wrappers otherwise keep from being reached.  Every matcher and filter result is
compared bit for bit with ``sgm_host`` / ``filter_speckles_host`` (tests/test_disparity_limits_host.py shows that none of the
scenes is degenerate), every refusal with the code that include/deepcharuco_amd.h states."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import disparity_limit_cases as lc
from deepcharuco_amd import _lib, disparity as dp

pytestmark = pytest.mark.gpu

E_ARG, E_SHAPE, E_WS = -1, -2, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _gpu(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)                              # (a copy: the scenes are read-only)


@functools.lru_cache(maxsize=None)
def _host(scene, *args, **kw):
    """sgm_host on a scene of the cases module, computed once per parameter set."""
    left, right = getattr(lc, scene)(*args)[:2]
    want = dp.sgm_host(left, right, **kw)
    want.setflags(write=False)
    return want


def _same(got, want, what=None):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    differ = got != want
    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:5].tolist(), got[differ][:5], want[differ][:5])


def _agree(dev, scene, *args, **kw):
    left, right = getattr(lc, scene)(*args)[:2]
    want = _host(scene, *args, **kw)
    got = dp.sgm_device(_gpu(dev, left), _gpu(dev, right), **kw)
    assert got.is_contiguous()
    _same(got, want, (scene, args, kw))
    return want


# ------------------------------------------------------------------------------------------------ B1, B2: width and line length

@pytest.mark.parametrize("h,D,paths", [(3, 64, 8), (3, 64, 4), (2, 256, 8), (1, 64, 8)])
def test_frames_of_the_greatest_width(dev, h, D, paths):
    """W = kMaxWidth: the select kernel's 32 KB of dynamic LDS, a row pass of 4096 steps, 64 census workgroups to a row."""
    out = _agree(dev, "wide_pair", h, num_disparities=D, paths=paths)
    assert (out == -16).any() and (out != -16).mean() > 0.99


@pytest.mark.parametrize("w", [3, 1])
def test_lines_of_2100_pixels(dev, w):
    """A column pass of 2100 steps; at W = 3 a start-column wave of the diagonal kernels wraps 700 times, at W = 1 at every step."""
    out = _agree(dev, "tall_pair", w, paths=8)
    assert (out == -16).any() and (out != -16).any()


# ------------------------------------------------------------------------------------------------ B3, B4: the chunk caps

@pytest.mark.parametrize("speckle", [{}, lc.SMALL_SPECKLE], ids=["plain", "filtered"])
def test_one_frame_more_than_the_matcher_s_chunk(dev, speckle):
    """16385 frames with the whole batch's workspace: the cap of 16384 frames decides the chunks (16384 and 1), not the workspace.
    The frames repeat with period 7 and 16384 mod 7 = 4, so a tail that read or wrote frame 0's place shows.  With the filter on,
    that runs across the same batch in the matcher's workspace (one chunk: its cap is 32768)."""
    B = lc.SGM_CHUNK_CAP + 1
    left, right = (lc.tiled(a, B) for a in lc.sgm_period())
    want = lc.tiled(_host("sgm_period", paths=8, **speckle), B)
    h, w = lc.SMALL
    nbytes = dp.sgm_workspace_bytes(B, h, w, 64)
    assert nbytes == B * h * w * (16 + 2 * 64)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.full((B, h, w), 77, dtype=torch.int16, device=dev)
    assert dp.sgm_device(_gpu(dev, left), _gpu(dev, right), out=out, workspace=ws, paths=8, **speckle) is out
    _same(out, want)


def test_one_frame_more_than_the_filter_s_chunk(dev):
    """32769 frames, period 11 (32768 mod 11 = 10), the whole batch's workspace: chunks of 32768 frames and of one."""
    B = lc.SPECKLE_CHUNK_CAP + 1
    disp = lc.tiled(lc.speckle_period(), B)
    want = lc.tiled(dp.filter_speckles_host(lc.speckle_period(), *lc.SMALL_FILTER), B)
    h, w = lc.SMALL
    nbytes = dp.filter_speckles_workspace_bytes(B, h, w)
    assert nbytes == B * h * w * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    src = _gpu(dev, disp)
    out = torch.full((B, h, w), 77, dtype=torch.int16, device=dev)
    assert dp.filter_speckles_device(src, *lc.SMALL_FILTER, out=out, workspace=ws) is out
    _same(out, want)
    _same(src, disp)                                                          # out of place: the input is left alone


# ------------------------------------------------------------------------------------------------ B5: the int16 range's ends

@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("end", ["low", "high"])
def test_min_disparity_at_the_ends_of_the_int16_range(dev, end, paths):
    """m = -2047: the invalid value is -32768 and a true match at d* = 0 gives -32752; m + D = 2047: a true match at d* = D - 1 gives
    32736, the largest value the matcher can store."""
    e = lc.EDGES[end]
    m, D, true = e["min_disparity"], e["num_disparities"], e["true"]
    out = _agree(dev, "edge_scene", end, min_disparity=m, num_disparities=D, paths=paths)
    match = lc.edge_scene(end)[2]
    assert (out[:, match] == 16 * true).mean() >= 0.9 and (out[:, ~match] == 16 * (m - 1)).mean() >= 0.95
    assert {16 * true, 16 * (m - 1)} == ({-32752, -32768} if end == "low" else {32736, 28640})


def test_min_disparity_with_no_candidate_on_the_frame(dev):
    assert (_agree(dev, "narrow_pair", min_disparity=-2047, paths=8) == -32768).all()


# ------------------------------------------------------------------------------------------------ B6: a frame stride of 0

def test_one_left_frame_broadcast_over_three_right_frames(dev):
    left, right = lc.broadcast_batch()
    want = dp.sgm_host(np.ascontiguousarray(np.broadcast_to(left, right.shape)), right)
    tl = _gpu(dev, left)[None].expand(3, -1, -1)
    assert tl.stride(0) == 0
    _same(dp.sgm_device(tl, _gpu(dev, right)), want)
    assert all((want[a] != want[b]).any() for a, b in ((0, 1), (1, 2), (0, 2)))


# ------------------------------------------------------------------------------------------------ B7: whatever the workspace held

def test_the_matcher_does_not_read_what_the_workspace_held(dev):
    """Eight paths and the filter, one workspace tensor: zeroed, all ones, and as a call on another shape left it."""
    kw = dict(min_disparity=-3, paths=8, **lc.SPECKLE)
    want = _host("small_batch", 0, **kw)
    left, right = (_gpu(dev, a) for a in lc.small_batch(0))
    ws = torch.empty(dp.sgm_workspace_bytes(3, 11, 70, 64), dtype=torch.uint8, device=dev)
    other = tuple(_gpu(dev, a) for a in lc.broadcast_batch())
    results = []
    for prepare in (lambda: ws.fill_(0x00), lambda: ws.fill_(0xFF),
                    lambda: dp.sgm_device(other[0], other[1][0], num_disparities=128, workspace=ws, **lc.SPECKLE)):
        prepare()
        out = torch.full((3, 11, 70), 77, dtype=torch.int16, device=dev)
        dp.sgm_device(left, right, out=out, workspace=ws, **kw)
        _same(out, want)
        results.append(out)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])


def test_the_filter_does_not_read_what_the_workspace_held(dev):
    disp = lc.speckle_batch(7)
    want = dp.filter_speckles_host(disp, *lc.FILTER)
    src = _gpu(dev, disp)
    ws = torch.empty(dp.filter_speckles_workspace_bytes(3, 40, 70), dtype=torch.uint8, device=dev)
    other = _gpu(dev, lc.speckle_batch(8)[0, :33, :65])
    results = []
    for prepare in (lambda: ws.fill_(0x00), lambda: ws.fill_(0xFF), lambda: dp.filter_speckles_device(other, lc.NV, 40, 40, workspace=ws)):
        prepare()
        out = torch.full_like(src, 77)
        dp.filter_speckles_device(src, *lc.FILTER, out=out, workspace=ws)
        _same(out, want)
        results.append(out)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])


# ------------------------------------------------------------------------------------------------ C: the C entry points' own refusals

H, W = 9, 70
SGM_ARGS = ("d_left", "frame_stride_l", "pitch_l", "d_right", "frame_stride_r", "pitch_r", "batch", "height", "width", "min_disparity",
            "num_disparities", "p1", "p2", "uniqueness", "lr_max_diff", "paths", "d_disp16", "d_workspace", "workspace_bytes", "stream")


def test_the_matcher_s_c_entry_point_refuses(dev):
    """One bad argument at a time: the code, and nothing launched (the output keeps its fill)."""
    lib = _lib.lib()
    left, right = (_gpu(dev, a[0, :H]) for a in lc.small_batch(0))
    one = H * W * (16 + 2 * 64)
    assert lib.dcx_sgm_workspace_bytes(1, H, W, 64) == one and lib.dcx_sgm_workspace_bytes(3, H, W, 256) == 3 * H * W * (16 + 2 * 256)
    assert lib.dcx_sgm_workspace_bytes(16385, 2, 4096, 128) == 16385 * 2 * 4096 * (16 + 2 * 128) and lib.dcx_sgm_workspace_bytes(1, 32768, 1, 64)
    for shape in ((0, H, W, 64), (1, 0, W, 64), (1, H, 0, 64), (1, H, 4097, 64), (1, 32769, W, 64), (1, H, W, 32), (1, H, W, 96), (-1, H, W, 64)):
        assert lib.dcx_sgm_workspace_bytes(*shape) == 0, shape
    ws = torch.empty(one + 8, dtype=torch.uint8, device=dev)
    out = torch.full((H, W + 1), 77, dtype=torch.int16, device=dev)         # (a spare column: the odd address stays inside it)
    good = dict(d_left=left.data_ptr(), frame_stride_l=0, pitch_l=W, d_right=right.data_ptr(), frame_stride_r=0, pitch_r=W, batch=1, height=H,
                width=W, min_disparity=0, num_disparities=64, p1=7, p2=86, uniqueness=10, lr_max_diff=1, paths=8, d_disp16=out.data_ptr(),
                d_workspace=ws.data_ptr(), workspace_bytes=one, stream=_lib.current_stream())
    assert tuple(good) == SGM_ARGS

    def call(**bad):
        return lib.dcx_sgm_u8_paths(*dict(good, **bad).values())

    arg = [dict(d_left=None), dict(d_right=None), dict(d_disp16=None), dict(d_workspace=None), dict(d_disp16=out.data_ptr() + 1),
           dict(d_workspace=ws.data_ptr() + 4), dict(frame_stride_l=-1), dict(frame_stride_r=-1), dict(p1=-1), dict(p1=87), dict(p2=256),
           dict(uniqueness=-1), dict(uniqueness=100), dict(min_disparity=-2048), dict(min_disparity=2048 - 64),
           dict(min_disparity=2048 - 256, num_disparities=256)]
    shape = [dict(batch=0), dict(height=0), dict(width=0), dict(width=4097, pitch_l=4097, pitch_r=4097), dict(height=32769),
             dict(num_disparities=32), dict(num_disparities=96), dict(pitch_l=W - 1), dict(pitch_r=W - 1)]
    for bad in arg:
        assert call(**bad) == E_ARG, bad
    for bad in shape:
        assert call(**bad) == E_SHAPE, bad
    assert call(workspace_bytes=one - 1) == E_WS and call(workspace_bytes=0) == E_WS
    torch.cuda.synchronize()
    assert (out == 77).all()                                                  # nothing was launched


def test_the_matcher_s_c_entry_point_accepts_the_limits_it_states(dev):
    """Exactly one frame's bytes for a batch of two (chunks of one frame), m = -2047 and m + D = 2047 accepted."""
    lib = _lib.lib()
    lr = lc.small_batch(0)
    left, right = (_gpu(dev, a[:2]) for a in lr)
    h, w = left.shape[1:]
    one = lib.dcx_sgm_workspace_bytes(1, h, w, 64)
    ws = torch.full((one,), 0xFF, dtype=torch.uint8, device=dev)
    for m in (0, -2047, 2047 - 64):
        out = torch.full((2, h, w), 77, dtype=torch.int16, device=dev)
        assert lib.dcx_sgm_u8_paths(left.data_ptr(), h * w, w, right.data_ptr(), h * w, w, 2, h, w, m, 64, 7, 86, 10, 1, 8, out.data_ptr(),
                                    ws.data_ptr(), one, _lib.current_stream()) == 0
        _same(out, dp.sgm_host(lr[0][:2], lr[1][:2], min_disparity=m, paths=8), m)


def test_the_points_c_entry_point_refuses(dev):
    lib = _lib.lib()
    disp = torch.zeros((H, W + 1), dtype=torch.int16, device=dev)
    xyz = torch.full((H, W + 1, 3), 77.0, dtype=torch.float32, device=dev)
    Q = np.eye(4) + np.arange(16).reshape(4, 4) / 16.0

    def q(values):
        return (ctypes.c_double * 16)(*np.asarray(values, np.float64).ravel().tolist())

    good = dict(d_disp16=disp.data_ptr(), batch=1, height=H, width=W, min_disparity=0, h_Q16=q(Q), d_xyz=xyz.data_ptr(),
                stream=_lib.current_stream())

    def call(**bad):
        return lib.dcx_disparity_to_points(*dict(good, **bad).values())

    bad_q = []
    for value, at in ((np.nan, 0), (np.inf, 5), (-np.inf, 15), (np.nan, 10)):
        bad = Q.copy()
        bad.ravel()[at] = value
        bad_q.append(dict(h_Q16=q(bad)))
    for bad in [dict(d_disp16=None), dict(h_Q16=None), dict(d_xyz=None), dict(d_disp16=disp.data_ptr() + 1), dict(d_xyz=xyz.data_ptr() + 2),
                dict(d_xyz=xyz.data_ptr() + 1)] + bad_q:
        assert call(**bad) == E_ARG, bad
    for bad in (dict(batch=0), dict(height=0), dict(width=0), dict(batch=-1)):
        assert call(**bad) == E_SHAPE, bad
    torch.cuda.synchronize()
    assert (xyz == 77.0).all()                                                # nothing was launched
    assert call() == 0                                                        # (the same arguments with nothing wrong)
    torch.cuda.synchronize()
    want = dp.disparity_to_points_host(np.zeros((H, W), np.int16), Q)
    assert np.isnan(want).all() and torch.isnan(xyz.reshape(-1)[:H * W * 3]).all()     # d = 0 everywhere: the host's NaN
