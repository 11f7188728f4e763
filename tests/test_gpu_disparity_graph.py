"""``sgm_device``, ``filter_speckles_device`` and ``disparity_to_points_device`` replayed from a captured graph, as a per-frame
stereo loop would use them: a replay reads what its input buffers hold NOW, gives the same bits whatever the workspace held, and
allocates nothing.  Every graph is linear, captured on one stream after a warm-up call on a side stream, with every tensor
preallocated.  After each replay the buffers are compared with ``sgm_host`` / ``filter_speckles_host`` bit for bit and the points
with ``disparity_to_points_host`` as tests/test_gpu_disparity.py does (equal NaN positions, at most 1 ulp of the host's float32);
tests/test_disparity_limits_host.py shows that the swapped-in inputs change the answer."""
import numpy as np
import pytest
import torch

import disparity_limit_cases as lc
import rectify_exact as rx
import stereo_exact as sx
from deepcharuco_amd import disparity as dp, rectify as rc
from test_gpu_disparity import _ulps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _gpu(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)                              # (a copy: the scenes are read-only)


def _capture(enqueue):
    """A warm-up call on a side stream, then ``enqueue`` captured into one linear graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    return g


def _replayed(g, *tensors):
    g.replay()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _strided(dev, shape, pitch, spare, offset):
    """An uninitialised-looking (all 255) buffer and a (B, h, w) view of it: rows at ``pitch``, ``spare`` bytes between frames, the
    first frame ``offset`` bytes in."""
    B, h, w = shape
    stride = h * pitch + spare
    buf = torch.full((offset + B * stride,), 255, dtype=torch.uint8, device=dev)
    return torch.as_strided(buf, shape, (stride, pitch, 1), offset)


def _replay_sequence(dev, g, inputs, swapped, out, ws, want_first, want_swapped):
    """Replay; overwrite the inputs outside the graph, poison the output and the workspace, replay; zero the workspace and replay
    twice more.  Nothing is allocated from before the first replay to after the last."""
    assert not np.array_equal(want_first, want_swapped)
    out.fill_(77)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    got, = _replayed(g, out)
    assert np.array_equal(got, want_first)
    for t, new in zip(inputs, swapped):
        t.copy_(new)
    out.fill_(77)
    ws.fill_(0xFF)
    got, = _replayed(g, out)
    assert np.array_equal(got, want_swapped)                                  # the replay read the new frames
    ws.fill_(0x00)
    again = [_replayed(g, out)[0] for _ in range(2)]
    assert np.array_equal(again[0], again[1]) and np.array_equal(again[0], want_swapped)
    assert torch.cuda.memory_allocated(dev) == before


@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("paths", [4, 8])
def test_the_matcher_replays_from_a_graph(dev, paths, window):
    """Three frames 11 x 70 through a workspace of one frame and a half (two chunks in the capture), the left frames at pitch 80
    with 33 spare bytes between them from an odd address, the right ones at pitch 75."""
    kw = dict(min_disparity=-3, num_disparities=64, paths=paths, speckle_window_size=window, speckle_range=2)
    first, swapped = lc.small_batch(0), lc.small_batch(1)
    shape = first[0].shape
    assert shape == (3, 11, 70)
    want_first, want_swapped = dp.sgm_host(*first, **kw), dp.sgm_host(*swapped, **kw)
    left, right = _strided(dev, shape, 80, 33, 5), _strided(dev, shape, 75, 7, 0)
    assert left.data_ptr() % 2 == 1
    left.copy_(_gpu(dev, first[0]))
    right.copy_(_gpu(dev, first[1]))
    new = [_gpu(dev, a) for a in swapped]
    one = dp.sgm_workspace_bytes(1, 11, 70, 64)
    ws = torch.empty(one + one // 2, dtype=torch.uint8, device=dev)
    out = torch.empty(shape, dtype=torch.int16, device=dev)
    g = _capture(lambda: dp.sgm_device(left, right, out=out, workspace=ws, **kw))
    _replay_sequence(dev, g, (left, right), new, out, ws, want_first, want_swapped)


def test_the_filter_replays_from_a_graph(dev):
    """Three frames 40 x 70 (2 x 3 tiles each: the border kernel runs), out of place, through a one-frame workspace: three chunks."""
    first, swapped = lc.speckle_batch(7), lc.speckle_batch(8)
    want_first, want_swapped = (dp.filter_speckles_host(a, *lc.FILTER) for a in (first, swapped))
    src, new = _gpu(dev, first), _gpu(dev, swapped)
    ws = torch.empty(dp.filter_speckles_workspace_bytes(1, 40, 70), dtype=torch.uint8, device=dev)
    out = torch.empty_like(src)
    g = _capture(lambda: dp.filter_speckles_device(src, *lc.FILTER, out=out, workspace=ws))
    _replay_sequence(dev, g, (src,), (new,), out, ws, want_first, want_swapped)
    assert torch.equal(src, new)                                              # out of place: the input is left alone


def _points_agree(got, disp16, Q, m):
    want = dp.disparity_to_points_host(disp16, Q, m).astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.any() and not nan.all()
    steps = _ulps(got[~nan], want[~nan])
    print(f"{int((steps > 0).sum())} of {steps.size} coordinates differ from the host's float32, by at most {int(steps.max())} ulp")
    assert steps.max() <= 1


def test_the_matcher_the_filter_and_the_points_replay_from_one_graph(dev):
    """The two-plane scene and its two flips -> eight paths -> the filter in the matcher's workspace -> 3-D points, one graph; then
    the same frames in another order."""
    m = -3
    kw = dict(min_disparity=m, paths=8, **lc.SPECKLE)
    R, T = rx.rig_RT("verge15", "B", "C")
    Q = rc.stereo_rectify_host(*sx.cam("B"), *sx.cam("C"), rx.SIZE, R, T).Q
    first, swapped = lc.two_plane_batch(), lc.two_plane_batch(lc.REORDER)
    want_first, want_swapped = dp.sgm_host(*first, **kw), dp.sgm_host(*swapped, **kw)
    assert not np.array_equal(want_first, want_swapped)
    left, right = (_gpu(dev, a) for a in first)
    new = [_gpu(dev, a) for a in swapped]
    shape = tuple(left.shape)
    ws = torch.empty(dp.sgm_workspace_bytes(*shape, 64), dtype=torch.uint8, device=dev)
    out = torch.empty(shape, dtype=torch.int16, device=dev)
    xyz = torch.empty(shape + (3,), dtype=torch.float32, device=dev)

    def enqueue():
        dp.sgm_device(left, right, out=out, workspace=ws, **kw)
        dp.disparity_to_points_device(out, Q, m, out=xyz)
    g = _capture(enqueue)
    out.fill_(77)
    xyz.fill_(77.0)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    disp, pts = _replayed(g, out, xyz)
    assert np.array_equal(disp, want_first)
    _points_agree(pts, want_first, Q, m)
    left.copy_(new[0])
    right.copy_(new[1])
    out.fill_(77)
    xyz.fill_(77.0)
    ws.fill_(0xFF)
    disp, pts = _replayed(g, out, xyz)
    assert np.array_equal(disp, want_swapped)
    _points_agree(pts, want_swapped, Q, m)
    assert torch.cuda.memory_allocated(dev) == before
