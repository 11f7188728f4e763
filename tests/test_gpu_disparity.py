"""The device side of the stereo matcher (csrc/dcx_sgm.hip through deepcharuco_amd/disparity.py) against its numpy definition:
every case bit for bit against ``sgm_host``; the points against ``disparity_to_points_host`` cast to float32 (equal or one ulp,
equal NaN positions); repeatability, the no-allocation call and the chain from two distorted frames to 3-D points on the device."""
import numpy as np
import pytest
import torch

import disparity_cases as dc
import rectify_exact as rx
import stereo_exact as sx
from deepcharuco_amd import disparity as dp, rectify as rc

pytestmark = pytest.mark.gpu

DEFAULTS = dict(min_disparity=0, num_disparities=64, p1=7, p2=86, uniqueness=10, lr_max_diff=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _mixed_pair(seed, h, w, d_a=9, d_b=3):
    """A textured pair: disparity d_a in the upper half, d_b in the lower, a few columns of noise: valid and invalid pixels, and
    winners that change along both path directions."""
    rng = np.random.default_rng([41, seed, h, w])
    la, ra = dc.shifted_pair(rng, h, w, d_a)
    lb, rb = dc.shifted_pair(rng, h, w, d_b)
    left, right = la.copy(), ra.copy()
    left[h // 2:], right[h // 2:] = lb[h // 2:], rb[h // 2:]
    if w > 8:
        right[:, w // 2:w // 2 + 3] = rng.integers(0, 256, (h, 3), dtype=np.uint8)
    return left, right


def _agree(dev, left, right, **kw):
    """sgm_device against sgm_host on one pair or batch -> the host result."""
    par = dict(DEFAULTS, **kw)
    want = dp.sgm_host(left, right, **par)
    got = dp.sgm_device(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), **par)
    assert got.dtype == torch.int16 and tuple(got.shape) == left.shape and got.is_contiguous()
    got = got.cpu().numpy()
    differ = got != want
    assert not differ.any(), (par, left.shape, int(differ.sum()), np.argwhere(differ)[:5].tolist(), got[differ][:5], want[differ][:5])
    return want


# ------------------------------------------------------------------------------------------------ shapes

@pytest.mark.parametrize("w", [1, 63, 64, 65, 70, 131])
def test_widths_around_64_disparities(dev, w):
    out = _agree(dev, *_mixed_pair(0, 9, w))
    if w >= 70:
        assert (out != -16).any() and (out == -16).any()


@pytest.mark.parametrize("w,D", [(130, 128), (40, 256), (300, 256)])
def test_more_than_one_disparity_to_a_lane(dev, w, D):
    """D = 128 and 256: two and four disparities to a lane.  At 40 x 256 most candidates clamp to the row's first column; at 300 the
    true disparities 200 (upper half) and 70 lie in different lanes' registers."""
    left, right = _mixed_pair(1, 9, w, *((200, 70) if w == 300 else (9, 3)))
    out = _agree(dev, left, right, num_disparities=D)
    if w == 300:
        assert (out[:4, 210:] // 16 == 200).mean() > 0.5 and (out[5:, 80:] // 16 == 70).mean() > 0.5


@pytest.mark.parametrize("h", [1, 6, 7, 8, 9, 23])
def test_heights_around_the_census_window(dev, h):
    _agree(dev, *_mixed_pair(2, h, 70))


@pytest.mark.parametrize("m", [0, 5, -16])
def test_min_disparity(dev, m):
    out = _agree(dev, *_mixed_pair(3, 9, 70), min_disparity=m)
    assert (out != 16 * (m - 1)).any()
    _agree(dev, *_mixed_pair(3, 9, 70, 20, 0), min_disparity=m, num_disparities=128)


# ------------------------------------------------------------------------------------------------ parameters

@pytest.mark.parametrize("p1,p2", [(0, 0), (7, 86), (255, 255), (0, 255)])
def test_penalties(dev, p1, p2):
    _agree(dev, *_mixed_pair(4, 12, 70), p1=p1, p2=p2)


@pytest.mark.parametrize("uniqueness", [0, 10, 99])
@pytest.mark.parametrize("lr", [-1, 0, 1])
def test_uniqueness_and_left_right_check(dev, uniqueness, lr):
    _agree(dev, *_mixed_pair(5, 12, 70), uniqueness=uniqueness, lr_max_diff=lr)


# ------------------------------------------------------------------------------------------------ content

def test_noise_is_nearly_all_invalid(dev):
    rng = np.random.default_rng(6)
    left, right = rng.integers(0, 256, (2, 23, 131), dtype=np.uint8)
    out = _agree(dev, left, right)
    assert (out == -16).mean() > 0.7
    _agree(dev, left, right, uniqueness=0, lr_max_diff=-1)                   # the same S with every winner kept


@pytest.mark.parametrize("D", [64, 256])
def test_constant_frames_tie_everywhere(dev, D):
    img = np.full((9, 70), 93, np.uint8)
    assert not _agree(dev, img, img, num_disparities=D).any()
    assert (_agree(dev, img, img, num_disparities=D, min_disparity=5)[:, 5:] == 80).all()


def test_two_plane_scene(dev):
    left, right, truth, occluded, off_frame = dc.two_plane_scene()
    out = _agree(dev, np.array(left), np.array(right))
    valid = out != -16
    assert valid[~occluded & ~off_frame].mean() >= 0.965                      # (the host test's gate: the case is not degenerate)


@pytest.mark.parametrize("d", [0, 63])
def test_true_disparity_at_the_range_edges(dev, d):
    """The winner at d* = 0 and at d* = D - 1: no sub-pixel step, no d - 1 / d + 1 term in the recursion."""
    left, right = dc.shifted_pair(np.random.default_rng([7, d]), 12, 131, d)
    out = _agree(dev, left, right)
    assert (out[:, 70:] == 16 * d).mean() > 0.9


# ------------------------------------------------------------------------------------------------ batch and layout

def test_batch_chunks_strides_and_an_odd_address(dev):
    """A batch of 3 in one pass and with a workspace that holds one frame and a half (chunks of one frame); the left frames at pitch
    80 with 33 spare bytes between frames, starting 5 bytes into their buffer; the right frames at pitch 75, 7 spare bytes."""
    h, w, B = 11, 70, 3
    pairs = [_mixed_pair(10 + i, h, w, 9 + i, 2 * i) for i in range(B)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = _agree(dev, left, right)
    _agree(dev, left[:1], right[:1])
    one = dp.sgm_workspace_bytes(1, h, w, 64)
    assert dp.sgm_workspace_bytes(B, h, w, 64) == B * one == B * h * w * (16 + 2 * 64)
    ws = torch.empty(one + one // 2, dtype=torch.uint8, device=dev)
    got = dp.sgm_device(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), workspace=ws)
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError):
        dp.sgm_device(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), workspace=ws[:one - 8])

    def strided(frames, pitch, spare, offset):
        stride = h * pitch + spare
        buf = torch.full((offset + B * stride,), 255, dtype=torch.uint8, device=dev)
        view = torch.as_strided(buf, (B, h, w), (stride, pitch, 1), offset)
        view.copy_(torch.from_numpy(frames).to(dev))
        return view

    ls, rs = strided(left, 80, 33, 5), strided(right, 75, 7, 0)
    assert ls.data_ptr() % 2 == 1
    assert np.array_equal(dp.sgm_device(ls, rs).cpu().numpy(), want)
    assert np.array_equal(dp.sgm_device(ls, rs, workspace=ws).cpu().numpy(), want)
    assert np.array_equal(dp.sgm_device(ls[1], rs[1]).cpu().numpy(), want[1])


def test_two_calls_give_equal_bits_and_nothing_is_allocated(dev):
    rng = np.random.default_rng(8)
    left, right = (torch.from_numpy(a).to(dev) for a in rng.integers(0, 256, (2, 3, 23, 131), dtype=np.uint8))
    out = [torch.empty((3, 23, 131), dtype=torch.int16, device=dev) for _ in range(2)]
    ws = torch.empty(dp.sgm_workspace_bytes(3, 23, 131, 128), dtype=torch.uint8, device=dev)
    dp.sgm_device(left, right, num_disparities=128, out=out[0], workspace=ws)          # (the library is loaded by now)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert dp.sgm_device(left, right, num_disparities=128, out=out[1], workspace=ws) is out[1]
    assert torch.cuda.memory_allocated(dev) == before
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])
    assert np.array_equal(out[1].cpu().numpy(), dp.sgm_host(left.cpu().numpy(), right.cpu().numpy(), num_disparities=128))


def test_device_refusals(dev):
    a = torch.zeros((8, 8), dtype=torch.uint8, device=dev)
    for kw in (dict(num_disparities=32), dict(p1=90), dict(uniqueness=100), dict(min_disparity=-4000)):
        with pytest.raises(ValueError):
            dp.sgm_device(a, a, **kw)
    with pytest.raises(ValueError):
        dp.sgm_device(a, a.t())                                                   # rows that are not contiguous
    with pytest.raises(ValueError):
        dp.sgm_device(a, a[:, :7])
    with pytest.raises(ValueError):
        dp.sgm_device(a, a, out=torch.empty((8, 8), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        dp.sgm_workspace_bytes(1, 8, dp.MAX_DEVICE_WIDTH + 1, 64)


# ------------------------------------------------------------------------------------------------ the points

def _ulps(a, b):
    """Distance in float32 steps between finite arrays (sign-magnitude order made monotone)."""
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("shape", [(1, 1), (23, 131), (2, 23, 131)])
def test_points_device_matches_host(dev, shape):
    R, T = rx.rig_RT("verge15", "B", "C")
    r = rc.stereo_rectify_host(*sx.cam("B"), *sx.cam("C"), rx.SIZE, R, T)
    m = -16
    rng = np.random.default_rng(9)
    disp = rng.integers(16 * m, 16 * 64, shape).astype(np.int16)
    flat = disp.reshape(-1)
    flat[::7] = 16 * (m - 1)                                                 # invalid pixels
    flat[3::11] = 0                                                          # zero disparities
    flat[5::13] = -9                                                         # negative ones (valid: m = -16)
    if disp.size == 1:
        flat[0] = 300
    want = dp.disparity_to_points_host(disp, r.Q, m).astype(np.float32)
    got = dp.disparity_to_points_device(torch.from_numpy(disp).to(dev), r.Q, m)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape + (3,)
    got = got.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert nan.any() or disp.size == 1
    assert not np.isnan(want[disp == -9]).any()
    steps = _ulps(got[~nan], want[~nan])
    print(f"{shape}: {int((steps > 0).sum())} of {steps.size} coordinates differ from the host's float32, by at most {int(steps.max())} ulp")
    assert steps.max() <= 1
    pre = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    assert dp.disparity_to_points_device(torch.from_numpy(disp).to(dev), r.Q, m, out=pre) is pre
    assert np.array_equal(pre.cpu().numpy(), got, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the chain

OUT_W, OUT_H, X_OFF, Y_OFF = 96, 64, 112, 88                                  # the window of the rectified 320 x 240 frame that is matched
PLANE_D = 20                                                                 # the plane's disparity: its depth is f |Tn| / PLANE_D


def _render(K, dist, Rc, shift_x, tex, plane_z):
    """What a distorted camera sees of the plane Z = plane_z of rectified camera 0's frame, textured by ``tex`` (162 texels per
    metre, bilinear): source pixel -> Newton undistortion -> the ray in the camera's rectified frame -> the plane -> the texture.
    ``shift_x``: the camera's rectified frame lies at X + shift_x of rectified camera 0's."""
    W, H = rx.SIZE
    ys, xs = np.mgrid[0:H, 0:W]
    n = rc.undistort_points_newton(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64), K, dist)
    ray = np.c_[n, np.ones(len(n))] @ np.asarray(Rc).T
    X = ray[:, 0] / ray[:, 2] * plane_z - shift_x
    Y = ray[:, 1] / ray[:, 2] * plane_z
    tx, ty = X * 162.0 + tex.shape[1] / 2, Y * 162.0 + tex.shape[0] / 2
    x0 = np.clip(np.floor(tx).astype(int), 0, tex.shape[1] - 2)
    y0 = np.clip(np.floor(ty).astype(int), 0, tex.shape[0] - 2)
    fx, fy = np.clip(tx - x0, 0, 1), np.clip(ty - y0, 0, 1)
    t = tex.astype(np.float64)
    v = (t[y0, x0] * (1 - fx) + t[y0, x0 + 1] * fx) * (1 - fy) + (t[y0 + 1, x0] * (1 - fx) + t[y0 + 1, x0 + 1] * fx) * fy
    return np.where(np.isfinite(v), np.rint(v), 0).astype(np.uint8).reshape(H, W)


def test_chain_from_distorted_frames_to_points(dev):
    """Both cameras of the 15 degree vergence rig (B: 5 distortion coefficients, C: 8) look at a fronto-parallel textured plane at
    the depth whose disparity is 20 px (0.986 m); a 96 x 64 window of the rectified frames goes map -> remap -> matcher -> points, all on the device.  The host chain is
    remap_host and sgm_host over the SAME maps (the device's, copied back: the map is the one step that agrees with its host
    definition only up to rounding ties, tests/test_gpu_rectify.py).  The window is cut by moving both projections' principal
    point, which leaves the disparity as it is and moves Q's with it.
    The depth gate is one disparity step, a sixteenth of a pixel.  It checks the chain's geometry (the window, Q, the sign and scale
    of d), so the plane lies at a whole disparity, where the parabola's sub-pixel step has no bias by symmetry; between whole and
    half disparities a parabola through census costs is pulled towards the whole one (measured on the host at 1.0 m, 19.72 px: the
    median comes out at 19.875 px, 0.992 m), which is the definition's property and DESIGN 3.13's to state, not this gate's."""
    (K0, d0), (K1, d1) = sx.cam("B"), sx.cam("C")
    R, T = rx.rig_RT("verge15", "B", "C")
    r = rc.stereo_rectify_host(K0, d0, K1, d1, rx.SIZE, R, T)
    assert r.axis == 0 and r.Tn < 0
    tex = np.random.default_rng(12).integers(0, 256, (512, 512), dtype=np.uint8)
    f, m = r.P1[0, 0], 0
    plane_z = f * abs(r.Tn) / PLANE_D
    src0, src1 = _render(K0, d0, r.R1, 0.0, tex, plane_z), _render(K1, d1, r.R2, r.Tn, tex, plane_z)
    P1, P2, Q = r.P1.copy(), r.P2.copy(), r.Q.copy()
    for P in (P1, P2):
        P[0, 2] -= X_OFF
        P[1, 2] -= Y_OFF
    Q[0, 3] += X_OFF
    Q[1, 3] += Y_OFF

    maps = [rc.undistort_rectify_map_device(K, d, Rc, P, OUT_W, OUT_H, device=dev)
            for K, d, Rc, P in ((K0, d0, r.R1, P1), (K1, d1, r.R2, P2))]
    rect = [rc.remap_device(torch.from_numpy(s).to(dev), mp) for s, mp in zip((src0, src1), maps)]
    disp_dev = dp.sgm_device(rect[0], rect[1], min_disparity=m)
    pts_dev = dp.disparity_to_points_device(disp_dev, Q, m)

    rect_host = [rc.remap_host(s, mp.cpu().numpy()) for s, mp in zip((src0, src1), maps)]
    for a, b in zip(rect, rect_host):
        assert np.array_equal(a.cpu().numpy(), b)
    disp_host = dp.sgm_host(rect_host[0], rect_host[1], min_disparity=m)
    assert np.array_equal(disp_dev.cpu().numpy(), disp_host)

    valid = disp_host >= 16 * m
    pts = dp.disparity_to_points_host(disp_host, Q, m)
    z = pts[..., 2][valid & (disp_host != 0)]
    step = plane_z ** 2 / (16.0 * f * abs(r.Tn))
    print(f"{valid.mean():.3f} of the window valid, true disparity {PLANE_D} px, median depth {np.median(z):.5f} m for {plane_z:.5f} m, "
          f"one disparity step {step:.5f} m")
    assert valid.mean() > 0.5
    assert abs(np.median(z) - plane_z) <= step
    got = pts_dev.cpu().numpy()
    want = pts.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert _ulps(got[~np.isnan(want)], want[~np.isnan(want)]).max() <= 1
