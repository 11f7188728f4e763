"""The device side of stereo rectification (csrc/dcx_rectify.hip through deepcharuco_amd/rectify.py) against its host definitions:
the map (equal entries but for ties that rounding decides, counted by the test itself), the remap (bit for bit), the corner pool in
rectified coordinates (1e-9 px, DESIGN 3.8's gate; NaN where the host has NaN), the chain from two corner pools to epipolar rows and
3-D points, repeatability and graph capture.  Rigs, cameras and scenes are tests/rectify_exact.py's."""
import numpy as np
import pytest
import torch

import camera_exact as cx
import rectify_exact as rx
import stereo_exact as sx
from camera_exact import f64
from deepcharuco_amd import corner_pool, rectify as rc, stereo, weights

pytestmark = pytest.mark.gpu

W, H = rx.SIZE
F = rc.REMAP_FRAME_GROUP
R100 = f64(cx.rotation([0.0, np.deg2rad(100.0), 0.0]))
P_WIDE = np.array([[20.0, 0, 32.0], [0, 20.0, 24.0], [0, 0, 1]])          # +-58 degrees: with R100, rays on both sides of q_z = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _rectify(kind, c0, c1, alpha=None):
    R, T = rx.rig_RT(kind, c0, c1)
    (K0, d0), (K1, d1) = sx.cam(c0), sx.cam(c1)
    return rc.stereo_rectify_host(K0, d0, K1, d1, rx.SIZE, R, T, alpha)


# ------------------------------------------------------------------------------------------------ the map

def _map_agrees(dev, K, d, R, P, w, h, name, out=None):
    """Device map against host map: equal, but for entries whose unquantised 32 m lies within 1e-6 of a half-integer on the host
    (the two sum in different orders), which may differ by 1.  -> (entries differing, entries near a tie).  ``out``: the device
    tensor that receives the map."""
    host = rc.undistort_rectify_map_host(K, d, R, P, w, h)
    got = rc.undistort_rectify_map_device(K, d, R, P, w, h, device=dev, out=out)
    assert got.dtype == torch.int32 and tuple(got.shape) == (h, w, 2)
    got = got.cpu().numpy()
    s_h, s_d = host == rc.MAP_SENTINEL, got == rc.MAP_SENTINEL
    m32 = 32.0 * rc.undistort_rectify_map_host(K, d, R, P, w, h, quantised=False)
    with np.errstate(invalid="ignore"):
        near = np.abs(m32 - np.floor(m32) - 0.5) < 1e-6                      # (False at NaN: a sentinel is never excused)
    differ = host != got
    assert np.array_equal(s_h, s_d), name                                    # the sentinels are equal
    assert not (differ & ~near).any(), (name, int((differ & ~near).sum()))
    assert np.abs(host.astype(np.int64) - got)[differ].max(initial=0) <= 1, name
    print(f"{name}: {int(differ.sum())} of {host.size} entries differ, {int(near.sum())} lie within 1e-6 of a tie, "
          f"{int(s_h[..., 0].sum())} sentinels")
    assert differ.sum() <= near.sum()
    return host, got


@pytest.mark.parametrize("i,kind", list(enumerate(rx.RIGS)))
def test_map_device_matches_host(dev, i, kind):
    """Both cameras of every rig at 320 x 240 (pairs A/B, B/C, C/A, A/B: cameras without distortion, with 5 and with 8
    coefficients), and an odd 37 x 19 output cut from a 41 x 23 source."""
    c0, c1 = rx.PAIRS[i % 3]
    r = _rectify(kind, c0, c1)
    for cam, Rc, P in ((c0, r.R1, r.P1), (c1, r.R2, r.P2)):
        K, d = sx.cam(cam)
        _map_agrees(dev, K, d, Rc, P, W, H, f"{kind} camera {cam} 320x240")
        Ks = K.copy()
        Ks[:2] *= 41.0 / W                                                   # the camera of a 41 x 23 source
        Ps = P.copy()
        Ps[:2] *= 37.0 / W
        _map_agrees(dev, Ks, d, Rc, Ps, 37, 19, f"{kind} camera {cam} 37x19 of 41x23")


def test_map_sentinels_and_defaults(dev):
    K, d = sx.cam("B")
    host, _ = _map_agrees(dev, K, d, R100, P_WIDE, 64, 48, "R of 100 degrees")
    out = host == rc.MAP_SENTINEL
    assert out.any() and not out.all()
    for cam in ("A", "B", "C"):                                              # R = NULL, P = NULL: cv2.undistort's map
        K, d = sx.cam(cam)
        _map_agrees(dev, K, d, None, None, W, H, f"camera {cam}, R = NULL, P = NULL")
        _map_agrees(dev, K, d, None, np.c_[K, np.zeros(3)], 65, 3, f"camera {cam}, P = K as 3x4")
    pre = torch.full((19, 37, 2), 7, dtype=torch.int32, device=dev)
    assert rc.undistort_rectify_map_device(K, d, None, None, 37, 19, out=pre) is pre
    assert np.array_equal(pre.cpu().numpy(), rc.undistort_rectify_map_device(K, d, None, None, 37, 19, device=dev).cpu().numpy())
    with pytest.raises(ValueError):
        rc.undistort_rectify_map_device(K, np.zeros(12), None, None, 8, 8, device=dev)


# ------------------------------------------------------------------------------------------------ the remap

SRC_H, SRC_W = 23, 41


def _strided_source(dev, rng, batch, ch):
    """Random u8 frames 23 x 41 inside a larger buffer: gray at pitch 48, BGR at pitch 128, frames 24 bytes more than a frame
    apart, 5 bytes into the buffer -> (the strided device view, the same pixels as a dense host array)."""
    pitch = 48 if ch == 1 else 128
    stride = SRC_H * pitch + 24
    buf = torch.from_numpy(rng.integers(0, 256, 5 + batch * stride, dtype=np.uint8)).to(dev)
    shape, strides = ((batch, SRC_H, SRC_W), (stride, pitch, 1)) if ch == 1 else ((batch, SRC_H, SRC_W, 3), (stride, pitch, 3, 1))
    view = torch.as_strided(buf, shape, strides, 5)
    return view, view.cpu().numpy().copy()


def _random_map(rng, oh, ow):
    """Entries in [-3, 44) x [-3, 26) px of a 41 x 23 source: inside, across every edge and corner, wholly outside; plus
    sentinels and a few entries far away."""
    m = np.stack([rng.integers(-3 * 32, 44 * 32, (oh, ow)), rng.integers(-3 * 32, 26 * 32, (oh, ow))], 2).astype(np.int32)
    m[rng.random((oh, ow)) < 0.05] = rc.MAP_SENTINEL
    m[0, 0] = (-1, -1)
    m[0, 1] = (40 * 32 + 31, 22 * 32 + 31)
    m[1, 0] = (rc.MAP_SENTINEL, 64)
    m[1, 1] = (2 ** 31 - 1, 2 ** 31 - 1)
    m[2, 0] = (-2 ** 31 + 1, 77)
    return m


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("oh,ow", [(19, 37), (19, 36), (20, 37)])
def test_remap_bit_for_bit(dev, ch, oh, ow):
    """Output 19 x 37 (703 pixels: byte stores), 19 x 36 (out_w a multiple of 4) and 20 x 37 (whole dwords although out_w is
    odd); batches 1 and F - 1, F, F + 1 for the kernel's frame group F; border 0 and 7."""
    rng = np.random.default_rng([61, ch, oh, ow])
    m = _random_map(rng, oh, ow)
    md = torch.from_numpy(m).to(dev)
    for batch in (1, F - 1, F, F + 1):
        src, host_src = _strided_source(dev, rng, batch, ch)
        for border in (0, 7):
            want = rc.remap_host(host_src, m, border)
            got = rc.remap_device(src, md, border)
            assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (batch, border)
        one = rc.remap_device(src[batch - 1], md, 7)                         # a single frame: (H, W) or (H, W, 3)
        assert np.array_equal(one.cpu().numpy(), rc.remap_host(host_src[batch - 1], m, 7))


def test_remap_unaligned_map_and_out(dev):
    """A map that does not start on 16 bytes and an output that does not start on a dword take the byte path: same bits."""
    rng = np.random.default_rng(62)
    m = _random_map(rng, 19, 36)
    src, host_src = _strided_source(dev, rng, 3, 1)
    want = rc.remap_host(host_src, m, 3)
    mbuf = torch.zeros(2 + m.size, dtype=torch.int32, device=dev)
    mbuf[2:] = torch.from_numpy(m.ravel()).to(dev)
    obuf = torch.zeros(1 + want.size, dtype=torch.uint8, device=dev)
    got = rc.remap_device(src, mbuf[2:].view(19, 36, 2), 3, out=obuf[1:].view(3, 19, 36))
    assert got.data_ptr() % 4 == 1 and mbuf[2:].data_ptr() % 16 == 8
    assert np.array_equal(got.cpu().numpy(), want)


def test_remap_real_map_on_frames(dev):
    """A real rectification map (alpha = 0.5: some output pixels read outside) over nine 240 x 320 frames: 75 workgroups by two
    frame groups."""
    r = _rectify("verge15", "B", "C", alpha=0.5)
    K, d = sx.cam("B")
    m = rc.undistort_rectify_map_host(K, d, r.R1, r.P1, W, H)
    frames = weights.synthetic_frames("board", 11, F + 1, H, W)
    got = rc.remap_device(torch.from_numpy(frames).to(dev), torch.from_numpy(m).to(dev), border=0)
    want = rc.remap_host(frames, m, 0)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != frames).any() and want.std() > 10
    bgr = np.stack([frames[:2], 255 - frames[:2], frames[:2] // 3], 3)
    got3 = rc.remap_device(torch.from_numpy(bgr).to(dev), torch.from_numpy(m).to(dev), border=9)
    assert np.array_equal(got3.cpu().numpy(), rc.remap_host(bgr, m, 9))


def test_remap_refuses(dev):
    src = torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)
    m = torch.zeros((4, 4, 2), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        rc.remap_device(src.float(), m)
    with pytest.raises(ValueError):
        rc.remap_device(src, m, border=300)
    with pytest.raises(ValueError):
        rc.remap_device(src.transpose(1, 2), m)                              # pixels of a row not contiguous
    with pytest.raises(ValueError):
        rc.remap_device(src, m, out=torch.zeros((2, 4, 5), dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------ the points

def _pool(dev, xy, rows_xy=None):
    """A one-frame corner pool (counts | starts | rows | xy) of len(xy) slots."""
    n = len(xy)
    packed = np.zeros(corner_pool.packed_len(1, n), np.int32)
    counts, _, rows, xy_v, _ = corner_pool.views(packed, 1, n)
    counts[0] = n
    rows[:, 2] = np.arange(n) % 60
    if rows_xy is not None:
        rows[:, :2] = rows_xy
    xy_v[:] = np.asarray(xy, np.float32).reshape(n, 2)
    return torch.from_numpy(packed).to(dev)


def _points_agree(got, want, name):
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), name
    ok = ~np.isnan(want)
    gap = float(np.abs(got[ok] - want[ok]).max(initial=0.0))
    print(f"{name}: device - host {gap:.2e} px over {int(ok.sum()) // 2} points, {int((~ok).sum()) // 2} NaN")
    assert gap <= 1e-9, name


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_points_device_matches_host(dev, n):
    """Pools at the wave boundaries, cameras with no, 5 and 8 coefficients, under a rectification and under R = NULL / P = NULL;
    slot 0 (where there is one) lies far outside the frame, where camera B's model has no inverse within reach: NaN on both
    sides."""
    rng = np.random.default_rng([63, n])
    r = _rectify("verge15", "B", "C")
    xy = np.stack([rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)], 1).astype(np.float32)
    if n:
        xy[0] = (40000.0, 30000.0)
    packed = _pool(dev, xy)
    for cam, R, P in (("B", r.R1, r.P1), ("C", r.R2, r.P2), ("A", r.R1, r.P1), ("B", None, None)):
        K, d = sx.cam(cam)
        want = rc.rectify_points_host(xy.astype(np.float64), K, d, R, P)
        got = rc.rectify_points_pool(packed, 1, n, True, K, d, R, P)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, 2)
        _points_agree(got, want, f"n = {n} camera {cam}")
        if n and cam == "B":
            assert np.isnan(want[0]).all()


def test_points_behind_the_rectified_camera(dev):
    """Under a 100 degree rotation a part of the frame has rotated z <= 0: NaN there on both sides.  Rays within 0.05 of the
    horizon z = 0 are left out of the pool: there the rectified pixel grows as 1 / z and its rounding as 1 / z^2, and 1e-9 px
    is a gate for pixels, not for points at infinity."""
    rng = np.random.default_rng(67)
    K, d = sx.cam("C")
    xy = np.stack([rng.uniform(0, W, 400), rng.uniform(0, H, 400)], 1).astype(np.float32)
    n = rc.undistort_points_newton(xy.astype(np.float64), K, d)
    z = R100[2, 0] * n[:, 0] + R100[2, 1] * n[:, 1] + R100[2, 2]
    xy = xy[np.abs(z) >= 0.05][:129]
    assert len(xy) == 129
    want = rc.rectify_points_host(xy.astype(np.float64), K, d, R100, P_WIDE)
    assert np.isnan(want).any() and np.isfinite(want).any()
    _points_agree(rc.rectify_points_pool(_pool(dev, xy), 1, 129, True, K, d, R100, P_WIDE), want, "R of 100 degrees")


def test_points_from_the_integer_rows(dev):
    """d_xy == NULL: the integer x, y of the rows are the pixels (the xy words of the pool hold something else)."""
    rng = np.random.default_rng(64)
    n = 70
    cells = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    packed = _pool(dev, rng.uniform(0, 200, (n, 2)), rows_xy=cells)
    K, d = sx.cam("C")
    r = _rectify("small", "C", "A")
    got = rc.rectify_points_pool(packed, 1, n, False, K, d, r.R1, r.P1)
    _points_agree(got, rc.rectify_points_host(cells.astype(np.float64), K, d, r.R1, r.P1), "integer rows")
    short = packed[:2 + 4 * n].contiguous()                                  # a pool without xy words is enough
    _points_agree(rc.rectify_points_pool(short, 1, n, False, K, d, r.R1, r.P1),
                  rc.rectify_points_host(cells.astype(np.float64), K, d, r.R1, r.P1), "integer rows, pool without xy")
    with pytest.raises(ValueError):
        rc.rectify_points_pool(short, 1, n, True, K, d, r.R1, r.P1)


# ------------------------------------------------------------------------------------------------ the chain

@pytest.mark.parametrize("kind,c0,c1", [("small", "A", "B"), ("verge15", "B", "C"), ("vertical", "C", "A")])
def test_chain_from_pools_to_epipolar_rows(dev, kind, c0, c1):
    """Scene -> two corner pools -> stereo_calibrate_pool -> stereo_rectify_host -> rectify_points_pool on both pools: the
    epipolar gap and the 3-D error are within 4x of what the host chain (stereo_calibrate_host_full -> stereo_rectify_host ->
    rectify_points_host) gives on the same scene."""
    s = rx.scene(kind, c0, c1)
    cams = sx.cam_args(s)
    (p0, b, pool0), (p1, _, pool1) = corner_pool.pack_keypoints(s.kps0, dev), corner_pool.pack_keypoints(s.kps1, dev)
    est = stereo.stereo_calibrate_pool(p0, p1, b, pool0, pool1, True, *s.board, *cams)
    assert est.status == stereo.STEREO_OK and est.pairs_used == b
    r = rc.stereo_rectify_host(*cams, rx.SIZE, est.R, est.T)
    q0 = rc.rectify_points_pool(p0, b, pool0, True, cams[0], cams[1], r.R1, r.P1).cpu().numpy()
    q1 = rc.rectify_points_pool(p1, b, pool1, True, cams[2], cams[3], r.R2, r.P2).cpu().numpy()

    def slots(kps, q):
        starts = np.concatenate([[0], np.cumsum([len(k) for k in kps])[:-1]])

        def of(t, ids, pix):
            sorted_ids = np.sort(kps[t][:, 2], kind="stable")
            at = starts[t] + np.searchsorted(sorted_ids, ids)
            return q[at]
        return of
    gap_d, err_d = rx.epipolar_and_depth(s, r, rc.reproject_to_3d, slots(s.kps0, q0), slots(s.kps1, q1))

    h = stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *cams)
    assert h.status == stereo.STEREO_OK
    rh = rc.stereo_rectify_host(*cams, rx.SIZE, h.R, h.T)
    assert rh.axis == r.axis == (1 if kind == "vertical" else 0)
    gap_h, err_h = rx.epipolar_and_depth(s, rh, rc.reproject_to_3d,
                                         lambda t, ids, pix: rc.rectify_points_host(pix, cams[0], cams[1], rh.R1, rh.P1),
                                         lambda t, ids, pix: rc.rectify_points_host(pix, cams[2], cams[3], rh.R2, rh.P2))
    print(f"{kind} {c0}/{c1}: epipolar gap device {gap_d:.3e} px, host {gap_h:.3e} px; 3-D error device {err_d:.3e}, host {err_h:.3e}")
    assert gap_d <= 4 * gap_h
    assert err_d <= 4 * err_h


# ------------------------------------------------------------------------------------------------ repeatability, capture

def test_two_calls_give_equal_bits(dev):
    rng = np.random.default_rng(65)
    K, d = sx.cam("C")
    r = _rectify("toe90", "C", "A")
    maps = [rc.undistort_rectify_map_device(K, d, r.R1, r.P1, W, H, device=dev) for _ in range(2)]
    assert torch.equal(maps[0], maps[1])
    src, _ = _strided_source(dev, rng, F + 1, 3)
    small = torch.from_numpy(_random_map(rng, 19, 36)).to(dev)
    outs = [rc.remap_device(src, small, 7) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    packed = _pool(dev, np.stack([rng.uniform(0, W, 129), rng.uniform(0, H, 129)], 1))
    pts = [rc.rectify_points_pool(packed, 1, 129, True, K, d, r.R1, r.P1).cpu().numpy() for _ in range(2)]
    assert np.array_equal(pts[0].view(np.uint64), pts[1].view(np.uint64))


def test_remap_and_points_replay_from_a_graph(dev):
    """remap_device and rectify_points_pool captured in one linear graph replay to the eager bits (neither synchronises nor
    allocates when given its output)."""
    rng = np.random.default_rng(66)
    K, d = sx.cam("B")
    r = _rectify("verge15", "B", "C", alpha=0.0)
    md = rc.undistort_rectify_map_device(K, d, r.R1, r.P1, W, H, device=dev)
    frames = torch.from_numpy(weights.synthetic_frames("board", 12, F + 1, H, W)).to(dev)
    packed = _pool(dev, np.stack([rng.uniform(0, W, 129), rng.uniform(0, H, 129)], 1))
    eager = (rc.remap_device(frames, md, 5), rc.rectify_points_pool(packed, 1, 129, True, K, d, r.R1, r.P1))
    out = (torch.zeros_like(eager[0]), torch.zeros_like(eager[1]))

    def enqueue():
        rc.remap_device(frames, md, 5, out=out[0])
        rc.rectify_points_pool(packed, 1, 129, True, K, d, r.R1, r.P1, out=out[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                               # warm-up launch outside the capture
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    out[0].zero_()
    out[1].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0])
    assert np.array_equal(out[1].cpu().numpy().view(np.uint64), eager[1].cpu().numpy().view(np.uint64))
