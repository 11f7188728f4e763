"""deepcharuco_amd/resize.py on the host: the numpy definition of the resize against float64 interpolation written here on its own,
the identities the three modes share, what is refused, the two ways between resized and source pixels against the exact camera
model of tests/camera_exact.py, and the C entry's refusals (which come before anything is launched, so they need no GPU)."""
import ctypes

import numpy as np
import pytest

import camera_exact as cx
import resize_cases as rc
from deepcharuco_amd import resize as rz


def _frames(shape, kind, seed):
    return rc.noise(shape, seed) if kind == "noise" else rc.extremes(shape, seed)


def _bilinear_f64(img, dh, dw):
    """Float64 bilinear interpolation of (H, W): the output pixel's centre in source coordinates, (d + 0.5) sn / dn - 0.5, clamped
    into the frame; the two neighbours on each axis weighted by the distance."""
    sh, sw = img.shape
    y = np.clip((np.arange(dh) + 0.5) * sh / dh - 0.5, 0, sh - 1)
    x = np.clip((np.arange(dw) + 0.5) * sw / dw - 0.5, 0, sw - 1)
    y0, x0 = np.minimum(np.floor(y).astype(int), max(sh - 2, 0)), np.minimum(np.floor(x).astype(int), max(sw - 2, 0))
    y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
    wy, wx = (y - y0)[:, None], (x - x0)[None, :]
    f = img.astype(np.float64)
    top = f[y0][:, x0] * (1 - wx) + f[y0][:, x1] * wx
    bot = f[y1][:, x0] * (1 - wx) + f[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def test_linear_is_within_one_level_of_float64_bilinear():
    """Every pixel of every "linear" shape differs from exact bilinear interpolation by less than 1 gray level (the scheme's own
    error: 11-bit coefficients, a 4-bit and two 16-bit truncations and the final rounding; 0.78 at worst when it was
    prototyped).  The share of pixels that are not the rounded exact value is printed, not gated."""
    worst, off, total = 0.0, 0, 0
    for i, (sh, sw, dh, dw) in enumerate(rc.shapes("linear")):
        for kind in ("noise", "extremes"):
            img = _frames((sh, sw), kind, i)
            got = rz.resize_host(img, (dh, dw), "linear")
            exact = _bilinear_f64(img, dh, dw)
            assert got.shape == (dh, dw) and got.dtype == np.uint8
            gap = np.abs(got.astype(np.float64) - exact)
            print(f"linear {sh}x{sw} -> {dh}x{dw} {kind}: worst {gap.max():.4f}")
            assert gap.max() < 1.0, (sh, sw, dh, dw, kind, float(gap.max()))
            worst = max(worst, float(gap.max()))
            off += int((got != np.clip(np.rint(exact), 0, 255)).sum())
            total += got.size
    print(f"linear: worst gap {worst:.4f} gray levels; {100.0 * off / total:.2f} % of {total} pixels are not the rounded exact value")


@pytest.mark.parametrize("shape", rc.shapes("area"), ids=lambda s: "x".join(map(str, s)))
def test_area_is_the_rounded_mean(shape):
    sh, sw, dh, dw = shape
    fy, fx = sh // dh, sw // dw
    for kind in ("noise", "extremes"):
        img = _frames((sh, sw), kind, fy * 100 + fx)
        mean = img.astype(np.float64).reshape(dh, fy, dw, fx).mean(axis=(1, 3))
        got = rz.resize_host(img, (dh, dw), "area")
        assert got.shape == (dh, dw) and np.abs(got - mean).max() <= 0.5 + 1e-4


def test_linear_on_a_2x_shape_is_area():
    for sh, sw in ((48, 64), (10, 14), (2, 2)):
        for shape in ((sh, sw), (3, sh, sw, 3)):
            img = rc.noise(shape, sh)
            assert np.array_equal(rz.resize_host(img, (sh // 2, sw // 2), "linear"), rz.resize_host(img, (sh // 2, sw // 2), "area"))
    img = rc.noise((48, 64), 5)                                # 2x on one axis only: not the rule
    assert not np.array_equal(rz.resize_host(img, (24, 16), "linear"), rz.resize_host(img, (24, 16), "area"))


@pytest.mark.parametrize("mode", rc.MODES)
def test_blocks_of_4x4_come_back_and_identity_is_identity(mode):
    img = rc.noise((11, 13), 3)
    big = np.kron(img, np.ones((4, 4), np.uint8))
    assert np.array_equal(rz.resize_host(big, img.shape, mode), img)
    bgr = rc.noise((2, 11, 13, 3), 4)
    big = np.kron(bgr, np.ones((1, 4, 4, 1), np.uint8))
    assert np.array_equal(rz.resize_host(big, (11, 13), mode), bgr)
    for shape in ((8, 8), (37, 53), (2, 9, 11, 3)):
        x = rc.noise(shape, 6)
        size = shape[-3:-1] if len(shape) == 4 else shape
        assert np.array_equal(rz.resize_host(x, size, mode), x)


@pytest.mark.parametrize("mode", rc.MODES)
def test_channels_and_frames_are_independent(mode):
    sh, sw, dh, dw = (30, 42, 10, 14) if mode == "area" else (30, 40, 7, 9)
    x = rc.noise((3, sh, sw, 3), 8)
    got = rz.resize_host(x, (dh, dw), mode)
    assert got.shape == (3, dh, dw, 3) and got.flags.c_contiguous
    for b in range(3):
        assert np.array_equal(rz.resize_host(x[b], (dh, dw), mode), got[b])                      # (H, W, 3): one colour frame
        for c in range(3):
            assert np.array_equal(rz.resize_host(np.ascontiguousarray(x[b, :, :, c]), (dh, dw), mode), got[b, :, :, c])
    gray = np.ascontiguousarray(x[..., 0])
    assert np.array_equal(rz.resize_host(gray, (dh, dw), mode), got[..., 0])                     # (B, H, W)


def test_refusals():
    img = rc.noise((10, 10), 1)
    with pytest.raises(ValueError):
        rz.resize_host(img, (3, 3), "area")                                  # a fractional factor
    with pytest.raises(ValueError):
        rz.resize_host(rc.noise((65, 7), 1), (1, 7), "area")                 # a factor of 65
    assert rz.resize_host(rc.noise((64, 7), 1), (1, 7), "area").shape == (1, 7)
    with pytest.raises(ValueError):
        rz.resize_host(img, (20, 20), "area")                                # area does not enlarge
    with pytest.raises(ValueError):
        rz.resize_host(img.astype(np.float32), (5, 5))
    with pytest.raises(ValueError):
        rz.resize_host(img.astype(np.int8), (5, 5), "nearest")
    with pytest.raises(ValueError):
        rz.resize_host(img, (5, 5), "cubic")
    with pytest.raises(ValueError):
        rz.resize_host(img, (0, 5))
    with pytest.raises(ValueError):
        rz.resize_host(img, (5, 32769), "nearest")
    with pytest.raises(ValueError):
        rz.resize_host(rc.noise((2, 4, 4, 2), 1), (2, 2))                    # two channels


# ------------------------------------------------------------------------------------------------ points and cameras

K_CAM = np.array([[1510.25, 0.0, 963.5], [0.0, 1498.75, 531.25], [0.0, 0.0, 1.0]])
DIST = np.array([-0.21, 0.07, 0.0011, -0.0007, 0.013])


@pytest.mark.parametrize("src,dst,origin", [((1440, 1920), (240, 320), (0, 0)), ((1080, 1440), (240, 320), (240, 0)),
                                             ((1000, 1700), (240, 320), (37.0, 11.0)), ((240, 320), (480, 960), (0, 0))])
def test_scaled_camera_projects_where_mapped_points_land(src, dst, origin):
    """A board projected with K, the pixels taken to the resized frame == the board projected with scale_camera_matrix(K), to
    1e-9 px, with a window origin and with sw / dw != sh / dh; and map_points brings them back."""
    board = (6, 5)
    obj = cx.board_points(np.arange(cx.n_ids(board)), board[0], board[1], 0.04).astype(np.float64)
    pose = np.array([0.21, -0.33, 0.12, -0.09, -0.07, 0.62])
    pix = cx.f64(cx.project(obj, pose, K_CAM, cx.dist8(DIST)))
    Ks = rz.scale_camera_matrix(K_CAM, src, dst, origin)
    assert Ks.shape == (3, 3) and Ks[2].tolist() == [0, 0, 1] and Ks[0, 1] == 0
    assert Ks[0, 0] == pytest.approx(K_CAM[0, 0] * dst[1] / src[1], rel=1e-14)
    assert Ks[1, 1] == pytest.approx(K_CAM[1, 1] * dst[0] / src[0], rel=1e-14)
    small = cx.f64(cx.project(obj, pose, Ks, cx.dist8(DIST)))
    there = rz.map_points(pix, src, dst, origin, inverse=True)
    assert np.abs(there - small).max() < 1e-9
    sx, sy = src[1] / dst[1], src[0] / dst[0]
    assert np.abs((pix[:, 0] + 0.5 - origin[0]) / sx - 0.5 - small[:, 0]).max() < 1e-9           # the formula, written out
    assert np.abs((pix[:, 1] + 0.5 - origin[1]) / sy - 0.5 - small[:, 1]).max() < 1e-9
    back = rz.map_points(there, src, dst, origin)
    assert np.abs(back - pix).max() < 1e-9
    assert np.abs(rz.map_points(small, src, dst, origin) - pix).max() < 1e-9


def test_map_points_forms():
    import torch
    src, dst = (960, 1280), (240, 320)
    p = np.array([[0.0, 0.0, 5.0], [319.0, 239.0, 2.0], [10.25, 7.5, 0.0]])
    got = rz.map_points(p, src, dst)
    assert got.dtype == np.float64 and np.array_equal(got[:, 2], p[:, 2]) and got is not p
    assert np.array_equal(got[:, :2], [[1.5, 1.5], [1277.5, 957.5], [42.5, 31.5]])               # (x + 0.5) * 4 - 0.5
    assert np.array_equal(rz.map_points(p[:2].astype(np.int64), src, dst), got[:2])              # integer rows become float64
    assert np.array_equal(rz.map_points(got, src, dst, inverse=True), p)
    assert np.array_equal(rz.map_points(rz.map_points(p, dst, src), src, dst), p)               # swapping the sizes is the inverse
    t = torch.from_numpy(p[:, :2].astype(np.float32))
    gt = rz.map_points(t, src, dst, origin=(100, 50))
    assert isinstance(gt, torch.Tensor) and gt.dtype == torch.float32 and gt is not t
    assert np.array_equal(gt.numpy(), (got[:, :2] + [100, 50]).astype(np.float32))
    assert np.array_equal(t.numpy(), p[:, :2].astype(np.float32))                                # the input is left alone
    with pytest.raises(ValueError):
        rz.map_points(torch.zeros((3, 2), dtype=torch.int32), src, dst)
    with pytest.raises(ValueError):
        rz.map_points(np.zeros(3), src, (0, 320))


# ------------------------------------------------------------------------------------------------ the C entry

def test_c_entry_refuses_before_it_launches():
    """Every call here is refused, so nothing is launched and the pointers (never read) need not be device memory."""
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    p = ctypes.c_void_p(4096)

    def call(src=p, stride=0, pitch=64, sh=8, sw=8, ch=1, dh=4, dw=4, batch=1, interp=1, out=p):
        return lib.dcx_resize_u8(src, stride, pitch, sh, sw, ch, dh, dw, batch, interp, out, None)

    assert call(src=None) == E_ARG and call(out=None) == E_ARG
    assert call(ch=2) == E_ARG and call(ch=0) == E_ARG and call(ch=4) == E_ARG
    assert call(interp=3) == E_ARG and call(interp=-1) == E_ARG
    assert call(stride=-1) == E_ARG
    assert call(ch=2, sh=0) == E_ARG                                         # a bad argument is named before a bad shape
    for name in ("sh", "sw", "dh", "dw", "batch"):
        for v in (0, -1, 32769):
            assert call(**{name: v, "pitch": 40000}) == E_SHAPE, (name, v)
    assert call(pitch=7) == E_SHAPE and call(ch=3, pitch=23) == E_SHAPE
    assert call(pitch=70000, sh=32768, dh=32768) == E_SHAPE                  # pitch * src_h beyond an int32
    assert call(sh=10, sw=10, dh=3, dw=3, interp=2) == E_SHAPE               # a fractional area factor
    assert call(sh=10, sw=9, dh=5, dw=4, interp=2) == E_SHAPE
    assert call(sh=65, sw=8, dh=1, dw=8, interp=2) == E_SHAPE                # a factor of 65
    assert call(sh=8, sw=130, pitch=130, dh=8, dw=2, interp=2) == E_SHAPE
    assert call(sh=8, sw=8, dh=16, dw=16, interp=2) == E_SHAPE               # area does not enlarge
