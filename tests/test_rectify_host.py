"""The host definition of stereo rectification (deepcharuco_amd/rectify.py) against exact math: the properties that define a
rectifying pair of rotations, the Newton undistortion against the long-double camera model of tests/camera_exact.py, epipolar rows
and 3-D recovery on noise-free two-camera scenes, the promises of ``alpha``, the map against tests/rectify_exact.py, and the integer
remap on hand-computed cases.  No GPU.

Measured on the committed definition (the gates of the truth-recovery test are 4x these, the project's convention):

    rig        epipolar gap (px)   3-D error (relative)     worst of the pairs A/B, B/C, C/A, 6 noise-free pairs each
    small      1.36e-5             1.84e-7
    toe90      1.74e-5             4.3e-8
    verge15    1.37e-5             2.86e-7
    vertical   2.15e-5             1.24e-7

(the gap is the float32 rounding of the input pixels, 1.5e-5 px at 300 px, carried through the rectification)."""
import numpy as np
import pytest

import camera_exact as cx
import rectify_exact as rx
import stereo_exact as sx
from camera_exact import _w, f64
from deepcharuco_amd import rectify as rc

W, H = rx.SIZE
MEASURED = {"small": (1.36e-5, 1.84e-7), "toe90": (1.74e-5, 4.3e-8), "verge15": (1.37e-5, 2.86e-7), "vertical": (2.15e-5, 1.24e-7)}
CASES = [(k, c0, c1) for k in rx.RIGS for c0, c1 in rx.PAIRS]


def _rectify(kind, c0, c1, alpha=None):
    R, T = rx.rig_RT(kind, c0, c1)
    (K0, d0), (K1, d1) = sx.cam(c0), sx.cam(c1)
    return rc.stereo_rectify_host(K0, d0, K1, d1, rx.SIZE, R, T, alpha), R, T


# ------------------------------------------------------------------------------------------------ the rotations

@pytest.mark.parametrize("kind,c0,c1", CASES)
def test_rectify_properties(kind, c0, c1):
    r, R, T = _rectify(kind, c0, c1)
    for M in (r.R1, r.R2):
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(M) - 1) <= 1e-14
    e_rot = float(np.abs(r.R2 @ R @ r.R1.T - np.eye(3)).max())
    t = r.R2 @ T
    e_off = float(np.linalg.norm(np.delete(t, r.axis)) / np.linalg.norm(T))
    print(f"{kind} {c0}/{c1}: |R2 R R1^T - I| = {e_rot:.2e}, off-axis part of R2 T = {e_off:.2e}, axis {r.axis}")
    assert e_rot <= 1e-14
    assert e_off <= 1e-14
    assert r.axis == (1 if kind == "vertical" else 0)
    assert r.Tn == t[r.axis] and abs(abs(r.Tn) - np.linalg.norm(T)) <= 1e-14 * np.linalg.norm(T)
    assert r.P2[r.axis, 3] == r.Tn * r.P1[0, 0] and np.array_equal(np.delete(r.P2.ravel(), 4 * r.axis + 3), np.delete(r.P1.ravel(), 4 * r.axis + 3))
    assert r.P1[0, 0] == r.P1[1, 1] == min(sx.cam_K(c0)[1, 1], sx.cam_K(c1)[1, 1])


def test_parallel_rig_is_left_alone():
    """R = I with T along x: both rectifying rotations are the identity, exactly."""
    for tx in (-0.06, 0.11):
        r = rc.stereo_rectify_host(sx.K_A, None, sx.K_B, sx.cam_coeffs("B"), rx.SIZE, np.eye(3), [tx, 0.0, 0.0])
        assert np.array_equal(r.R1, np.eye(3)) and np.array_equal(r.R2, np.eye(3))
        assert r.axis == 0 and r.Tn == tx


def test_refused_arguments():
    K, d = sx.cam("B")
    with pytest.raises(ValueError):
        rc.stereo_rectify_host(K, d, K, d, rx.SIZE, np.eye(3), [0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        rc.stereo_rectify_host(K, d, K, d, rx.SIZE, np.eye(3), [0.1, 0.0, 0.0], alpha=1.5)
    with pytest.raises(ValueError):
        rc.stereo_rectify_host(K, np.zeros(12), K, d, rx.SIZE, np.eye(3), [0.1, 0.0, 0.0])
    with pytest.raises(ValueError):
        rc.undistort_rectify_map_host(K, d, None, np.eye(4), 8, 8)


# ------------------------------------------------------------------------------------------------ Newton undistortion

@pytest.mark.parametrize("cam", ["B", "C", "A4"])
def test_newton_undistortion_round_trip(cam):
    """Newton's result, pushed through the exact distortion model, returns to the pixel within 1e-12 px on a 7-px grid over the
    frame; the documented 5 fixed-point rounds, held to the same assertion, miss it by nine orders of magnitude."""
    K, d = sx.cam(cam)
    g = rx.pixel_grid(7)
    n = rc.undistort_points_newton(g, K, d)
    assert np.isfinite(n).all()
    e = float(np.abs(cx.distort(_w(n[:, 0]), _w(n[:, 1]), K, cx.dist8(d)) - _w(g)).max())
    n5 = cx.undistort5(g, K, d)
    e5 = float(np.abs(cx.distort(n5[:, 0], n5[:, 1], K, cx.dist8(d)) - _w(g)).max())
    print(f"camera {cam}: round trip through the exact model, Newton {e:.2e} px, 5 fixed-point rounds {e5:.2e} px")
    assert e <= 1e-12
    assert not e5 <= 1e-12                      # the gate separates the two


def test_newton_without_distortion_and_out_of_reach():
    g = rx.pixel_grid(31)
    n = rc.undistort_points_newton(g, sx.K_A, None)
    assert np.array_equal(n, np.stack([(g[:, 0] - sx.K_A[0, 2]) / sx.K_A[0, 0], (g[:, 1] - sx.K_A[1, 2]) / sx.K_A[1, 1]], 1))
    K, d = sx.cam("B")                          # far outside the frame the model of camera B has no inverse near the start
    out = rc.rectify_points_host(np.array([[40000.0, 30000.0], [100.0, 100.0]]), K, d)
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all()
    behind = rc.rectify_points_host(np.array([[160.0, 120.0]]), K, d, f64(cx.rotation([0.0, np.deg2rad(100.0), 0.0])))
    assert np.isnan(behind).all()               # rotated z <= 0


@pytest.mark.parametrize("cam", ["A", "B", "C"])
def test_rectified_projection_against_exact(cam):
    """Exact pixels of known normalised points -> rectify_points_host returns the exact rectified projection of those points.
    1e-11 px: the pixels are rounded to float64 (4e-14 px at 320), Newton returns through the model to 8e-14 px, and the rectified
    camera magnifies by at most P00 / fx * (1 + tan^2) < 4 on this grid and rotation."""
    K, d = sx.cam(cam)
    r, _, _ = _rectify("verge15", cam, "A" if cam != "A" else "B")
    n = np.stack([(g - c) / f for g, c, f in zip(rx.pixel_grid(13).T, (K[0, 2], K[1, 2]), (K[0, 0], K[1, 1]))], 1) * 0.8
    pix = f64(cx.distort(_w(n[:, 0]), _w(n[:, 1]), K, cx.dist8(d)))
    got = rc.rectify_points_host(pix, K, d, r.R1, r.P1)
    e = float(np.abs(_w(got) - rx.rectified_exact(n, r.R1, r.P1)).max())
    print(f"camera {cam}: rectified projection against the exact one {e:.2e} px")
    assert e <= 1e-11


# ------------------------------------------------------------------------------------------------ epipolar rows, 3-D recovery

@pytest.mark.parametrize("kind,c0,c1", CASES)
def test_epipolar_rows_and_depth_under_the_true_rig(kind, c0, c1):
    s = rx.scene(kind, c0, c1)
    r, _, _ = _rectify(kind, c0, c1)
    (K0, d0), (K1, d1) = sx.cam(c0), sx.cam(c1)
    gap, err = rx.epipolar_and_depth(s, r, rc.reproject_to_3d, lambda t, i, p: rc.rectify_points_host(p, K0, d0, r.R1, r.P1),
                                     lambda t, i, p: rc.rectify_points_host(p, K1, d1, r.R2, r.P2))
    print(f"{kind} {c0}/{c1}: epipolar gap {gap:.3e} px, 3-D error {err:.3e}")
    assert gap <= 4 * MEASURED[kind][0]
    assert err <= 4 * MEASURED[kind][1]


def test_q_is_the_depth_of_a_disparity():
    r, _, _ = _rectify("small", "A", "B")
    f, cxp, cyp = r.P1[0, 0], r.P1[0, 2], r.P1[1, 2]
    X = rc.reproject_to_3d(r.Q, [[cxp + 10.0, cyp - 4.0]], [[cxp + 2.0, cyp - 4.0]], 0)[0]
    Z = -f * r.Tn / 8.0
    assert np.allclose(X, [10.0 * Z / f, -4.0 * Z / f, Z], rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------ alpha

@pytest.mark.parametrize("kind,c0,c1", [c for c in CASES if c[0] != "toe90"])
def test_alpha(kind, c0, c1):
    """alpha = 0: no output pixel reads outside the source; alpha = 1: no source border pixel falls outside the output; f falls
    monotonically in between."""
    cams = (sx.cam(c0), sx.cam(c1))
    r0, _, _ = _rectify(kind, c0, c1, 0.0)
    for (K, d), Rc, P in zip(cams, (r0.R1, r0.R2), (r0.P1, r0.P2)):
        m = rc.undistort_rectify_map_host(K, d, Rc, P, W, H, quantised=False)
        print(f"{kind} {c0}/{c1} alpha 0: sources x [{m[..., 0].min():.6f}, {m[..., 0].max():.6f}] y [{m[..., 1].min():.6f}, {m[..., 1].max():.6f}]")
        assert np.isfinite(m).all()
        assert m[..., 0].min() >= -1e-6 and m[..., 0].max() <= W - 1 + 1e-6
        assert m[..., 1].min() >= -1e-6 and m[..., 1].max() <= H - 1 + 1e-6
    r1, _, _ = _rectify(kind, c0, c1, 1.0)
    border = np.concatenate(rc._border_pixels(W, H))
    for (K, d), Rc, P in zip(cams, (r1.R1, r1.R2), (r1.P1, r1.P2)):
        q = rc.rectify_points_host(border, K, d, Rc, P)
        assert q[:, 0].min() >= -1e-6 and q[:, 0].max() <= W - 1 + 1e-6
        assert q[:, 1].min() >= -1e-6 and q[:, 1].max() <= H - 1 + 1e-6
    fs = [_rectify(kind, c0, c1, a)[0].P1[0, 0] for a in (0.0, 0.25, 0.5, 0.75, 1.0)]
    assert all(a > b for a, b in zip(fs, fs[1:])), fs
    for a in (0.0, 1.0):                      # alpha moves f alone
        ra = _rectify(kind, c0, c1, a)[0]
        rn = _rectify(kind, c0, c1)[0]
        assert np.array_equal(ra.R1, rn.R1) and np.array_equal(ra.P1[:, 2], rn.P1[:, 2])


# ------------------------------------------------------------------------------------------------ the map

MAP_CASES = [("small", "A", "B"), ("verge15", "B", "C"), ("vertical", "C", "A")]


@pytest.mark.parametrize("kind,c0,c1", MAP_CASES)
def test_map_against_exact(kind, c0, c1):
    r, _, _ = _rectify(kind, c0, c1)
    for (K, d), Rc, P in zip((sx.cam(c0), sx.cam(c1)), (r.R1, r.R2), (r.P1, r.P2)):
        m = rc.undistort_rectify_map_host(K, d, Rc, P, W, H, quantised=False)
        q = rc.undistort_rectify_map_host(K, d, Rc, P, W, H)
        ex = rx.map_exact(K, d, Rc, P, W, H)
        assert np.isfinite(m).all() and q.dtype == np.int32 and q.shape == (H, W, 2)
        e = float(np.abs(_w(m) - ex).max())
        differ = int((np.rint(f64(ex * 32)) != q).sum())
        print(f"{kind} {c0}/{c1}: map against the long-double model {e:.2e} px, quantised entries differing {differ} of {q.size}")
        assert e <= 1e-12
        assert differ == 0


def test_map_identity_sentinel_and_sizes():
    K, d = sx.cam("B")
    m = rc.undistort_rectify_map_host(sx.K_A, None, None, None, 37, 19)             # no distortion, R = I, P = K: the identity
    u, v = np.meshgrid(np.arange(37), np.arange(19))
    assert np.array_equal(m[..., 0], 32 * u) and np.array_equal(m[..., 1], 32 * v)
    R100 = f64(cx.rotation([0.0, np.deg2rad(100.0), 0.0]))
    Pw = np.array([[20.0, 0, 32.0], [0, 20.0, 24.0], [0, 0, 1]])                     # +-58 degrees: rays on both sides of q_z = 0
    q = rc.undistort_rectify_map_host(K, d, R100, Pw, 64, 48)
    out = (q == rc.MAP_SENTINEL)
    assert out.any() and not out.all() and np.array_equal(out[..., 0], out[..., 1])
    f = rc.undistort_rectify_map_host(K, d, R100, Pw, 64, 48, quantised=False)
    assert np.array_equal(np.isnan(f[..., 0]), out[..., 0])
    # ties to even: 32 m = k + 1/2 exactly
    Kt = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
    P = np.array([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]])
    t = rc.undistort_rectify_map_host(Kt, None, None, P, 8, 1)                      # m = u / 64, 32 m = u / 2
    assert t[0, :, 0].tolist() == [0, 0, 1, 2, 2, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ the remap

def _map_of(xy32):
    return np.asarray(xy32, np.int32).reshape(1, -1, 2)


def test_remap_identity():
    rng = np.random.default_rng(5)
    for shape in ((9, 14), (3, 9, 14), (9, 14, 3), (2, 9, 14, 3)):
        src = rng.integers(0, 256, shape, dtype=np.uint8)
        h, w = (shape[-3], shape[-2]) if shape[-1] == 3 else shape[-2:]
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        m = np.stack([32 * u, 32 * v], 2).astype(np.int32)
        out = rc.remap_host(src, m)
        assert out.dtype == np.uint8 and out.shape == src.shape and np.array_equal(out, src)


def test_remap_weights_by_hand():
    src = np.array([[10, 20], [40, 250]], np.uint8)
    # (fx, fy) -> ((32-fx)(32-fy) 10 + fx (32-fy) 20 + (32-fx) fy 40 + fx fy 250 + 512) >> 10
    cases = {(0, 0): 10, (31, 0): (32 * 10 + 31 * 32 * 20 + 512) >> 10, (0, 31): (32 * 10 + 31 * 32 * 40 + 512) >> 10,
             (16, 16): (256 * (10 + 20 + 40 + 250) + 512) >> 10, (31, 31): (10 + 31 * 20 + 31 * 40 + 961 * 250 + 512) >> 10,
             (8, 24): (24 * 8 * 10 + 8 * 8 * 20 + 24 * 24 * 40 + 8 * 24 * 250 + 512) >> 10}
    assert cases[(16, 16)] == 80 and cases[(31, 31)] == 236 and cases[(8, 24)] == 73
    for (fx, fy), want in cases.items():
        assert rc.remap_host(src, _map_of([[fx, fy]]))[0, 0] == want, (fx, fy)
    rgb = np.stack([src, 255 - src, src // 2], 2)
    got = rc.remap_host(rgb, _map_of([[8, 24]]))[0, 0]
    assert got.tolist() == [rc.remap_host(np.ascontiguousarray(rgb[..., c]), _map_of([[8, 24]]))[0, 0] for c in range(3)]


def test_remap_border_per_tap_and_sentinel():
    src = np.full((3, 4), 200, np.uint8)
    b = 8
    half = (512 * 200 + 512 * b + 512) >> 10                          # two taps inside, two outside, at fx or fy = 16
    quarter = (256 * 200 + 768 * b + 512) >> 10                       # one tap inside at (16, 16)
    S = rc.MAP_SENTINEL
    m = _map_of([[-16, 32],            # x0 = -1: the left taps are outside
                 [3 * 32 + 16, 32],    # x0 = 3 = W - 1: the right taps are outside
                 [32, -16],            # y0 = -1: the upper taps
                 [32, 2 * 32 + 16],    # y0 = 2 = H - 1: the lower taps
                 [-16, -16],           # only tap (0, 0) is inside
                 [3 * 32 + 16, 2 * 32 + 16],
                 [-32, 32], [4 * 32, 32], [32, -33], [32, 3 * 32],   # wholly outside, each side
                 [-1, 32],             # x0 = -1, fx = 31: 31/32 of the pixel
                 [S, S], [100000 * 32, 5], [3 * 32, 2 * 32]])        # the sentinel; far outside; the last pixel exactly
    out = rc.remap_host(src, m, border=b)[0].tolist()
    assert out == [half, half, half, half, quarter, quarter, b, b, b, b, (32 * b + 31 * 32 * 200 + 512) >> 10, b, b, 200]
    assert rc.remap_host(src, m, border=0)[0].tolist()[6:10] == [0, 0, 0, 0]
    assert rc.remap_host(src, m, border=b).shape == (1, 14)
    with pytest.raises(ValueError):
        rc.remap_host(src, m, border=256)
    with pytest.raises(ValueError):
        rc.remap_host(src.astype(np.int16), m)
