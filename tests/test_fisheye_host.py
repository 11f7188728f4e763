"""The host definitions of the fisheye model (deepcharuco_amd/fisheye.py) against tests/fisheye_exact.py, an independent
restatement in extended precision: the model and its inverse, the analytic Jacobians against central differences of the exact
projection, the pose solver and the calibration on noise-free exact scenes, the pinhole limit, a view outside the start camera's
field, and the map's edge cases.  No GPU.

Bounds, from the formats and the reference's own error:
* model: a pixel is a sum of ~20 fp64 operations on values up to 640: 1e-10 px;
* inverse: Newton stops at a step below 1e-15 in theta, and d tan(theta) / d theta <= 1 / cos^2(56 deg) = 3.2 here: 1e-12;
* Jacobians: the differences' own truncation and rounding are ~1e-12 of a column (fisheye_exact.jacobian_fd): 1e-9 of a column;
* recovery from float32 pixels: a pixel below 640 is rounded by at most 3.1e-5 px, rms 1.8e-5 at the most: rms <= 2e-5 px; the
  parameters move by that noise times the problem's conditioning, gated at 1e-3 px for K, 1e-4 for k and 1e-5 relative for poses.
"""
import numpy as np
import pytest

import camera_exact as cx
import fisheye_exact as fx
from camera_exact import f64
from deepcharuco_amd import calib, fisheye as fe, pnp, rectify as rc

CAMS = [(fx.camera(150.0, 152.0, off=(4.0, -3.0)), fx.K_ZERO), (fx.camera(150.0, 152.0, off=(4.0, -3.0)), fx.K_LENS),
        (fx.camera(400.0, 395.0, off=(4.0, -3.0)), fx.K_ZERO), (fx.camera(400.0, 395.0, off=(4.0, -3.0)), fx.K_LENS)]
CAM_IDS = ["f150_k0", "f150_k", "f400_k0", "f400_k"]


def _axis_points():
    """Camera-frame points at pose zero: on the axis, at r = 1e-12, below and above the series threshold, out to 80 degrees."""
    r = np.array([0.0, 1e-12, 1e-7, 0.99e-4, 1.01e-4, 1e-3, 0.1, 1.0, np.tan(np.deg2rad(80.0))])
    ang = np.linspace(0.3, 5.0, r.size)
    return np.stack([r * np.cos(ang), r * np.sin(ang), np.ones_like(r)], 1)


def test_exact_model_is_pinned_by_mpmath():
    K, k = CAMS[1]
    obj = _axis_points()
    for p in (np.zeros(6), np.array([0.2, -0.3, 0.1, 0.01, -0.02, 0.05])):
        got = fx.project(obj, p, K, k)
        want = fx.project_mp(obj, p, K, k)
        err = max(abs(float(got[i, j]) - float(want[i][j])) for i in range(len(obj)) for j in range(2))
        print("longdouble against 40-digit mpmath, px:", err)
        assert err <= 1e-15 * 640                        # a 64-bit mantissa on values up to 640 px


@pytest.mark.parametrize("K,k", CAMS, ids=CAM_IDS)
def test_host_model_against_the_exact_one(K, k):
    obj = _axis_points()
    p0 = np.zeros(6)
    got = fe.project_points_host(obj, p0[:3], p0[3:], K, k)
    want = f64(fx.project(obj, p0, K, k))
    print("on-axis and tiny-r points, px:", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-10
    assert np.array_equal(got[0], [K[0, 2], K[1, 2]])                        # the optical axis is the principal point
    objs, _, _, poses = fx.make_views(5, 6, K, k)
    for o, p in zip(objs, poses):
        got = fe.project_points_host(o, p[:3], p[3:], K, k)
        assert np.abs(got - f64(fx.project(o, p, K, k))).max() <= 1e-10
    behind = fe.project_points_host(np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]), np.zeros(3), np.zeros(3), K, k)
    assert np.isnan(behind[0]).all() and np.isfinite(behind[1]).all()


@pytest.mark.parametrize("K,k", CAMS, ids=CAM_IDS)
def test_undistort_inverts_project(K, k):
    obj = _axis_points()
    pix = f64(fx.project(obj, np.zeros(6), K, k))
    n = fe.undistort_points_host(pix, K, k)
    gap = np.abs(n - obj[:, :2])
    print("undistort(project) - identity, per point:", gap.max(1))
    assert gap[:-1].max() <= 1e-12                       # theta <= 45 degrees
    assert gap[-1].max() <= 1e-12 / np.cos(np.deg2rad(80.0)) ** 2            # 80 degrees: d tan / d theta = 33
    objs, _, _, poses = fx.make_views(6, 4, K, k)
    for o, p in zip(objs, poses):
        X = cx.camera_points(o, p)
        n = fe.undistort_points_host(f64(fx.project(o, p, K, k)), K, k)
        assert np.abs(n - np.stack([f64(X[0] / X[2]), f64(X[1] / X[2])], 1)).max() <= 1e-12


def test_undistort_outside():
    K = fx.camera(150.0)
    pix = np.array([[K[0, 2], K[1, 2]], [K[0, 2] + 150.0 * 1.5, K[1, 2]], [K[0, 2] + 150.0 * 1.6, K[1, 2]], [np.nan, 0.0]])
    n = fe.undistort_points_host(pix, K, None)           # k = 0: theta = theta_d; pi / 2 = 1.5708
    assert np.array_equal(n[0], [0.0, 0.0]) and np.isfinite(n[1]).all() and np.isnan(n[2]).all() and np.isnan(n[3]).all()
    assert abs(n[1, 0] - np.tan(1.5)) <= 1e-12 * np.tan(1.5) / np.cos(1.5) ** 2
    with pytest.raises(ValueError):
        fe.undistort_points_host(pix, K, np.zeros(5))
    skew = K.copy()
    skew[0, 1] = 0.1
    with pytest.raises(ValueError):
        fe.undistort_points_host(pix, skew, None)


@pytest.mark.parametrize("K,k", CAMS, ids=CAM_IDS)
def test_analytic_jacobians_against_exact_differences(K, k):
    """Pose, intrinsic and k columns, on scene views and on the on-axis / tiny-r points (both sides of the series threshold)."""
    objs, _, _, poses = fx.make_views(7, 3, K, k)
    cases = list(zip(objs, poses)) + [(_axis_points()[:, :3] - [0, 0, 1.0], np.array([0, 0, 0, 0, 0, 1.0]))]
    worst = 0.0
    for o, p in cases:
        o = np.asarray(o, np.float64)
        _, J = fe.project_points_host(o, p[:3], p[3:], K, k, jacobian=True)
        Jfd = fx.jacobian_fd(o, p, K, k)
        col = np.maximum(np.abs(Jfd).max(0), 1e-300)
        worst = max(worst, float((np.abs(J - Jfd) / col).max()))
    print("analytic - central differences, relative to the column:", worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("K,k", CAMS, ids=CAM_IDS)
def test_pose_and_calibration_recover_exact_scenes(K, k):
    objs, imgs, ids_l, poses = fx.make_views(11, 12, K, k)
    for kp, p in zip(fx.keypoints(imgs, ids_l), poses):
        st, pose = fe.solve_pnp_fisheye_host_full(kp, *fx.BOARD, K, k)
        assert st == pnp.PNP_OK and pose[6] <= 2e-5
        assert np.linalg.norm(pose[:3] - p[:3]) <= 1e-5 * np.linalg.norm(p[:3])
        assert np.linalg.norm(pose[3:6] - p[3:]) <= 1e-5 * np.linalg.norm(p[3:])
    r = fe.calibrate_fisheye_host_full(objs, imgs, fx.SIZE)
    print(f"fx {K[0, 0]} k1 {k[0]}: rms {r.rms:.3e} steps {r.iterations} attempts {r.attempts} |K - K*| "
          f"{np.abs(r.camera_matrix - K).max():.3e} |k - k*| {np.abs(r.dist_coeffs.ravel() - k).max():.3e}")
    assert r.status == calib.CALIB_OK and (r.view_status == pnp.PNP_OK).all() and r.iterations < fe.CALIB_MAX_ITER
    assert r.dist_coeffs.shape == (1, 4) and r.views_used == 12 and r.points_used == 12 * 28
    assert r.rms <= 2e-5
    assert np.abs(r.camera_matrix - K).max() <= 1e-3 and np.abs(r.dist_coeffs.ravel() - k).max() <= 1e-4
    assert np.all(np.linalg.norm(r.rvecs - poses[:, :3], axis=1) <= 1e-5 * np.linalg.norm(poses[:, :3], axis=1))
    assert np.all(np.linalg.norm(r.tvecs - poses[:, 3:], axis=1) <= 1e-5 * np.linalg.norm(poses[:, 3:], axis=1))
    rms, Kc, D, rv, tv = fe.calibrate_fisheye_host(objs, imgs, fx.SIZE, focal0=K[0, 0] * 1.1)      # a given start, cv2's tuple
    assert D.shape == (1, 4) and len(rv) == len(tv) == 12 and np.abs(Kc - K).max() <= 1e-3 and rms <= 2e-5


def test_k_zero_and_small_theta_agree_with_the_pinhole_solver():
    """The board (half diagonal 0.14 m) at 4 m or more: theta <= 0.035.  With k = 0, theta_d = theta falls short of the pinhole's
    tan(theta) by theta^2 / 3 relative, so a fisheye pixel rho from the centre lies within G = rho theta^2 / 3 of the pinhole's
    at the same pose.  The pinhole solver minimises its rms residual and the true pose offers it one of G at the most; the
    fisheye solver fits the pixels to their float32 rounding (2e-5 px).  So the two poses, each projected through its own
    model, agree to G + 2e-5 px rms: the stated bound.  (The rotation vectors themselves are not comparable at that size: a
    tilt is read from a foreshortening of 0.035 relative, and G is 1 % of that.)"""
    K = fx.camera(40000.0)
    rng = np.random.default_rng(3)
    obj = cx.board_points(np.arange(28), *fx.BOARD)
    for _ in range(3):
        p = fx.random_pose(rng, fx.BOARD, (4.0, 5.0), lateral=0.0)
        pix = f64(fx.project(obj, p, K, fx.K_ZERO))
        kp = np.c_[pix.astype(np.float32), np.arange(28)]
        sf, pf = fe.solve_pnp_fisheye_host_full(kp, *fx.BOARD, K, None)
        sp, pp = pnp.solve_pnp_host_full(kp, *fx.BOARD, K, None)
        assert sf == sp == pnp.PNP_OK
        rho = np.hypot(pix[:, 0] - K[0, 2], pix[:, 1] - K[1, 2])
        bound = float(np.max(rho * (rho / 40000.0) ** 2 / 3.0)) + 2e-5
        a = fe.project_points_host(obj, pf[:3], pf[3:6], K, None)
        b = f64(cx.project(obj, pp[:6], K, None))
        gap = float(np.sqrt(((a - b) ** 2).sum(1).mean()))
        print(f"fisheye k = 0 against pinhole at small theta: {gap:.3e} px rms, bound {bound:.3e}")
        assert gap <= bound


def test_a_view_beyond_the_start_cameras_field_is_left_out():
    """True focal 150 px, start focal 90 px: a pixel more than 90 pi / 2 = 141.4 px from the centre has theta_d > pi / 2 at the start
    camera (k = 0 there)."""
    K, k = CAMS[1]
    objs, imgs, ids_l, _ = fx.make_views(11, 12, K, k)
    far = [i for i, m in enumerate(imgs) if np.hypot(m[:, 0] - 319.5, m[:, 1] - 239.5).max() > 90.0 * np.pi / 2]
    assert 0 < len(far) < 12                             # a condition on the input
    r = fe.calibrate_fisheye_host_full(objs + [objs[0][:3]], imgs + [imgs[0][:3]], fx.SIZE, focal0=90.0)
    want = [pnp.PNP_DEGENERATE if i in far else pnp.PNP_OK for i in range(12)] + [pnp.PNP_TOO_FEW]
    assert r.view_status.tolist() == want and r.views_used == 12 - len(far)
    assert not r.rvecs[far].any() and not r.view_rms[far].any()
    st, pose = fe.solve_pnp_fisheye_host_full(fx.keypoints(imgs, ids_l)[far[0]], *fx.BOARD, fx.camera(90.0), None)
    assert st == pnp.PNP_DEGENERATE and not pose.any()
    none = fe.calibrate_fisheye_host_full([o[:3] for o in objs], [m[:3] for m in imgs], fx.SIZE)
    assert none.status == calib.CALIB_NO_VIEWS and none.rms == 0.0
    with pytest.raises(ValueError):
        fe.calibrate_fisheye_host(objs + [objs[0][:3]], imgs + [imgs[0][:3]], fx.SIZE)


def test_map_edge_cases():
    K, k = CAMS[1]
    one = fe.undistort_rectify_map_fisheye_host(K, k, None, None, 1, 1)
    assert one.shape == (1, 1, 2) and one.dtype == np.int32
    want = f64(fx.distort(np.array([-K[0, 2] / K[0, 0]]), np.array([-K[1, 2] / K[1, 1]]), K, k))[0]
    assert np.abs(one[0, 0] - 32.0 * want).max() <= 0.5 + 1e-6
    # q_z <= 0: a rotation of 100 degrees about y puts one side of the output behind the camera
    R100 = f64(cx.rotation([0.0, np.deg2rad(100.0), 0.0]))
    P = np.array([[20.0, 0, 32.0], [0, 20.0, 24.0], [0, 0, 1]])
    m = fe.undistort_rectify_map_fisheye_host(K, k, R100, P, 64, 48)
    fl = fe.undistort_rectify_map_fisheye_host(K, k, R100, P, 64, 48, quantised=False)
    out = m[..., 0] == rc.MAP_SENTINEL
    assert out.any() and not out.all() and np.array_equal(out, m[..., 1] == rc.MAP_SENTINEL) and np.array_equal(out, np.isnan(fl[..., 0]))
    x = (np.arange(64) - 32.0) / 20.0
    qz = R100[0, 2] * x[None, :] + R100[1, 2] * ((np.arange(48) - 24.0) / 20.0)[:, None] + R100[2, 2]
    assert np.array_equal(out, ~(qz > 0))
    # beyond MAP_LIMIT: a focal length of 1e6 px sends every pixel but the centre's neighbourhood past 2^15 px
    big = fe.undistort_rectify_map_fisheye_host(fx.camera(1e6), None, None, fx.camera(100.0), 640, 480, quantised=False)
    assert np.isnan(big[0, 0]).all() and np.isfinite(big[240, 320]).all()
    assert np.nanmax(np.abs(big)) <= rc.MAP_LIMIT
    pts = fe.rectify_points_fisheye_host(np.array([[250.0, 240.0], [400.0, 240.0]]), K, k, R100, P)
    n = fe.undistort_points_host(np.array([[250.0, 240.0], [400.0, 240.0]]), K, k)
    z = R100[2, 0] * n[:, 0] + R100[2, 1] * n[:, 1] + R100[2, 2]
    assert np.array_equal(np.isnan(pts[:, 0]), ~(z > 0)) and np.isnan(pts).any() and np.isfinite(pts).any()
