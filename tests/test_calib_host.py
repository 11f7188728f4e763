"""The OpenCV-free calibration's host definition (deepcharuco_amd/calib.py, calibrate_camera_host_full): truth recovery, the
init formula, the extrinsics init against pnp, the Jacobian against pnp's, the block elimination against a dense solve,
optimality with noise, failed views, argument handling, the C ABI's argument checks, and (where cv2 exists) agreement with
cv2.calibrateCamera.  No GPU needed.

The scenes: a 320x240 camera whose K differs from the init's (fx 400, fy 410, cx 163.2, cy 117.5) with all five distortion
coefficients non-zero, and an 8x8-square board (49 corner ids) close enough that its corners reach the image edges (k2 and k3
are not observable from the centre of the image alone)."""
import ctypes
import math

import numpy as np
import pytest

from deepcharuco_amd import calib, pnp

SIZE = (320, 240)
K_TRUE = np.array([[400.0, 0, 163.2], [0, 410.0, 117.5], [0, 0, 1]])
DIST_TRUE = np.array([-0.25, 0.1, 1e-3, -5e-4, -0.02])
BOARD = (8, 8, 0.02)                  # 7 x 7 = 49 corners at 0.02 .. 0.14 m
N_IDS = 49
CENTRE = np.array([0.08, 0.08, 0.0])


def _theta(K, dist):
    return np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.asarray(dist, np.float64).ravel()]


def _pose(rng):
    """A view of the board, tilted 5-60 degrees, its centre near the optical axis at 0.2-0.3 m (the board spans most of the
    image)."""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    r = ax * np.deg2rad(rng.uniform(5, 60))
    R = pnp._rodrigues(r)
    t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.2, 0.3)]) - R @ CENTRE
    return r, t


def _ids(rng, full=False):
    if full:
        return np.arange(N_IDS)
    while True:
        ids = np.sort(rng.choice(N_IDS, int(rng.integers(6, N_IDS + 1)), replace=False))
        obj = pnp.object_points(ids, *BOARD)[:, :2]
        if np.linalg.matrix_rank(obj - obj.mean(0), tol=1e-6) == 2:
            return ids


def make_views(seed, n_views, sigma=0.0, K=K_TRUE, dist=DIST_TRUE, f32=True, partial=True):
    """-> (object points [float32 board corners], image points, ids, true poses [n, 6]).  f32: image points rounded to float32
    (what the corner pool holds)."""
    rng = np.random.default_rng(seed)
    objs, imgs, ids_l, poses = [], [], [], []
    k8 = pnp._dist(dist)
    for i in range(n_views):
        ids = _ids(rng, full=not partial or i % 4 == 0)
        r, t = _pose(rng)
        obj = pnp.object_points(ids, *BOARD)
        img, _, _ = pnp._project(obj.astype(np.float64), np.zeros((len(ids), 2)), np.r_[r, t], K, k8, False)
        if sigma:
            img = img + rng.normal(scale=sigma, size=img.shape)
        if f32:
            img = img.astype(np.float32)
        objs.append(obj)
        imgs.append(img)
        ids_l.append(ids)
        poses.append(np.r_[r, t])
    return objs, imgs, ids_l, np.array(poses)


def _dense_system(objs, imgs, theta, poses):
    """Full J (sum 2n_i x (9 + 6N)) and r of every view."""
    N = len(objs)
    rows, Js, rs = 0, [], []
    for i, (o, m) in enumerate(zip(objs, imgs)):
        res, _, J = calib._project_full(o.astype(np.float64), m.astype(np.float64), theta, poses[i], True)
        Jf = np.zeros((J.shape[0], 9 + 6 * N))
        Jf[:, :9] = J[:, :9]
        Jf[:, 9 + 6 * i:15 + 6 * i] = J[:, 9:]
        Js.append(Jf)
        rs.append(res.ravel())
    return np.concatenate(Js, 0), np.concatenate(rs)


def _cost(objs, imgs, theta, poses):
    return sum(calib._project_full(o.astype(np.float64), m.astype(np.float64), theta, poses[i], False)[1]
               for i, (o, m) in enumerate(zip(objs, imgs)))


def test_truth_recovery_fp64():
    objs, imgs, _, poses = make_views(1, 24, f32=False)
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert r.status == calib.CALIB_OK and (r.view_status == pnp.PNP_OK).all() and r.views_used == 24
    assert np.abs(r.camera_matrix - K_TRUE).max() <= 1e-9 * 400
    assert np.abs(r.dist_coeffs.ravel() - DIST_TRUE).max() <= 1e-9
    for i in range(24):
        assert np.linalg.norm(r.rvecs[i] - poses[i, :3]) <= 1e-9 * np.linalg.norm(poses[i, :3])
        assert np.linalg.norm(r.tvecs[i] - poses[i, 3:]) <= 1e-9 * np.linalg.norm(poses[i, 3:])
    assert r.rms <= 1e-9 and r.points_used == sum(len(o) for o in objs)


def test_truth_recovery_float32():
    """Float32 image points carry a rounding error of at most 2^-24 * 320 px ~ 1.9e-5 px (about 1e-5 px rms).  Over ~700 points
    that moves the least-squares K by well under 1e-6 relative; the gate is 1e-5 relative in K and poses, 1e-5 in dist."""
    objs, imgs, _, poses = make_views(2, 32)
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert r.status == calib.CALIB_OK
    assert np.abs(r.camera_matrix - K_TRUE).max() <= 1e-5 * 400
    assert np.abs(r.dist_coeffs.ravel() - DIST_TRUE).max() <= 1e-5
    for i in range(32):
        assert np.linalg.norm(r.rvecs[i] - poses[i, :3]) <= 1e-5 * np.linalg.norm(poses[i, :3])
        assert np.linalg.norm(r.tvecs[i] - poses[i, 3:]) <= 1e-5 * np.linalg.norm(poses[i, 3:])
    assert r.rms <= 2e-5
    assert np.all(np.abs(r.view_rms) <= 2e-5) and r.view_points.tolist() == [len(o) for o in objs]
    # cv2's 5-tuple
    rms, K, dist, rvecs, tvecs = calib.calibrate_camera_host(objs, imgs, SIZE)
    assert rms == r.rms and np.array_equal(K, r.camera_matrix) and dist.shape == (1, 5)
    assert len(rvecs) == 32 and rvecs[0].shape == (3, 1) and np.array_equal(tvecs[5].ravel(), r.tvecs[5])


def test_init_formula_is_exact_without_distortion():
    """With zero distortion and the principal point exactly at ((w-1)/2, (h-1)/2) every homography is exact, and the init's
    two rows per view are exact constraints on (1/fx^2, 1/fy^2)."""
    K = np.array([[400.0, 0, (SIZE[0] - 1) / 2], [0, 410.0, (SIZE[1] - 1) / 2], [0, 0, 1]])
    objs, imgs, _, _ = make_views(3, 20, K=K, dist=np.zeros(5), f32=False)
    views = calib._views(objs, imgs)
    st, theta0, _ = calib._initialise(views, SIZE)
    assert (st == pnp.PNP_OK).all()
    assert np.abs(theta0[:4] - _theta(K, np.zeros(5))[:4]).max() <= 1e-9 * 400 and not theta0[4:].any()


def test_extrinsics_init_is_pnp_with_k0():
    objs, imgs, ids_l, _ = make_views(4, 20)
    views = calib._views(objs, imgs)
    st, theta0, P0 = calib._initialise(views, SIZE)
    K0, _ = calib._camera_of(theta0)
    for i in range(20):
        kp = np.c_[imgs[i].astype(np.float64), ids_l[i]]
        hs, hp = pnp.solve_pnp_host_full(kp, *BOARD, K0, np.zeros(5))
        assert st[i] == hs == pnp.PNP_OK
        assert np.array_equal(P0[i].view(np.uint64), hp[:6].view(np.uint64))


def test_extrinsic_jacobian_columns_are_pnps():
    objs, imgs, _, poses = make_views(5, 6, sigma=0.3)
    theta = _theta(K_TRUE, DIST_TRUE) * 1.01
    K, k = calib._camera_of(theta)
    for i in range(6):
        o, m = objs[i].astype(np.float64), imgs[i].astype(np.float64)
        res, cost, J = calib._project_full(o, m, theta, poses[i] + 1e-3, True)
        res_p, cost_p, J_p = pnp._project(o, m, poses[i] + 1e-3, K, k, True)
        assert np.array_equal(J[:, 9:].view(np.uint64), J_p.view(np.uint64))
        assert np.array_equal(res, res_p) and cost == cost_p


def test_intrinsic_jacobian_matches_finite_differences():
    objs, imgs, _, poses = make_views(6, 3, sigma=0.3)
    theta = _theta(K_TRUE, DIST_TRUE)
    o, m = objs[0].astype(np.float64), imgs[0].astype(np.float64)
    _, _, J = calib._project_full(o, m, theta, poses[0], True)
    for j in range(9):
        h = 1e-6 * max(1.0, abs(theta[j]))
        d = np.zeros(9)
        d[j] = h
        fd = (calib._project_full(o, m, theta + d, poses[0], False)[0]
              - calib._project_full(o, m, theta - d, poses[0], False)[0]).ravel() / (2 * h)
        assert np.abs(fd - J[:, j]).max() <= 1e-6 * max(np.abs(J[:, j]).max(), 1.0), j


@pytest.mark.parametrize("n_views,lg", [(4, -3), (5, 2), (6, 0)])
def test_block_elimination_equals_dense_solve(n_views, lg):
    objs, imgs, _, poses = make_views(7 + n_views, n_views, sigma=0.3)
    theta = _theta(K_TRUE, DIST_TRUE) * 1.02
    P = poses + 1e-3
    views = calib._views(objs, imgs)
    U, W, V, ga, gb, _ = calib._normal_blocks(views, theta, P)
    dt, dp = calib._schur_step(U, W, V, ga, gb, lg)
    J, r = _dense_system(objs, imgs, theta, P)
    A = J.T @ J
    A[np.diag_indices(A.shape[0])] *= 1.0 + 10.0 ** lg
    x = np.linalg.solve(A, J.T @ r)
    got = np.r_[dt, dp.ravel()]
    assert np.linalg.norm(got - x) <= 1e-12 * np.linalg.norm(x)


def test_optimality_with_noise():
    """sigma = 0.3 px: at the result the gradient J^T r vanishes relative to |J| |r| and the cost is no higher than at the
    truth; whatever the init or the LM details, only a least-squares minimum passes this."""
    objs, imgs, _, poses = make_views(20, 30, sigma=0.3)
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert r.status == calib.CALIB_OK
    theta = _theta(r.camera_matrix, r.dist_coeffs)
    P = np.c_[r.rvecs, r.tvecs]
    J, res = _dense_system(objs, imgs, theta, P)
    assert np.linalg.norm(J.T @ res) <= 1e-9 * np.linalg.norm(J) * np.linalg.norm(res)
    cost, cost_true = _cost(objs, imgs, theta, P), _cost(objs, imgs, _theta(K_TRUE, DIST_TRUE), poses)
    assert cost <= cost_true
    assert abs(r.rms - math.sqrt(cost / r.points_used)) <= 1e-12 * r.rms
    assert 0.3 < r.rms < 0.5 and r.iterations >= 1 and r.attempts >= r.iterations
    assert np.abs(r.camera_matrix - K_TRUE).max() <= 2.0                     # px: the noise moves K, not by much


def test_failed_views_are_excluded_and_reported():
    objs, imgs, _, _ = make_views(30, 20, sigma=0.3)
    base = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    col = np.arange(7) * 7                                    # a board column: collinear
    o_col = pnp.object_points(col, *BOARD)
    m_col = imgs[0][:7] * 0 + np.c_[np.linspace(20, 300, 7), np.linspace(30, 200, 7)].astype(np.float32)
    objs2 = [objs[0][:3], objs[0][:0]] + objs[:10] + [o_col] + objs[10:]
    imgs2 = [imgs[0][:3], imgs[0][:0]] + imgs[:10] + [m_col] + imgs[10:]
    r = calib.calibrate_camera_host_full(objs2, imgs2, SIZE)
    assert r.view_status.tolist() == [pnp.PNP_TOO_FEW] * 2 + [pnp.PNP_OK] * 10 + [pnp.PNP_DEGENERATE] + [pnp.PNP_OK] * 10
    assert r.view_points.tolist()[:3] == [3, 0, len(objs[0])] and r.views_used == 20
    keep = np.flatnonzero(r.view_status == pnp.PNP_OK)
    for a, b in ((r.camera_matrix, base.camera_matrix), (r.dist_coeffs, base.dist_coeffs), (r.rvecs[keep], base.rvecs),
                 (r.tvecs[keep], base.tvecs), (r.view_rms[keep], base.view_rms)):
        assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    assert r.rms == base.rms and (r.iterations, r.attempts) == (base.iterations, base.attempts)
    assert not r.rvecs[[0, 1, 12]].any() and not r.view_rms[[0, 1, 12]].any()
    with pytest.raises(ValueError):
        calib.calibrate_camera_host(objs2, imgs2, SIZE)
    nv = calib.calibrate_camera_host_full(objs2[:2], imgs2[:2], SIZE)
    assert nv.status == calib.CALIB_NO_VIEWS and nv.views_used == 0
    with pytest.raises(ValueError):
        calib.calibrate_camera_host(objs2[:2], imgs2[:2], SIZE)


def test_argument_errors():
    objs, imgs, _, _ = make_views(40, 4)
    bad = [o.copy() for o in objs]
    bad[1][0, 2] = 0.01
    with pytest.raises(ValueError, match="planar"):
        calib.calibrate_camera_host_full(bad, imgs, SIZE)
    with pytest.raises(ValueError, match="planar"):
        calib.calibrate_camera_host(bad, imgs, SIZE)
    with pytest.raises(ValueError):
        calib.calibrate_camera_host_full(objs, imgs[:3], SIZE)
    with pytest.raises(ValueError):
        calib.calibrate_camera_host_full([objs[0][:5]], [imgs[0][:6]], SIZE)
    for size in ((0, 240), (320, -1)):
        with pytest.raises(ValueError):
            calib.calibrate_camera_host_full(objs, imgs, size)


def test_null_abi_arguments_are_rejected_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    assert lib.dcx_calibrate_workspace_bytes(0) == 0
    ws = lib.dcx_calibrate_workspace_bytes(4)
    assert ws > 0 and lib.dcx_calibrate_workspace_bytes(128) > lib.dcx_calibrate_workspace_bytes(64) > ws
    res = (ctypes.c_double * 16)()
    p = 4096              # a non-null address that is never read: every call below fails a check before any device access
    args = [p, p, p, p, 4, 16, 8, 8, 0.02, 320, 240, p, ws, p, p, res, None]
    for i in (0, 1, 2, 11, 13, 14, 15):                # null counts, starts, rows, workspace, status, pose, h_result
        a = list(args)
        a[i] = None
        assert lib.dcx_calibrate_pool(*a) == -1, i
    for i, v in ((4, 0), (5, -1), (6, 1), (7, 1), (8, float("nan")), (9, 0), (10, 0)):
        a = list(args)
        a[i] = v
        assert lib.dcx_calibrate_pool(*a) == -1, i
    a = list(args)
    a[12] = ws - 1                                     # workspace too small
    assert lib.dcx_calibrate_pool(*a) == -3


def test_matches_cv2_where_available():
    cv2 = pytest.importorskip("cv2")
    objs, imgs, _, _ = make_views(50, 24, sigma=0.3)
    rms, K, dist, _, _ = cv2.calibrateCamera([o.reshape(-1, 1, 3) for o in objs], [m.reshape(-1, 1, 2) for m in imgs], SIZE,
                                             None, None)
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert abs(r.rms - rms) <= 1e-6 * rms
    assert np.abs(r.camera_matrix - K).max() <= 1e-4 * 400
    assert np.abs(r.dist_coeffs - dist.reshape(1, -1)[:, :5]).max() <= 1e-4
