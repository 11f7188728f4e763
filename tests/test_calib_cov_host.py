"""The host definition of the calibration uncertainty (deepcharuco_amd/calib.py calibration_uncertainty_host, fisheye.py
calibration_uncertainty_fisheye_host, _lm.schur_covariance): the Schur form against the inverse of the dense normal matrix and
against a pseudo-inverse of the stacked Jacobian that forms no normal equations, sigma^2 against the noise that was put in, masks,
statuses and refusals, and the CalibResult / RobustCalibResult overloads.  No GPU needed.

The gate of the first test, 1000 * cond(S) * 2^-52 relative to the largest entry compared, is the forward error of inverting a
matrix of that condition in float64 with three decimal digits of room; the test computes cond(S) itself (about 2e7 on these
scenes, so a gate of about 4e-6; the gaps printed are of the order of 1e-12)."""
import numpy as np
import pytest

import fisheye_exact as fx
from deepcharuco_amd import _lm, calib, fisheye as fe, pnp
from test_calib_host import BOARD, DIST_TRUE, K_TRUE, SIZE, make_views

SIGMA = 0.3
FE_K, FE_DIST = fx.camera(150.0, 152.0, off=(4.0, -3.0)), fx.K_LENS

MODELS = {
    "pinhole": (calib.calibration_uncertainty_host, calib._project_full, 9),
    "fisheye": (fe.calibration_uncertainty_fisheye_host, fe._project_full, 8),
}


def _scene(model, n_views, sigma=SIGMA):
    """-> (objs, imgs float32, the host calibration of them)."""
    if model == "pinhole":
        objs, imgs, _, _ = make_views(520 + n_views, n_views, sigma=sigma)
        return objs, imgs, calib.calibrate_camera_host_full(objs, imgs, SIZE)
    objs, imgs, _, _ = fx.make_views(520 + n_views, n_views, FE_K, FE_DIST, sigma=sigma)
    return objs, imgs, fe.calibrate_fisheye_host_full(objs, imgs, fx.SIZE)


_SOLVED = {}


def solved(model, n_views):
    """One calibration per (model, views), shared by the tests and left unchanged."""
    key = (model, n_views)
    if key not in _SOLVED:
        objs, imgs, r = _scene(model, n_views)
        assert r.status == calib.CALIB_OK and r.views_used == n_views
        _SOLVED[key] = (objs, imgs, r)
    return _SOLVED[key]


def _theta(r):
    K = r.camera_matrix
    return np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], r.dist_coeffs.ravel()]


def _same_bits(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        else:
            assert x == y


@pytest.mark.parametrize("n_views", [8, 24])
@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_schur_form_against_the_dense_inverse_and_the_pseudo_inverse(model, n_views):
    fn, project_full, ng = MODELS[model]
    objs, imgs, r = solved(model, n_views)
    u = fn(objs, imgs, r)
    assert u.status == calib.COV_OK and u.views == n_views and u.points == r.points_used
    assert u.dof == 2 * u.points - ng - 6 * n_views
    theta, poses = _theta(r), np.c_[r.rvecs, r.tvecs]
    views = [(o.astype(np.float64), m.astype(np.float64)) for o, m in zip(objs, imgs)]
    U, W, V, _, _, costs = calib._normal_blocks(views, theta, poses, project_full)
    assert u.sigma2 == calib._total(costs) / u.dof
    N = ng + 6 * n_views
    A = np.zeros((N, N))
    A[:ng, :ng] = V
    rows = []
    for i, (o, m) in enumerate(views):
        s = slice(ng + 6 * i, ng + 6 * i + 6)
        A[:ng, s], A[s, :ng], A[s, s] = W[i], W[i].T, U[i]
        J = project_full(o, m, theta, poses[i], True)[2]
        Jf = np.zeros((J.shape[0], N))
        Jf[:, :ng], Jf[:, s] = J[:, :ng], J[:, ng:]
        rows.append(Jf)
    S = V - sum(W[i] @ np.linalg.solve(U[i], W[i].T) for i in range(n_views))
    cond = float(np.linalg.cond(S))
    gate = 1000.0 * cond * 2.0 ** -52
    dense = u.sigma2 * np.linalg.inv(A)
    gaps = {"cov_intrinsics": float(np.abs(dense[:ng, :ng] - u.cov_intrinsics).max() / np.abs(dense[:ng, :ng]).max())}
    blocks = np.array([dense[ng + 6 * i:ng + 6 * i + 6, ng + 6 * i:ng + 6 * i + 6] for i in range(n_views)])
    gaps["cov_extrinsics"] = float(np.abs(blocks - u.cov_extrinsics).max() / np.abs(blocks).max())
    Jp = np.linalg.pinv(np.concatenate(rows, 0))
    d = u.sigma2 * np.einsum("ij,ij->i", Jp, Jp)                      # diag(pinv(J) pinv(J)^T): no normal equations formed
    mine = np.r_[np.diag(u.cov_intrinsics), np.diagonal(u.cov_extrinsics, axis1=1, axis2=2).ravel()]
    gaps["pinv diagonal, intrinsics"] = float(np.abs(d[:ng] - mine[:ng]).max() / d[:ng].max())
    gaps["pinv diagonal, poses"] = float(np.abs(d[ng:] - mine[ng:]).max() / d[ng:].max())
    print(f"{model}, {n_views} views: cond(S) {cond:.3g}, gate {gate:.3g}, gaps {gaps}")
    assert max(gaps.values()) <= gate, (gaps, gate)
    assert np.array_equal(u.std_intrinsics, np.sqrt(np.diag(u.cov_intrinsics)))
    assert np.array_equal(u.std_extrinsics, np.sqrt(np.diagonal(u.cov_extrinsics, axis1=1, axis2=2)))
    assert np.array_equal(u.cov_intrinsics, u.cov_intrinsics.T)
    assert np.array_equal(u.cov_extrinsics, u.cov_extrinsics.transpose(0, 2, 1))


def test_schur_covariance_is_generic_in_the_global_size():
    """_lm.schur_covariance on random blocks with 6 global parameters (the stereo solve's size) against the dense inverse."""
    rng = np.random.default_rng(3)
    n, N = 6, 5
    J = rng.normal(size=(N, 40, n + 6))
    U = np.einsum("nri,nrj->nij", J[:, :, n:], J[:, :, n:])
    W = np.einsum("nri,nrj->nij", J[:, :, :n], J[:, :, n:])
    V = np.einsum("nri,nrj->ij", J[:, :, :n], J[:, :, :n])
    Si, P = _lm.schur_covariance(U, W, V, np.ones(N))
    A = np.zeros((n + 6 * N, n + 6 * N))
    A[:n, :n] = V
    for i in range(N):
        s = slice(n + 6 * i, n + 6 * i + 6)
        A[:n, s], A[s, :n], A[s, s] = W[i], W[i].T, U[i]
    inv = np.linalg.inv(A)
    gate = 1000.0 * np.linalg.cond(A) * 2.0 ** -52
    assert np.abs(inv[:n, :n] - Si).max() <= gate * np.abs(inv).max()
    for i in range(N):
        s = slice(n + 6 * i, n + 6 * i + 6)
        assert np.abs(inv[s, s] - P[i]).max() <= gate * np.abs(inv).max()
    U[2] = -U[2]
    assert _lm.schur_covariance(U, W, V, np.ones(N)) is None
    U[2] = -U[2]
    assert _lm.schur_covariance(U, W, V, np.r_[np.ones(N - 1), np.inf]) is None


def renoised(draws, seed=7, sigma=SIGMA):
    """The 24 clean views make_views(524, 24, sigma=0, f32=False) (818 points) -> (objs, ids, ``draws`` sets of image points:
    the clean ones plus noise of ``sigma`` px from default_rng(seed), drawn in order, each rounded to float32)."""
    objs, clean, ids_l, _ = make_views(524, 24, sigma=0.0, f32=False)
    rng = np.random.default_rng(seed)
    return objs, ids_l, [[(m + rng.normal(scale=sigma, size=m.shape)).astype(np.float32) for m in clean] for _ in range(draws)]


def test_sigma2_recovers_the_noise():
    """24 views at 0.3 px, dof = 1,483: sigma^2 / 0.09 within 1 +- 4 sqrt(2 / dof) = +-0.147, four standard deviations of a
    chi-square over its dof.  Measured: sigma^2 0.0861, ratio 0.957."""
    objs, _, (imgs,) = renoised(1)
    u = calib.calibration_uncertainty_host(objs, imgs, calib.calibrate_camera_host_full(objs, imgs, SIZE))
    half = 4.0 * np.sqrt(2.0 / 1483)
    print(f"sigma2 {u.sigma2:.6f}, ratio {u.sigma2 / SIGMA ** 2:.4f}, dof {u.dof}, allowed 1 +- {half:.4f}")
    assert u.status == calib.COV_OK and u.dof == 1483 and u.points == 818
    assert abs(u.sigma2 / SIGMA ** 2 - 1.0) <= half


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_masks(model):
    fn = MODELS[model][0]
    objs, imgs, r = solved(model, 8)
    rng = np.random.default_rng(11)
    masks = [rng.random(len(o)) < 0.8 for o in objs]
    masks[3][:] = True
    assert all(m.sum() >= 6 for m in masks) and not all(m.all() for m in masks)
    args = (r.camera_matrix, r.dist_coeffs, r.rvecs, r.tvecs)
    masked = fn(objs, imgs, *args, inliers=masks)
    removed = fn([o[m] for o, m in zip(objs, masks)], [i[m] for i, m in zip(imgs, masks)], *args)
    assert masked.status == calib.COV_OK and masked.points == sum(int(m.sum()) for m in masks)
    _same_bits(masked, removed)
    _same_bits(fn(objs, imgs, *args, inliers=[np.ones(len(o), bool) for o in objs]), fn(objs, imgs, *args))


def _zero_but_counts(u, ng, B):
    assert u.sigma2 == 0.0 and not u.std_intrinsics.any() and not u.cov_intrinsics.any()
    assert not u.std_extrinsics.any() and not u.cov_extrinsics.any()
    assert u.std_intrinsics.shape == (ng,) and u.cov_intrinsics.shape == (ng, ng)
    assert u.std_extrinsics.shape == (B, 6) and u.cov_extrinsics.shape == (B, 6, 6)


def test_statuses():
    objs, imgs, ids_l, poses = make_views(77, 2, sigma=0.0, f32=False, partial=False)     # all 49 ids, the true poses
    K, dist = K_TRUE, DIST_TRUE
    five = [0, 6, 24, 42, 48]                                         # the board's corners and its centre
    o5, i5 = [o[five] for o in objs], [i[five] for i in imgs]
    u = calib.calibration_uncertainty_host(o5, i5, K, dist, poses[:, :3], poses[:, 3:])
    assert (u.status, u.dof, u.points, u.views) == (calib.COV_NO_DOF, -1, 10, 2)      # 20 residuals, 21 parameters
    _zero_but_counts(u, 9, 2)

    u = calib.calibration_uncertainty_host(objs, imgs, K, dist, poses[:, :3], poses[:, 3:], view_status=[pnp.PNP_TOO_FEW] * 2)
    assert (u.status, u.points, u.views) == (calib.COV_NO_VIEWS, 0, 0)
    _zero_but_counts(u, 9, 2)

    back = poses.copy()
    back[1, 5] = -back[1, 5]                                          # the board behind the camera
    u = calib.calibration_uncertainty_host(objs, imgs, K, dist, back[:, :3], back[:, 3:])
    assert (u.status, u.views) == (calib.COV_SINGULAR, 2) and u.dof > 0
    _zero_but_counts(u, 9, 2)
    nan = poses.copy()
    nan[0, 1] = np.nan
    assert calibration_status(objs, imgs, K, dist, nan) == calib.COV_SINGULAR


def calibration_status(objs, imgs, K, dist, poses):
    return calib.calibration_uncertainty_host(objs, imgs, K, dist, poses[:, :3], poses[:, 3:]).status


def test_unused_views_get_zeros():
    objs, imgs, r = solved("pinhole", 8)
    st = r.view_status.copy()
    st[[1, 5]] = pnp.PNP_DEGENERATE
    u = calib.calibration_uncertainty_host(objs, imgs, r.camera_matrix, r.dist_coeffs, r.rvecs, r.tvecs, view_status=st)
    assert u.status == calib.COV_OK and u.views == 6 and u.points == sum(len(o) for i, o in enumerate(objs) if i not in (1, 5))
    assert not u.cov_extrinsics[[1, 5]].any() and not u.std_extrinsics[[1, 5]].any()
    assert (u.std_extrinsics[[0, 2, 3, 4, 6, 7]] > 0).all()
    keep = [0, 2, 3, 4, 6, 7]
    sub = calib.calibration_uncertainty_host([objs[i] for i in keep], [imgs[i] for i in keep], r.camera_matrix, r.dist_coeffs,
                                             r.rvecs[keep], r.tvecs[keep])
    assert np.array_equal(sub.cov_intrinsics, u.cov_intrinsics) and np.array_equal(sub.cov_extrinsics, u.cov_extrinsics[keep])


def test_refusals():
    objs, imgs, r = solved("pinhole", 8)
    for n in (0, 4, 8):
        with pytest.raises(ValueError, match="held fixed"):
            calib.calibration_uncertainty_host(objs, imgs, r.camera_matrix, np.zeros(n), r.rvecs, r.tvecs)
    with pytest.raises(ValueError, match="held fixed"):
        fe.calibration_uncertainty_fisheye_host(objs, imgs, r.camera_matrix, np.zeros(5), r.rvecs, r.tvecs)
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_host(objs, imgs, r.camera_matrix, r.dist_coeffs)                    # no poses
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_host(objs, imgs, r.camera_matrix, r.dist_coeffs, r.rvecs[:3], r.tvecs[:3])
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_host(objs, imgs, r, inliers=[np.ones(3, bool)] * 8)
    with pytest.raises(ValueError, match="failed"):
        calib.calibration_uncertainty_host(objs, imgs, r._replace(status=calib.CALIB_DEGENERATE))


def test_abi_arguments_are_refused_without_a_gpu():
    """DCX_E_ARG and DCX_E_WS come back before anything touches a device: dummy non-null addresses are never followed."""
    import ctypes
    from deepcharuco_amd import _lib
    L = _lib.lib()
    need = L.dcx_calibrate_uncertainty_workspace_bytes(3)
    assert need > 0 and L.dcx_calibrate_uncertainty_workspace_bytes(0) == 0 and L.dcx_calibrate_uncertainty_workspace_bytes(-1) == 0
    th = (ctypes.c_double * 9)(400, 410, 160, 120, 0, 0, 0, 0, 0)

    def call(counts=8, model=calib.CAMERA_PINHOLE, th=th, st=8, pose=8, ws=8, nbytes=need, g=8, p=8, batch=3):
        return L.dcx_calibrate_uncertainty_pool(counts, 8, 8, None, batch, 10, *BOARD, model, th, st, pose, None, ws, nbytes, g, p, None)

    assert call(counts=None) == -1 and call(batch=0) == -1 and call(model=2) == -1                # DCX_E_ARG
    for kw in ("th", "st", "pose", "ws", "g", "p"):
        assert call(**{kw: None}) == -1, kw
    assert call(nbytes=need - 1) == -3 and call(model=calib.CAMERA_FISHEYE, nbytes=0) == -3       # DCX_E_WS


def test_overloads():
    objs, imgs, r = solved("pinhole", 8)
    _same_bits(calib.calibration_uncertainty_host(objs, imgs, r),
               calib.calibration_uncertainty_host(objs, imgs, r.camera_matrix, r.dist_coeffs, r.rvecs, r.tvecs, r.view_status))
    _same_bits(calib.calibration_uncertainty_host(objs, imgs, r),
               calib.calibration_uncertainty_host(objs, imgs, r.camera_matrix, r.dist_coeffs, tuple(v.reshape(3, 1) for v in r.rvecs),
                                                  tuple(v.reshape(3, 1) for v in r.tvecs)))
    fobjs, fimgs, fr = solved("fisheye", 8)
    _same_bits(fe.calibration_uncertainty_fisheye_host(fobjs, fimgs, fr),
               fe.calibration_uncertainty_fisheye_host(fobjs, fimgs, fr.camera_matrix, fr.dist_coeffs, fr.rvecs, fr.tvecs,
                                                       fr.view_status))


def test_robust_result_overload_uses_its_inliers():
    """A RobustCalibResult in: its masks (caller's row order) are the rows counted."""
    objs, imgs, ids_l, _ = make_views(91, 8, sigma=SIGMA)
    kps = [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]
    for b in (1, 4):                                                  # two rows of two views carry another corner's pixels
        kps[b][[2, 3], :2] = kps[b][[3, 2], :2]
    rr = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE)
    assert rr.status == calib.CALIB_OK and int(rr.view_inliers.sum()) < sum(len(k) for k in kps)
    imgs2 = [k[:, :2].astype(np.float32) for k in kps]
    a = calib.calibration_uncertainty_host(objs, imgs2, rr)
    b = calib.calibration_uncertainty_host(objs, imgs2, rr.camera_matrix, rr.dist_coeffs, rr.rvecs, rr.tvecs, rr.view_status,
                                           rr.inliers)
    assert a.status == calib.COV_OK and a.points == rr.points_used and a.views == rr.views_used
    _same_bits(a, b)
    assert calib.calibration_uncertainty_host(objs, imgs2, rr, inliers=[np.ones(len(o), bool) for o in objs]).points > a.points
