"""The OpenCV-free PnP solver's host definition (deepcharuco_amd/pnp.py, solve_pnp_host): object points as the reference builds
them, pose recovery, optimality checks no implementation choice can fake, argument handling, and (where cv2 exists) agreement
with cv2.solvePnP.  No GPU needed."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from deepcharuco_amd import pnp
from deepcharuco_amd.inference import _pnp_points

K = np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]])
DIST5 = np.array([-0.2, 0.05, 1e-3, -1e-3, 0.0])
DIST8 = np.array([-0.2, 0.05, 1e-3, -1e-3, 0.01, 0.02, -0.01, 0.005])
BOARD = (5, 5, 0.01)


def _true_pose(rng, max_tilt_deg=60.0, min_tilt_deg=5.0):
    """A pose that keeps the 5x5 board (0.01 m squares, corners at 0.01..0.04 m) inside a 320x240 view at fx = 300."""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    r = ax * np.deg2rad(rng.uniform(min_tilt_deg, max_tilt_deg))
    R = pnp._rodrigues(r)
    z = rng.uniform(0.12, 0.2)
    t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), z]) - R @ np.array([0.025, 0.025, 0.0])
    return r, t


def _project(ids, r, t, dist):
    obj = pnp.object_points(ids, *BOARD).astype(np.float64)
    res, _, _ = pnp._project(obj, np.zeros((len(ids), 2)), np.r_[r, t], K, pnp._dist(dist), False)
    return res


def make_frame(rng, ids=None, dist=DIST5, sigma=0.0):
    """-> (keypoints (N,3) [x, y, id] as infer_image returns them, true rvec, true tvec)."""
    ids = np.arange(16) if ids is None else np.asarray(ids)
    r, t = _true_pose(rng)
    img = _project(ids, r, t, dist) + (rng.normal(scale=sigma, size=(len(ids), 2)) if sigma else 0.0)
    kp = np.c_[img.astype(np.float32).astype(np.float64), ids]
    return kp, r, t


def _cost_and_grad(kp, p, dist):
    obj, img = _pnp_points(kp, *BOARD)
    res, cost, J = pnp._project(obj.astype(np.float64), img.astype(np.float64), p, K, pnp._dist(dist), True)
    return res.ravel(), cost, J


def test_object_points_equal_the_reference_construction():
    fx = np.load(os.path.join(GOLDEN, "solve_pnp_points.npz"))
    for i in range(int(fx["n_cases"])):
        kp, (cc, rc, sq) = fx[f"kp{i}"], fx[f"board{i}"]
        want, _ = _pnp_points(kp, int(cc), int(rc), float(sq))
        got = pnp.object_points(kp[:, 2], int(cc), int(rc), float(sq))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got, fx[f"objp{i}"])


def test_object_points_bad_id_raises_like_the_reference():
    with pytest.raises(IndexError):
        pnp.object_points([0, 16], *BOARD)
    with pytest.raises(IndexError):
        _pnp_points(np.array([[0, 0, 0], [1, 1, 16]]), *BOARD)        # the reference's own behaviour


def test_recovery_noise_free():
    rng = np.random.default_rng(1234)
    for _ in range(16):
        kp, r, t = make_frame(rng)
        st, pose = pnp.solve_pnp_host_full(kp, *BOARD, K, DIST5)
        assert st == pnp.PNP_OK
        assert pose[6] <= 1e-4                                       # rms px (float32 rounding of the image points only)
        assert np.linalg.norm(pose[:3] - r) <= 1e-4 * np.linalg.norm(r)
        assert np.linalg.norm(pose[3:6] - t) <= 1e-4 * np.linalg.norm(t)
        ret, rvec, tvec = pnp.solve_pnp_host(kp, *BOARD, K, DIST5)
        assert ret is True and rvec.shape == (3, 1) and tvec.shape == (3, 1) and rvec.dtype == np.float64
        assert np.array_equal(rvec.ravel(), pose[:3]) and np.array_equal(tvec.ravel(), pose[3:6])


def test_optimality_with_noise():
    """At the returned pose the cost is no higher than at the truth and the gradient vanishes: whatever the initialisation or
    the LM details, only a least-squares minimum passes this."""
    rng = np.random.default_rng(99)
    for _ in range(16):
        kp, r, t = make_frame(rng, sigma=0.3)
        st, pose = pnp.solve_pnp_host_full(kp, *BOARD, K, DIST5)
        assert st == pnp.PNP_OK
        res, cost, J = _cost_and_grad(kp, pose[:6], DIST5)
        _, cost_true, _ = _cost_and_grad(kp, np.r_[r, t], DIST5)
        assert cost <= cost_true * (1 + 1e-9)
        assert np.linalg.norm(J.T @ res) <= 1e-6 * np.linalg.norm(J) * np.linalg.norm(res)
        assert abs(pose[6] - np.sqrt(cost / len(kp))) <= 1e-12


def test_analytic_jacobian_matches_finite_differences():
    rng = np.random.default_rng(5)
    kp, r, t = make_frame(rng, dist=DIST8, sigma=0.3)
    p = np.r_[r, t] + 1e-3
    res, _, J = _cost_and_grad(kp, p, DIST8)
    for j in range(6):
        h = 1e-7 * max(1.0, abs(p[j]))
        dp = np.zeros(6)
        dp[j] = h
        fd = (_cost_and_grad(kp, p + dp, DIST8)[0] - _cost_and_grad(kp, p - dp, DIST8)[0]) / (2 * h)
        assert np.abs(fd - J[:, j]).max() <= 1e-5 * np.abs(J[:, j]).max()


@pytest.mark.parametrize("n_points", [4, 6, 9, 12, 16])
@pytest.mark.parametrize("dist", [None, np.zeros(0), DIST5[:4], DIST5, DIST8], ids=["none", "0", "4", "5", "8"])
def test_point_counts_and_distortion_models(n_points, dist):
    rng = np.random.default_rng(n_points)
    ids = np.sort(rng.choice(16, n_points, replace=False))
    while True:      # four points must not be collinear (a row / column / diagonal of the board)
        obj = pnp.object_points(ids, *BOARD)[:, :2]
        if np.linalg.matrix_rank(obj - obj.mean(0), tol=1e-6) == 2:
            break
        ids = np.sort(rng.choice(16, n_points, replace=False))
    kp, r, t = make_frame(rng, ids=ids, dist=DIST5 if dist is None else dist)
    if dist is None:      # None = no distortion: make the frame without it
        img = _project(ids, r, t, np.zeros(5))
        kp = np.c_[img.astype(np.float32).astype(np.float64), ids]
    ret, rvec, tvec = pnp.solve_pnp_host(kp, *BOARD, K, dist)
    assert ret
    assert np.linalg.norm(rvec.ravel() - r) <= 1e-3 * np.linalg.norm(r)
    assert np.linalg.norm(tvec.ravel() - t) <= 1e-3 * np.linalg.norm(t)


def test_duplicate_ids():
    rng = np.random.default_rng(7)
    ids = np.array([0, 3, 3, 5, 12, 15, 15])
    kp, r, t = make_frame(rng, ids=ids)
    ret, rvec, tvec = pnp.solve_pnp_host(kp, *BOARD, K, DIST5)
    assert ret and np.linalg.norm(rvec.ravel() - r) <= 1e-4 * np.linalg.norm(r)


def test_refused_arguments():
    kp, _, _ = make_frame(np.random.default_rng(3))
    with pytest.raises(ValueError):
        pnp.solve_pnp_host(kp, *BOARD, K, np.zeros(12))
    with pytest.raises(ValueError):
        pnp.solve_pnp_host(kp, *BOARD, K, np.zeros(14))
    skew = K.copy()
    skew[0, 1] = 1.0
    with pytest.raises(ValueError):
        pnp.solve_pnp_host(kp, *BOARD, skew, DIST5)
    bad = kp.copy()
    bad[0, 2] = 16
    with pytest.raises(IndexError):
        pnp.solve_pnp_host(bad, *BOARD, K, DIST5)


def test_too_few_and_degenerate():
    kp, _, _ = make_frame(np.random.default_rng(4))
    for n in (0, 1, 3):
        assert pnp.solve_pnp_host(kp[:n], *BOARD, K, DIST5) == (False, None, None)
    assert pnp.solve_pnp_host(np.array([]), *BOARD, K, DIST5) == (False, None, None)
    for ids in ([0, 1, 2, 3], [0, 5, 10, 15], [1, 5, 9, 13, 1]):      # a board row, the diagonal, a column
        kpc, _, _ = make_frame(np.random.default_rng(5), ids=ids)
        st, _ = pnp.solve_pnp_host_full(kpc, *BOARD, K, DIST5)
        assert st == pnp.PNP_DEGENERATE
        assert pnp.solve_pnp_host(kpc, *BOARD, K, DIST5)[0] is False


def test_integer_keypoints():
    """Without RefineNet the keypoints are int64 [x, y, id]; the image points are their float32 values."""
    kp, r, t = make_frame(np.random.default_rng(8))
    kpi = np.rint(kp).astype(np.int64)
    ret, rvec, _ = pnp.solve_pnp_host(kpi, *BOARD, K, DIST5)
    assert ret and np.linalg.norm(rvec.ravel() - r) <= 0.05 * np.linalg.norm(r)


def test_matches_cv2_where_available():
    """Where cv2 is absent, tests/test_pose_exact_host.py stands in: it holds the same solver to an exact restatement of the
    camera model cv2 documents."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(11)
    for sigma in (0.0, 0.3):
        for dist in (np.zeros(0), DIST5[:4], DIST5, DIST8):
            kp, _, _ = make_frame(rng, dist=dist if dist.size else np.zeros(5), sigma=sigma)
            obj, img = _pnp_points(kp, *BOARD)
            ok, rv, tv = cv2.solvePnP(obj, img, K, dist)
            ret, rvec, tvec = pnp.solve_pnp_host(kp, *BOARD, K, dist)
            assert ok and ret
            assert np.abs(rvec - rv).max() <= 1e-6 * max(1.0, np.abs(rv).max())
            assert np.abs(tvec - tv).max() <= 1e-6 * max(1.0, np.abs(tv).max())
