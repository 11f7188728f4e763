"""An exact restatement of the fisheye camera model, and the scenes the fisheye tests share.

Written from the documented model (OpenCV's ``cv2.fisheye`` documentation, skew 0), not from deepcharuco_amd/fisheye.py: nothing
of that module is imported, no threshold of it is restated and no analytic Jacobian exists here at all.

    R = exp([r]x);  (X, Y, Z) = R m + t;  a = X / Z, b = Y / Z;  r = sqrt(a^2 + b^2);  theta = atan r
    theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)
    x' = (theta_d / r) a, y' = (theta_d / r) b;  u = fx x' + cx, v = fy y' + cy

Arithmetic: numpy.longdouble (64-bit mantissa on x86) as tests/camera_exact.py, whose rotation this module uses.  theta_d / r is
the plain quotient for every r > 0 (no cancellation: atan r / r is accurate to the working precision down to the smallest r), and
r = 0 exactly takes the limit x' = y' = 0.  ``project_mp`` is a second statement in 40-digit mpmath with the rotation as a true
matrix exponential; tests/test_fisheye_host.py pins the array version to it on a handful of points, r = 0 and r = 1e-12 included.
"""
import numpy as np

import camera_exact as cx
from camera_exact import LD, f64

_w = cx._w

SIZE = (640, 480)
BOARD = (8, 5, 0.03)                       # 7 x 4 = 28 inner corners, not square
K_ZERO = np.zeros(4)
K_LENS = np.array([0.05, -0.01, 0.003, -0.0006])          # theta_d stays increasing up to pi / 2


def camera(fx, fy=None, size=SIZE, off=(0.0, 0.0)):
    """K with the principal point ``off`` px from the image centre."""
    w, h = size
    return np.array([[fx, 0.0, (w - 1) / 2 + off[0]], [0.0, fx if fy is None else fy, (h - 1) / 2 + off[1]], [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------------------------------------ the model

def distort(a, b, K, k):
    """Normalised (a, b) -> pixels (N, 2), working precision."""
    K, k = _w(K), _w(k)
    a, b = _w(a), _w(b)
    r = np.sqrt(a * a + b * b)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1 + k[0] * t2 + k[1] * t2 * t2 + k[2] * t2 * t2 * t2 + k[3] * t2 * t2 * t2 * t2)
    zero = r == 0
    s = thd / np.where(zero, _w(1.0), r)
    xd, yd = np.where(zero, 0 * a, s * a), np.where(zero, 0 * b, s * b)
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1)


def project(obj, p, K, k, X=None):
    """Board points (N, 3), pose p = (rvec, tvec) [and on through X, as camera_exact.camera_points] -> pixels (N, 2) in the
    working precision; every Z must be positive."""
    Q = cx.camera_points(obj, p, X)
    assert all(z > 0 for z in Q[2]), "a point is not in front of the camera"
    return distort(Q[0] / Q[2], Q[1] / Q[2], K, k)


def theta_max(obj, p, X=None):
    """The largest angle from the optical axis of any point, radians."""
    Q = cx.camera_points(obj, p, X)
    return float(np.max(np.arctan2(f64(np.sqrt(Q[0] * Q[0] + Q[1] * Q[1])), f64(Q[2]))))


def project_mp(obj, p, K, k, dps=40):
    """The same in ``dps``-digit mpmath, rotation by mpmath.expm -> list of (u, v) mpf pairs."""
    import mpmath
    with mpmath.workdps(dps):
        mp = mpmath.mpf
        r = [mp(float(v)) for v in p[:3]]
        R = mpmath.expm(mpmath.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]))
        out = []
        for m in np.asarray(obj, np.float64):
            X = [sum(R[i, j] * mp(float(m[j])) for j in range(3)) + mp(float(p[3 + i])) for i in range(3)]
            a, b = X[0] / X[2], X[1] / X[2]
            rr = mpmath.sqrt(a * a + b * b)
            th = mpmath.atan(rr)
            thd = th * (1 + sum(mp(float(k[j])) * th ** (2 * j + 2) for j in range(4)))
            xd, yd = (mp(0), mp(0)) if rr == 0 else (thd / rr * a, thd / rr * b)
            out.append((mp(float(K[0][0])) * xd + mp(float(K[0][2])), mp(float(K[1][1])) * yd + mp(float(K[1][2]))))
        return out


def jacobian_fd(obj, p, K, k):
    """2N x 14 Jacobian of the pixels with respect to (fx, fy, cx, cy, k1..k4, rvec, tvec) by central differences of ``project``
    in the working precision -> float64.  Steps 1e-6 of a parameter's scale: truncation ~1e-12 and rounding ~1e-13 of a column."""
    th = np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.asarray(k, np.float64), np.asarray(p, np.float64)]
    tn = float(np.linalg.norm(p[3:]))
    scale = [abs(th[0]), abs(th[1]), abs(th[0]), abs(th[1]), 1, 1, 1, 1, 1, 1, 1, tn, tn, tn]

    def f(t):
        Kt = np.array([[t[0], 0 * t[0], t[2]], [0 * t[0], t[1], t[3]], [0 * t[0], 0 * t[0], 1 + 0 * t[0]]], dtype=t.dtype)
        return project(obj, t[8:], Kt, t[4:8])

    J = np.empty((2 * len(obj), 14))
    for j in range(14):
        h = _w(1e-6) * _w(scale[j])
        d = _w(np.zeros(14))
        d[j] = h
        J[:, j] = f64(((f(_w(th) + d) - f(_w(th) - d)) / (2 * h)).ravel())
    return J


# ------------------------------------------------------------------------------------------------ scenes

def n_ids(board=BOARD):
    return (board[0] - 1) * (board[1] - 1)


def random_pose(rng, board, z_range, tilt_deg=40.0, lateral=0.35):
    """The board's centre ``lateral`` z off the axis at the most, at a depth in ``z_range``, tilted by up to ``tilt_deg``."""
    col, row, sq = board
    r = rng.normal(size=3)
    r *= np.deg2rad(rng.uniform(3, tilt_deg)) / np.linalg.norm(r)
    R = f64(cx.rotation(r))
    z = rng.uniform(*z_range)
    centre = np.array([row * sq / 2, col * sq / 2, 0.0])
    t = np.array([rng.uniform(-lateral, lateral) * z, rng.uniform(-lateral, lateral) * z, z]) - R @ centre
    return np.r_[r, t]


def make_views(seed, n_views, K, k, size=SIZE, board=BOARD, rows=None, sigma=0.0, z_range=None):
    """``n_views`` views of the board through the exact model, every corner inside the frame and spread over at least a fifth of
    its diagonal (poses are redrawn until they are; RuntimeError after 200 draws a view).  ``rows``: corners per view (a number or one per view; default all), ids in general position.  -> (board points
    float32, image points float32, ids, poses [n, 6]): what a corner pool holds."""
    rng = np.random.default_rng(seed)
    w, h = size
    N = n_ids(board)
    if z_range is None:                                  # the board (0.24 m wide) fills a fair part of the frame
        z_range = (0.20 * K[0, 0] / 400.0 + 0.03, 0.45 * K[0, 0] / 400.0 + 0.03)
    objs, imgs, ids_l, poses = [], [], [], []
    draws = 0
    while len(objs) < n_views:
        draws += 1
        if draws > 200 * n_views:
            raise RuntimeError("no pose keeps the board inside the frame")
        n = N if rows is None else int(rows if np.isscalar(rows) else rows[len(objs)])
        while True:
            ids = np.sort(rng.choice(N, n, replace=False))
            g = cx.grid_xy(ids, board[1]).astype(np.float64)
            if np.linalg.matrix_rank(g - g.mean(0)) == 2:
                break
        obj = cx.board_points(ids, *board)
        p = random_pose(rng, board, z_range)
        if not all(z > 0.02 for z in cx.camera_points(obj, p)[2]):
            continue
        img = f64(project(obj, p, K, k))
        inside = (img[:, 0] >= 0) & (img[:, 0] <= w - 1) & (img[:, 1] >= 0) & (img[:, 1] <= h - 1)
        if not inside.all() or np.linalg.norm(np.ptp(img, axis=0)) < np.hypot(w, h) / 5:
            continue
        if sigma:
            img = img + rng.normal(scale=sigma, size=img.shape)
        objs.append(obj)
        imgs.append(img.astype(np.float32))
        ids_l.append(ids)
        poses.append(p)
    return objs, imgs, ids_l, np.array(poses)


def keypoints(imgs, ids_l):
    """-> ``infer_image``-format [x, y, id] arrays."""
    return [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]
