"""Rigs, camera pairs and scenes for the rectification tests, and an exact (long double) restatement of the two directions a
rectified camera is used in, made from the camera model of tests/camera_exact.py.  Nothing here imports deepcharuco_amd.

* the map direction: output pixel (u, v) of a rectified camera (R, P) -> x = (u - P02) / P00, y = (v - P12) / P11,
  q = R^T (x, y, 1) -> the source pixel ``cx.distort(q_x / q_z, q_y / q_z)``;
* the rectified projection: a point with normalised undistorted coordinates n in the source camera -> R (n, 1) -> P.

The rig convention is cv2's, q1 = R q0 + T."""
import functools

import numpy as np

import camera_exact as cx
import stereo_exact as sx
from camera_exact import _w, f64

SIZE = (320, 240)                                                    # (W, H) of every camera here
PAIRS = [("A", "B"), ("B", "C"), ("C", "A")]
RIGS = ("small", "toe90", "verge15", "vertical")
_FIXED = {"verge15": np.r_[0.02, np.deg2rad(15.0), -0.01, -0.06, 0.004, 0.008],
          "vertical": np.r_[np.deg2rad(-6.0), 0.01, 0.02, 0.003, 0.07, -0.004]}


def rig(kind, cam0, cam1):
    """The true rig X = (rvec, T): "small" and "toe90" are stereo_exact.make_rig's on the 7x11 board, "verge15" a 6 cm baseline
    at a 15 degree vergence, "vertical" camera 1 7 cm above camera 0."""
    if kind in _FIXED:
        return _FIXED[kind].copy()
    return sx.make_rig(kind, sx.BOARD_S, sx.cam_K(cam0), sx.cam_K(cam1))


def rig_RT(kind, cam0, cam1):
    X = rig(kind, cam0, cam1)
    return f64(cx.rotation(X[:3])), X[3:].copy()


def map_exact(K, dist, R, P, width, height):
    """The map direction for every pixel of a width x height output -> source pixels (height, width, 2), working precision; NaN
    where q_z <= 0.  R = None: identity; P = None: K."""
    K = np.asarray(K, np.float64)
    P = K if P is None else np.asarray(P, np.float64)
    Rw = _w(np.eye(3) if R is None else R)
    Pw = _w(P)
    u, v = np.meshgrid(_w(np.arange(width)), _w(np.arange(height)))
    x, y = ((u - Pw[0, 2]) / Pw[0, 0]).ravel(), ((v - Pw[1, 2]) / Pw[1, 1]).ravel()
    q = [Rw[0, i] * x + Rw[1, i] * y + Rw[2, i] for i in range(3)]
    front = np.array([bool(z > 0) for z in q[2]])
    one = _w(1.0)
    z = np.where(front, q[2], one)
    m = cx.distort(q[0] / z, q[1] / z, K, cx.dist8(dist))
    m[~front] = np.nan
    return m.reshape(height, width, 2)


def rectified_exact(n, R, P):
    """Normalised undistorted coordinates (N, 2) of the source camera -> rectified pixels (N, 2), working precision."""
    n, Rw, Pw = _w(n), _w(np.eye(3) if R is None else R), _w(P)
    q = [Rw[i, 0] * n[:, 0] + Rw[i, 1] * n[:, 1] + Rw[i, 2] for i in range(3)]
    return np.stack([Pw[0, 0] * q[0] / q[2] + Pw[0, 2], Pw[1, 1] * q[1] / q[2] + Pw[1, 2]], 1)


def pixel_grid(step=7, size=SIZE):
    """Pixel centres every ``step`` px over the frame, its last column and row included -> (N, 2) float64."""
    xs = np.unique(np.r_[np.arange(0, size[0], step), size[0] - 1]).astype(np.float64)
    ys = np.unique(np.r_[np.arange(0, size[1], step), size[1] - 1]).astype(np.float64)
    g = np.meshgrid(xs, ys)
    return np.stack([g[0].ravel(), g[1].ravel()], 1)


@functools.lru_cache(maxsize=None)
def scene(kind, cam0, cam1, seed=0, n_pairs=6):
    """A noise-free scene of ``n_pairs`` timestamps under rig ``kind`` -> stereo_exact.Scene.  "small" and "toe90" are
    stereo_exact.scene's own; for the two fixed rigs the same construction with the board's centre half way between the two
    optical axes at the working distance."""
    if kind not in _FIXED:
        return sx.scene(700 + seed, n_pairs, kind, sx.BOARD_S, cam0, cam1)
    rng = np.random.default_rng([9200, seed, RIGS.index(kind), PAIRS.index((cam0, cam1))])
    board = sx.BOARD_S
    (K0, d0), (K1, d1) = sx.cam(cam0), sx.cam(cam1)
    X = rig(kind, cam0, cam1)
    Rx = f64(cx.rotation(X[:3]))
    N = cx.n_ids(board)
    centre = cx.board_points(np.arange(N), *board).astype(np.float64).mean(0)
    tz = sx._tz(board, K0)
    c1, a1 = -Rx.T @ X[3:], Rx.T @ np.array([0.0, 0.0, 1.0])             # camera 1's centre and optical axis in camera 0's frame
    mid = 0.5 * (np.array([0.0, 0.0, tz]) + c1 + a1 * tz)
    kps0, kps1, poses = [], [], []
    for t in range(n_pairs):
        r = sx._compose(sx._base_tilt(X), sx._unit(rng.normal(size=3)) * np.deg2rad(rng.uniform(5, 25)))
        pos = mid + np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-0.05, 0.2)]) * tz
        P = np.r_[r, pos - f64(cx.rotation(r)) @ centre]
        ids = [cx.draw_ids(rng, board, int(rng.integers(20, N + 1))) for _ in range(2)]
        out = []
        for c, (K, d) in enumerate(((K0, d0), (K1, d1))):
            img = f64(sx.project_rig(cx.board_points(ids[c], *board), P, X if c else None, K, d))
            out.append(np.c_[img.astype(np.float32).astype(np.float64), ids[c]])
        kps0.append(out[0])
        kps1.append(out[1])
        poses.append(P)
    return sx.Scene(kps0, kps1, X, np.array(poses), board, cam0, cam1, f"{kind} {cam0}/{cam1}")


def common_rows(s, t):
    """The rows of timestamp t whose id both cameras saw -> (ids, pixels of camera 0 (n, 2), of camera 1 (n, 2))."""
    a, b = s.kps0[t], s.kps1[t]
    ids = np.intersect1d(a[:, 2], b[:, 2])
    ia = [int(np.flatnonzero(a[:, 2] == i)[0]) for i in ids]
    ib = [int(np.flatnonzero(b[:, 2] == i)[0]) for i in ids]
    return ids, a[ia, :2], b[ib, :2]


def board_in_camera0(s, t, ids):
    """The board points ``ids`` of timestamp t in camera 0's frame, from the scene's true pose -> (n, 3) float64."""
    obj = _w(cx.board_points(ids, *s.board))
    P = _w(s.P[t])
    R = cx.rotation(P[:3])
    return f64(np.stack([R[i, 0] * obj[:, 0] + R[i, 1] * obj[:, 1] + R[i, 2] * obj[:, 2] + P[3 + i] for i in range(3)], 1))


def epipolar_and_depth(s, r, reproject, pts0, pts1):
    """Worst gap between the two cameras' off-axis rectified coordinates (px) and worst relative distance of the reprojected 3-D
    point from the truth R1 (P_t o), over the ids both cameras saw at every timestamp.  ``r``: the rectification (R1, Q, axis);
    ``reproject(Q, xy0, xy1, axis)``; ``pts0(t, ids, pix)`` / ``pts1(t, ids, pix)`` give the rectified pixels of camera 0 / 1."""
    gap = err = 0.0
    seen = 0
    for t in range(len(s.kps0)):
        ids, p0, p1 = common_rows(s, t)
        seen += len(ids)
        if not len(ids):
            continue
        a, b = pts0(t, ids, p0), pts1(t, ids, p1)
        gap = max(gap, float(np.abs(a[:, 1 - r.axis] - b[:, 1 - r.axis]).max()))
        truth = board_in_camera0(s, t, ids) @ np.asarray(r.R1).T
        X = reproject(r.Q, a, b, r.axis)
        err = max(err, float((np.linalg.norm(X - truth, axis=1) / np.linalg.norm(truth, axis=1)).max()))
    assert seen >= 20, seen
    return gap, err
