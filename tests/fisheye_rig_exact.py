"""C-camera scenes whose cameras have a model each, pinhole or fisheye, for the tests of rigs with fisheye cameras in them: the
geometry of tests/rig_exact.py (``make_rig``: cameras on an arc around the board, each at the distance its focal length asks
for), pinhole views through tests/stereo_exact.py's ``project_rig`` and fisheye views through tests/fisheye_exact.py's ``distort``
at the composed pose X_c o P_t, all in long double; and that statement's own rig cost, finite-difference Jacobian and
stationarity, as rig_exact.py has them for pinholes.  Nothing here imports deepcharuco_amd.

A ``Scene`` has rig_exact.Scene's fields, so ``rig_exact.prefix``, ``pool_views``, ``rig_errors`` and ``chain_visibility`` serve
these scenes unchanged; ``cams`` holds names of ``CAMS`` below."""
import numpy as np

import camera_exact as cx
import fisheye_exact as fx
import rig_exact as rx
import stereo_exact as sx
from camera_exact import _w, f64

# name -> (model, K, coefficients): two wide lenses of a few pixels per degree and the two pinholes of the stereo tests
CAMS = {
    "F": ("fisheye", fx.camera(230.0, off=(3.0, -2.0)), fx.K_LENS),
    "F0": ("fisheye", fx.camera(150.0, 163.0), None),                     # k = 0: the equidistant lens
    "P": ("pinhole", sx.K_B, cx.CALIB_DIST),
    "P0": ("pinhole", sx.K_A, None),
    # theta_d = theta - 0.2 theta^3 has its maximum, 0.8607, at theta = 1.291 (74 degrees): a pixel further than 0.8607 f from the
    # principal point is the image of no direction, so the model's inverse does not exist there
    "FN": ("fisheye", fx.camera(230.0), np.array([-0.2, 0.0, 0.0, 0.0])),
}
THETA_D_MAX_FN = 0.8607

Scene = rx.Scene


def models(s):
    return [CAMS[n][0] for n in s.cams]


def cam_args(s):
    """(cameras, dists) of the rig entry points; ``models(s)`` goes with them."""
    return [CAMS[n][1] for n in s.cams], [CAMS[n][2] for n in s.cams]


def camera_points(obj, P, X):
    """Board points through the board pose P (camera 0's frame) and, with X, on through the rig -> [X, Y, Z], working precision."""
    obj, P = _w(obj), _w(P)
    R = cx.rotation(P[:3])
    Q = [R[i, 0] * obj[:, 0] + R[i, 1] * obj[:, 1] + R[i, 2] * obj[:, 2] + P[3 + i] for i in range(3)]
    if X is not None:
        X = _w(X)
        Rx = cx.rotation(X[:3])
        Q = [Rx[i, 0] * Q[0] + Rx[i, 1] * Q[1] + Rx[i, 2] * Q[2] + X[3 + i] for i in range(3)]
    return Q


def project_view(obj, P, X, name):
    """Pixels (N, 2) of camera ``name`` behind the rig transform X (None: the reference camera), working precision."""
    model, K, k = CAMS[name]
    if model == "pinhole":
        return sx.project_rig(obj, P, X, K, k)
    Q = camera_points(obj, P, X)
    assert all(z > 0 for z in Q[2]), "a point is not in front of the camera"
    return fx.distort(Q[0] / Q[2], Q[1] / Q[2], K, fx.K_ZERO if k is None else k)


def make_rig(angles, board, cams):
    """rig_exact.make_rig with these cameras' focal lengths."""
    d = [sx._tz(board, CAMS[n][1]) * 1.05 for n in cams]
    X = []
    for c in range(1, len(cams)):
        r = rx.AXIS * np.deg2rad(angles[c] - angles[0])
        X.append(np.r_[r, np.array([0, 0, d[c]]) - f64(cx.rotation(r)) @ np.array([0, 0, d[0]])])
    return np.array(X)


def scene(seed, n_stamps, angles, cams, board=sx.BOARD_S, visible=None, sigma=0.0, rows=None, tag="", rig=None):
    """rig_exact.scene, statement for statement, with ``project_view`` in place of the pinhole projection.  ``rig``: the true X
    [C - 1, 6] in place of ``make_rig``'s."""
    rng = np.random.default_rng([9300, seed])
    C = len(cams)
    X = make_rig(angles, board, cams) if rig is None else np.asarray(rig, np.float64)
    vis = np.ones((n_stamps, C), bool) if visible is None else np.asarray(visible, bool)
    N = cx.n_ids(board)
    centre = cx.board_points(np.arange(N), *board).astype(np.float64).mean(0)
    tz = sx._tz(board, CAMS[cams[0]][1])
    kps, poses = [[] for _ in range(C)], []
    for t in range(n_stamps):
        seen = [angles[c] for c in range(C) if vis[t, c]] or [angles[0]]
        base = -rx.AXIS * np.deg2rad((min(seen) + max(seen)) / 2 - angles[0])
        r = sx._compose(base, sx._unit(rng.normal(size=3)) * np.deg2rad(rng.uniform(5, 25)))
        pos = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.95, 1.2)]) * tz
        P = np.r_[r, pos - f64(cx.rotation(r)) @ centre]
        poses.append(P)
        for c in range(C):
            want = rows[t][c] if isinstance(rows, (list, tuple)) else rows
            n = int(rng.integers(6, N + 1)) if want is None else min(int(want), N)
            ids = cx.draw_ids(rng, board, n)
            noise = rng.normal(scale=sigma, size=(n, 2)) if sigma else 0.0     # (drawn for hidden views too: one stream per scene)
            if not vis[t, c]:
                kps[c].append(np.zeros((0, 3)))
                continue
            img = f64(project_view(cx.board_points(ids, *board), P, X[c - 1] if c else None, cams[c])) + noise
            kps[c].append(np.c_[img.astype(np.float32).astype(np.float64), ids])
    return Scene(kps, X, np.array(poses), board, tuple(cams), vis,
                 tag or f"{C} cameras {'/'.join(cams)} at {list(angles)} {board[0]}x{board[1]} sigma={sigma}")


def with_pose(s, t, P):
    """The noise-free scene with timestamp t's board pose replaced by P: its views are projected again, ids and order kept."""
    kps = [list(k) for k in s.kps]
    for c in range(len(s.cams)):
        ids = s.kps[c][t][:, 2]
        if len(ids):
            img = f64(project_view(cx.board_points(ids, *s.board), P, s.X[c - 1] if c else None, s.cams[c]))
            kps[c][t] = np.c_[img.astype(np.float32).astype(np.float64), ids]
    poses = s.P.copy()
    poses[t] = P
    return s._replace(kps=kps, P=poses)


def on_axis(s, t, c, row):
    """``with_pose`` with the board moved sideways until row ``row`` of view (c, t), c > 0, lies on camera c's optical axis: its
    pixel is then that camera's principal point (to float32 exactly, where the principal point is a float32)."""
    o = cx.board_points(s.kps[c][t][row:row + 1, 2], *s.board)
    q = np.array([float(v[0]) for v in camera_points(o, s.P[t], s.X[c - 1])])
    P = s.P[t].copy()
    P[3:] += f64(cx.rotation(s.X[c - 1, :3])).T @ np.array([-q[0], -q[1], 0.0])
    return with_pose(s, t, P)


def theta_max(s, t, c):
    """The largest angle from camera c's optical axis of a row of view (c, t), radians."""
    Q = camera_points(cx.board_points(s.kps[c][t][:, 2], *s.board), s.P[t], s.X[c - 1] if c else None)
    return float(np.max(np.arctan2(f64(np.sqrt(Q[0] * Q[0] + Q[1] * Q[1])), f64(Q[2]))))


# ------------------------------------------------------------------------------------------------ the exact cost

def residuals(views, s, X, P):
    """projected - observed of every row of ``rig_exact.pool_views``' views, timestamp by timestamp, cameras ascending -> (M, 2)."""
    parts = []
    for vs, p in zip(views, P):
        for c, o, i in vs:
            parts.append(project_view(o, p, X[c - 1] if c else None, s.cams[c]) - _w(i))
    return np.concatenate(parts)


def cost(views, s, X, P):
    r = residuals(views, s, X, P)
    return float((r * r).sum())


def jacobian_fd(views, s, X, P):
    """rig_exact.jacobian_fd over these residuals: 2M x (6 (C - 1) + 6 N), central differences in the working precision."""
    X, P = _w(X), _w(P)
    cols = []
    for block, other, first in ((X, P, True), (P, X, False)):
        for i in range(len(block)):
            for j in range(6):
                h = rx._step(block[i], j)
                d = _w(np.zeros(block.shape))
                d[i, j] = h
                hi = residuals(views, s, block + d, other) if first else residuals(views, s, other, block + d)
                lo = residuals(views, s, block - d, other) if first else residuals(views, s, other, block - d)
                cols.append(f64(((hi - lo) / (2 * h)).ravel()))
    return np.stack(cols, 1)


def stationarity(views, s, X, P):
    """-> (cost, |J^T r| / (|J| |r|)) at (X, P), from this module's residuals and finite differences."""
    r = f64(residuals(views, s, X, P)).ravel()
    J = jacobian_fd(views, s, X, P)
    nr = np.linalg.norm(r)
    return float(r @ r), (float(np.linalg.norm(J.T @ r) / (np.linalg.norm(J) * nr)) if nr > 0 else 0.0)
