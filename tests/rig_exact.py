"""C-camera scenes for the rig calibration tests, made by the exact camera model of tests/camera_exact.py (long double) through
tests/stereo_exact.py's ``project_rig`` and ``CAMS``, and that model's own statement of the rig cost: residuals of every camera, a
finite-difference Jacobian over all 6 (C - 1) + 6 N parameters, stationarity.  Nothing here imports deepcharuco_amd: the rig
convention is cv2's, q_c = R_c q_0 + T_c.

A scene: the cameras stand on an arc around the board and look at its centre (camera c at ``angles[c]`` degrees about a nearly
vertical axis, each at the distance its focal length asks for), a visibility table says which camera sees the board at which
timestamp, and every view draws its own id subset."""
from collections import namedtuple

import numpy as np

import camera_exact as cx
import stereo_exact as sx
from camera_exact import _w, f64

AXIS = sx._unit((0.05, 1.0, 0.02))

Scene = namedtuple("Scene", "kps X P board cams visible tag")


def make_rig(angles, board, cams):
    """The true X_c = (rvec, T), c = 1 .. C - 1 -> [C - 1, 6]: camera c's axis meets camera 0's on the board at angles[c] - angles[0]."""
    d = [sx._tz(board, sx.CAMS[n][0]) * 1.05 for n in cams]
    X = []
    for c in range(1, len(cams)):
        r = AXIS * np.deg2rad(angles[c] - angles[0])
        X.append(np.r_[r, np.array([0, 0, d[c]]) - f64(cx.rotation(r)) @ np.array([0, 0, d[0]])])
    return np.array(X)


def scene(seed, n_stamps, angles, cams, board=sx.BOARD_S, visible=None, sigma=0.0, rows=None, tag=""):
    """-> Scene.  ``visible``: None (every camera sees every timestamp) or a [T, C] bool table; ``rows``: None (6 .. all ids, drawn
    per view), an int, or a [T][C] table of ints.  The board is tilted towards the middle of the cameras that see it, then by a
    random 5 - 25 degrees."""
    rng = np.random.default_rng([9200, seed])
    C = len(cams)
    X = make_rig(angles, board, cams)
    vis = np.ones((n_stamps, C), bool) if visible is None else np.asarray(visible, bool)
    N = cx.n_ids(board)
    centre = cx.board_points(np.arange(N), *board).astype(np.float64).mean(0)
    tz = sx._tz(board, sx.CAMS[cams[0]][0])
    kps, poses = [[] for _ in range(C)], []
    for t in range(n_stamps):
        seen = [angles[c] for c in range(C) if vis[t, c]] or [angles[0]]
        base = -AXIS * np.deg2rad((min(seen) + max(seen)) / 2 - angles[0])
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
            K, d = sx.CAMS[cams[c]]
            img = f64(sx.project_rig(cx.board_points(ids, *board), P, X[c - 1] if c else None, K, d)) + noise
            kps[c].append(np.c_[img.astype(np.float32).astype(np.float64), ids])
    return Scene(kps, X, np.array(poses), board, tuple(cams), vis,
                 tag or f"{C} cameras {'/'.join(cams)} at {list(angles)} {board[0]}x{board[1]} sigma={sigma}")


def cam_args(s):
    """(cameras, dists) of the rig entry points."""
    return [sx.CAMS[n][0] for n in s.cams], [sx.CAMS[n][1] for n in s.cams]


def prefix(s, n):
    """The scene's first n timestamps."""
    return s._replace(kps=[k[:n] for k in s.kps], P=s.P[:n], visible=s.visible[:n])


# ------------------------------------------------------------------------------------------------ the exact cost

def pool_views(s, used, masks=None):
    """The rows as a corner pool holds them (id-sorted, stable) -> per used timestamp a list of (camera, obj float32, img float64) of
    the cameras that see it, ascending.  ``masks``: per camera None or per timestamp bool per row in the scene's row order."""
    out = []
    for t in used:
        views = []
        for c in range(len(s.cams)):
            kp = s.kps[c][t]
            if not len(kp):
                continue
            if masks is not None and masks[c] is not None and masks[c][t] is not None:
                kp = kp[np.asarray(masks[c][t]).astype(bool)]
            kp = kp[np.argsort(kp[:, 2], kind="stable")]
            views.append((c, cx.board_points(kp[:, 2], *s.board), kp[:, :2]))
        out.append(views)
    return out


def residuals(views, s, X, P):
    """projected - observed of every row, timestamp by timestamp, cameras ascending -> (M, 2), working precision."""
    parts = []
    for vs, p in zip(views, P):
        for c, o, i in vs:
            K, d = sx.CAMS[s.cams[c]]
            parts.append(sx.project_rig(o, p, X[c - 1] if c else None, K, d) - _w(i))
    return np.concatenate(parts)


def cost(views, s, X, P):
    r = residuals(views, s, X, P)
    return float((r * r).sum())


def _step(v, j):
    return _w(1e-6) * (1 if j < 3 else cx._sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5]))


def jacobian_fd(views, s, X, P):
    """2M x (6 (C - 1) + 6 N) Jacobian of ``residuals`` with respect to (X_1, ..., X_{C-1}, P_0, ..., P_{N-1}) by central
    differences in the working precision -> float64.  Steps as camera_exact.jacobian_fd: 1e-6 rad, 1e-6 |t|."""
    X, P = _w(X), _w(P)
    cols = []
    for i in range(len(X)):
        for j in range(6):
            h = _step(X[i], j)
            d = _w(np.zeros(X.shape))
            d[i, j] = h
            cols.append(f64(((residuals(views, s, X + d, P) - residuals(views, s, X - d, P)) / (2 * h)).ravel()))
    for i in range(len(P)):
        for j in range(6):
            h = _step(P[i], j)
            d = _w(np.zeros(P.shape))
            d[i, j] = h
            cols.append(f64(((residuals(views, s, X, P + d) - residuals(views, s, X, P - d)) / (2 * h)).ravel()))
    return np.stack(cols, 1)


def stationarity(views, s, X, P):
    """-> (cost, |J^T r| / (|J| |r|)) at (X, P), from this module's residuals and finite differences."""
    r = f64(residuals(views, s, X, P)).ravel()
    J = jacobian_fd(views, s, X, P)
    nr = np.linalg.norm(r)
    return float(r @ r), (float(np.linalg.norm(J.T @ r) / (np.linalg.norm(J) * nr)) if nr > 0 else 0.0)


def rig_errors(r, s):
    """Per camera 1 .. C - 1 (max |R - R_true|, |T - T_true| / |T_true|) -> the worst of each."""
    eR = max(float(np.abs(r.R[c] - f64(cx.rotation(s.X[c - 1, :3]))).max()) for c in range(1, len(s.cams)))
    eT = max(float(np.linalg.norm(r.T[c] - s.X[c - 1, 3:]) / np.linalg.norm(s.X[c - 1, 3:])) for c in range(1, len(s.cams)))
    return eR, eT


def chain_visibility(n_cams, per_link):
    """Timestamps seen by cameras (0, 1) only, then (1, 2) only, ...: ``per_link`` each."""
    vis = np.zeros(((n_cams - 1) * per_link, n_cams), bool)
    for k in range(n_cams - 1):
        vis[k * per_link:(k + 1) * per_link, [k, k + 1]] = True
    return vis
