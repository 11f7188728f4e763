"""C-camera scenes for the rig calibration tests, of cameras of either model, made by tests/stereo_exact.py's ``project_view``
(long double), and the rig cost over them: stereo_exact.view_residuals with a finite-difference Jacobian over all
6 (C - 1) + 6 N parameters and stationarity.  Nothing here imports deepcharuco_amd: the rig convention is cv2's,
q_c = R_c q_0 + T_c.

A scene: the cameras (names of stereo_exact.CAMS) stand on an arc around the board and look at its centre (camera c at
``angles[c]`` degrees about a nearly vertical axis, each at the distance its focal length asks for), a visibility table says which
camera sees the board at which timestamp, and every view draws its own id subset."""
from collections import namedtuple

import numpy as np

import camera_exact as cx
import fisheye_exact as fx
import stereo_exact as sx
from camera_exact import f64

AXIS = sx._unit((0.05, 1.0, 0.02))
STREAM = 9200                             # the random stream of ``scene``; fisheye_rig_exact.scene draws from another

Scene = namedtuple("Scene", "kps X P board cams visible tag")


def make_rig(angles, board, cams):
    """The true X_c = (rvec, T), c = 1 .. C - 1 -> [C - 1, 6]: camera c's axis meets camera 0's on the board at angles[c] - angles[0]."""
    d = [sx._tz(board, sx.cam_K(n)) * 1.05 for n in cams]
    X = []
    for c in range(1, len(cams)):
        r = AXIS * np.deg2rad(angles[c] - angles[0])
        X.append(np.r_[r, np.array([0, 0, d[c]]) - f64(cx.rotation(r)) @ np.array([0, 0, d[0]])])
    return np.array(X)


def scene(seed, n_stamps, angles, cams, board=sx.BOARD_S, visible=None, sigma=0.0, rows=None, tag="", rig=None, stream=STREAM):
    """-> Scene.  ``visible``: None (every camera sees every timestamp) or a [T, C] bool table; ``rows``: None (6 .. all ids, drawn
    per view), an int, or a [T][C] table of ints; ``rig``: the true X [C - 1, 6] in place of ``make_rig``'s.  The board is tilted
    towards the middle of the cameras that see it, then by a random 5 - 25 degrees."""
    rng = np.random.default_rng([stream, seed])
    C = len(cams)
    X = make_rig(angles, board, cams) if rig is None else np.asarray(rig, np.float64)
    vis = np.ones((n_stamps, C), bool) if visible is None else np.asarray(visible, bool)
    N = cx.n_ids(board)
    centre = cx.board_points(np.arange(N), *board).astype(np.float64).mean(0)
    tz = sx._tz(board, sx.cam_K(cams[0]))
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
            img = f64(sx.project_view(cx.board_points(ids, *board), P, X[c - 1] if c else None, cams[c])) + noise
            kps[c].append(np.c_[img.astype(np.float32).astype(np.float64), ids])
    return Scene(kps, X, np.array(poses), board, tuple(cams), vis,
                 tag or f"{C} cameras {'/'.join(cams)} at {list(angles)} {board[0]}x{board[1]} sigma={sigma}")


def with_pose(s, t, P):
    """The noise-free scene with timestamp t's board pose replaced by P: its views are projected again, ids and order kept."""
    kps = [list(k) for k in s.kps]
    for c in range(len(s.cams)):
        ids = s.kps[c][t][:, 2]
        if len(ids):
            img = f64(sx.project_view(cx.board_points(ids, *s.board), P, s.X[c - 1] if c else None, s.cams[c]))
            kps[c][t] = np.c_[img.astype(np.float32).astype(np.float64), ids]
    poses = s.P.copy()
    poses[t] = P
    return s._replace(kps=kps, P=poses)


def on_axis(s, t, c, row):
    """``with_pose`` with the board moved sideways until row ``row`` of view (c, t), c > 0, lies on camera c's optical axis: its
    pixel is then that camera's principal point (to float32 exactly, where the principal point is a float32)."""
    o = cx.board_points(s.kps[c][t][row:row + 1, 2], *s.board)
    q = np.array([float(v[0]) for v in cx.camera_points(o, s.P[t], s.X[c - 1])])
    P = s.P[t].copy()
    P[3:] += f64(cx.rotation(s.X[c - 1, :3])).T @ np.array([-q[0], -q[1], 0.0])
    return with_pose(s, t, P)


def theta_max(s, t, c):
    """The largest angle from camera c's optical axis of a row of view (c, t), radians."""
    return fx.theta_max(cx.board_points(s.kps[c][t][:, 2], *s.board), s.P[t], s.X[c - 1] if c else None)


def cam_args(s):
    """(cameras, dists) of the rig entry points."""
    return [sx.cam_K(n) for n in s.cams], [sx.cam_coeffs(n) for n in s.cams]


def models(s):
    return [sx.cam_model(n) for n in s.cams]


def entry_args(s):
    """What the scene passes an entry point for its cameras -> ((cameras, dists), keywords): ``models=`` is among the keywords if
    and only if the scene states models (every name in stereo_exact.STATES_MODELS), else there are none."""
    return cam_args(s), (dict(models=models(s)) if all(n in sx.STATES_MODELS for n in s.cams) else {})


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
    return sx.view_residuals(views, s.cams, X, P)


def cost(views, s, X, P):
    return sx.view_cost(views, s.cams, X, P)


def jacobian_fd(views, s, X, P):
    """2M x (6 (C - 1) + 6 N) Jacobian of ``residuals`` with respect to (X_1, ..., X_{C-1}, P_0, ..., P_{N-1}) -> float64
    (camera_exact.jacobian_of)."""
    return cx.jacobian_of(lambda x, p: residuals(views, s, x, p), X, P)


def stationarity(views, s, X, P):
    """-> (cost, |J^T r| / (|J| |r|)) at (X, P), from this module's residuals and finite differences."""
    return cx.stationarity_of(residuals(views, s, X, P), jacobian_fd(views, s, X, P))


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
