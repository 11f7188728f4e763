"""The cameras of the multi-camera tests and the exact cost of their views, and the two-camera scenes of the stereo calibration
tests.  Nothing here imports deepcharuco_amd: the rig convention is cv2's, q_c = R_c q_0 + T_c.

This is the lowest module that sees both camera models (tests/camera_exact.py, tests/fisheye_exact.py), so the statements that
serve cameras of either live here, once: the table ``CAMS`` with its accessors (and which names state models), ``project_view``, and ``view_residuals`` /
``view_cost`` over ``rig_exact.pool_views``' layout (per timestamp a list of (camera, obj, img)).  The stereo cost below is that
statement at C = 2, rig_exact's is it as it stands, rigpose_exact's is it with X held fixed and one timestamp.  The
finite-difference routine and the stationarity measure of all of them are camera_exact's ``jacobian_of`` and ``stationarity_of``.

A stereo scene: a true rig X = (rvec, T), per timestamp a true board pose P_t in camera 0's frame, and per camera an id subset
drawn independently of the other camera's (or, with ``disjoint``, two subsets without a common id)."""
from collections import namedtuple

import numpy as np

import camera_exact as cx
import fisheye_exact as fx
from camera_exact import _w, f64

K_A = cx.K_EDGE                                                                    # fx / fy = 1.08
K_B = np.array([[352.0, 0, 203.1], [0, 371.0, 116.2], [0, 0, 1]])                 # fx != fy, another principal point
K_C = np.array([[298.0, 0, 161.0], [0, 325.0, 118.5], [0, 0, 1]])
# name -> (model, K, coefficients); read through cam_model / cam_K / cam_coeffs / cam, never by position
CAMS = {
    "A": ("pinhole", K_A, None), "B": ("pinhole", K_B, cx.CALIB_DIST), "C": ("pinhole", K_C, cx.DIST8), "A4": ("pinhole", K_A, cx.DIST8[:4]),
    # the cameras of the rigs with fisheye cameras in them: two wide lenses of a few pixels per degree, and B and A again
    "F": ("fisheye", fx.camera(230.0, off=(3.0, -2.0)), fx.K_LENS),
    "F0": ("fisheye", fx.camera(150.0, 163.0), None),                     # k = 0: the equidistant lens
    "P": ("pinhole", K_B, cx.CALIB_DIST),
    "P0": ("pinhole", K_A, None),
    # theta_d = theta - 0.2 theta^3 has its maximum, 0.8607, at theta = 1.291 (74 degrees): a pixel further than 0.8607 f from the
    # principal point is the image of no direction, so the model's inverse does not exist there
    "FN": ("fisheye", fx.camera(230.0), np.array([-0.2, 0.0, 0.0, 0.0])),
}
# a scene of these names states its cameras' models to the entry points (models=...), all-pinhole rigs of "P" / "P0" included;
# a scene of "A" / "B" / "C" / "A4" calls them without
STATES_MODELS = frozenset(("F", "F0", "P", "P0", "FN"))
BOARD_S, BOARD_L = cx.CALIB_BOARD, cx.BOARDS[3]                                    # 7x11 (60 ids) and 24x17 (368 ids)

# the gates of device against host in the stereo, rig and rig pose tests: poses within REL, or within FALLBACK with an equal cost
# where the last LM step is decided by rounding; the host definition at least MARGIN from every discrete decision
REL, FALLBACK, MARGIN = 1e-9, 1e-6, 1e-6

Scene = namedtuple("Scene", "kps0 kps1 X P board cam0 cam1 tag")


def cam_model(name):
    return CAMS[name][0]


def cam_K(name):
    return CAMS[name][1]


def cam_coeffs(name):
    return CAMS[name][2]


def cam(name):
    """(K, coefficients): the two camera arguments of a single-camera entry point."""
    return cam_K(name), cam_coeffs(name)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _tz(board, K):
    allp = cx.board_points(np.arange(cx.n_ids(board)), *board).astype(np.float64)
    return 0.5 * (K[0, 0] + K[1, 1]) * np.abs(allp - allp.mean(0)).max() / 100.0


def make_rig(kind, board, K0, K1):
    """The true rig (rvec, T) of a class: "small" (a 6 cm baseline at a 2 degree vergence, scaled to the board's distance),
    "toe90" (the cameras' axes meet at 90 degrees on the board) and "r170" (camera 1 looks back at camera 0 through the board:
    a relative rotation of 170 degrees, which a median of rotation vectors would wrap)."""
    d0, d1 = _tz(board, K0) * 1.05, _tz(board, K1) * 1.05
    if kind == "small":
        return np.r_[0.01, -0.035, 0.005, np.array([-0.3, 0.01, 0.015]) * d0]
    axis, deg = {"toe90": ((0.05, 1.0, 0.02), 90.0), "r170": ((0.03, 1.0, -0.02), 170.0)}[kind]
    r = _unit(axis) * np.deg2rad(deg)
    return np.r_[r, np.array([0, 0, d1]) - f64(cx.rotation(r)) @ np.array([0, 0, d0])]


def _base_tilt(X):
    """A board rotation in camera 0's frame that both cameras see at the same tilt: half the rig's rotation back (for a rig
    beyond 90 degrees: half of what it lacks to 180, camera 1 then sees the board's other face)."""
    th = np.linalg.norm(X[:3])
    if th < 1e-12:
        return np.zeros(3)
    a = X[:3] / th
    return -a * (th / 2 if th <= np.pi / 2 else (th - np.pi) / 2)


def _compose(ra, rb):
    """rvec of R(ra) R(rb), float64 (scene making only; any rotation vector of the product will do)."""
    R = f64(cx.rotation(ra)) @ f64(cx.rotation(rb))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(w) / 2, (np.trace(R) - 1) / 2
    return np.zeros(3) if s < 1e-12 else w / (2 * s) * np.arctan2(s, c)


def project_rig(obj, P, X, K, dist):
    """Board points through the board pose P (camera 0's frame) and, with X, on through the rig into camera 1 -> pixels (N, 2) in
    the working precision.  Every Z must be positive."""
    return cx.project(obj, P, K, dist, X)


def project_view(obj, P, X, name):
    """Pixels (N, 2) of camera ``name`` behind the rig transform X (None: the reference camera), by its own model."""
    K, k = cam(name)
    if cam_model(name) == "pinhole":
        return cx.project(obj, P, K, k, X)
    return fx.project(obj, P, K, fx.K_ZERO if k is None else k, X)


def scene(seed, n_pairs, rig="small", board=BOARD_S, cam0="A", cam1="B", sigma=0.0, rows=None, disjoint=False, tag=""):
    """-> Scene.  ``rows``: None (6 .. all ids, drawn per view), an int, or per timestamp a pair (n0, n1)."""
    rng = np.random.default_rng([9100, seed])
    (K0, d0), (K1, d1) = cam(cam0), cam(cam1)
    X = make_rig(rig, board, K0, K1)
    N = cx.n_ids(board)
    centre = cx.board_points(np.arange(N), *board).astype(np.float64).mean(0)
    tz = _tz(board, K0)
    kps0, kps1, poses = [], [], []
    for t in range(n_pairs):
        r = _compose(_base_tilt(X), _unit(rng.normal(size=3)) * np.deg2rad(rng.uniform(5, 25)))
        pos = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.95, 1.2)]) * tz
        P = np.r_[r, pos - f64(cx.rotation(r)) @ centre]
        want = rows[t] if isinstance(rows, (list, tuple)) else (rows, rows)
        n = [int(rng.integers(6, N + 1)) if w is None else min(int(w), N) for w in want]
        if disjoint:
            perm = rng.permutation(N)
            n = [min(n[0], N // 2), min(n[1], N // 2)]
            ids = [np.sort(perm[:n[0]]), np.sort(perm[N // 2:N // 2 + n[1]])]
        else:
            ids = [cx.draw_ids(rng, board, n[0]), cx.draw_ids(rng, board, n[1])]
        out = []
        for c, (K, d) in enumerate(((K0, d0), (K1, d1))):
            img = f64(project_rig(cx.board_points(ids[c], *board), P, X if c else None, K, d))
            if sigma:
                img = img + rng.normal(scale=sigma, size=img.shape)
            out.append(np.c_[img.astype(np.float32).astype(np.float64), ids[c]])
        kps0.append(out[0])
        kps1.append(out[1])
        poses.append(P)
    return Scene(kps0, kps1, X, np.array(poses), board, cam0, cam1, tag or f"{rig} {board[0]}x{board[1]} {cam0}/{cam1} sigma={sigma}")


def cam_args(s):
    """The four camera arguments of the stereo entry points, in order."""
    return (*cam(s.cam0), *cam(s.cam1))


# ------------------------------------------------------------------------------------------------ the exact cost

def pool_views(s, used=None, masks=None):
    """The rows as a corner pool holds them (id-sorted, stable) -> per used timestamp (obj0, img0, obj1, img1), float32 board
    points and float64 image points.  ``masks``: (masks0, masks1), bool per row in the scene's row order."""
    out = []
    for t in (range(len(s.kps0)) if used is None else used):
        v = []
        for c, kps in enumerate((s.kps0, s.kps1)):
            kp = kps[t]
            if masks is not None and masks[c] is not None and masks[c][t] is not None:
                kp = kp[np.asarray(masks[c][t]).astype(bool)]
            kp = kp[np.argsort(kp[:, 2], kind="stable")]
            v += [cx.board_points(kp[:, 2], *s.board), kp[:, :2]]
        out.append(tuple(v))
    return out


def view_residuals(views, cams, X, P):
    """projected - observed of every row, timestamp by timestamp, cameras ascending -> (M, 2), working precision.  ``views``: per
    timestamp a list of (camera, obj, img), ``cams`` the cameras' names, X [C - 1, 6] the rig, P [N, 6] the board poses."""
    return np.concatenate([project_view(o, p, X[c - 1] if c else None, cams[c]) - _w(i) for vs, p in zip(views, P) for c, o, i in vs])


def view_cost(views, cams, X, P):
    r = view_residuals(views, cams, X, P)
    return float((r * r).sum())


def _rig_form(views, s, X):
    """The stereo layout (obj0, img0, obj1, img1) and X (6) as ``view_residuals`` takes them."""
    return [[(0, o0, i0), (1, o1, i1)] for o0, i0, o1, i1 in views], (s.cam0, s.cam1), X[None]


def residuals(views, s, X, P):
    """projected - observed of every row, pair by pair, camera 0's rows first -> (M, 2), working precision."""
    return view_residuals(*_rig_form(views, s, np.asarray(X)), P)


def cost(views, s, X, P):
    return view_cost(*_rig_form(views, s, np.asarray(X)), P)


def jacobian_fd(views, s, X, P):
    """2M x (6 + 6N) Jacobian of ``residuals`` with respect to (X, P_0, ..., P_N-1) -> float64 (camera_exact.jacobian_of)."""
    return cx.jacobian_of(lambda x, p: residuals(views, s, x, p), X, P)


def stationarity(views, s, X, P):
    """-> (cost, |J^T r| / (|J| |r|)) at (X, P), from this module's residuals and finite differences."""
    return cx.stationarity_of(residuals(views, s, X, P), jacobian_fd(views, s, X, P))


def rig_error(r, s):
    """(max |R - R_true|, |T - T_true| / |T_true|) of a result against the scene's truth."""
    return (float(np.abs(r.R - f64(cx.rotation(s.X[:3]))).max()),
            float(np.linalg.norm(r.T - s.X[3:]) / np.linalg.norm(s.X[3:])))
