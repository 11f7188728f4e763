"""The exact statement of the rig pose cost for the rig pose tests: with the rig X held fixed, the residuals of one timestamp's
rows of every camera as tests/rig_exact.py (pinholes) or tests/fisheye_rig_exact.py (cameras with a model each) state them in long
double, a finite-difference Jacobian over the 6 parameters of the board pose alone, and stationarity.  Nothing here imports
deepcharuco_amd."""
import numpy as np

import camera_exact as cx
import fisheye_rig_exact as frx
import rig_exact as rx
from camera_exact import _w, f64


def _residuals(s):
    """The scene's own statement: fisheye_rig_exact's for a scene whose cameras are named there, else rig_exact's."""
    return frx.residuals if all(n in frx.CAMS for n in s.cams) else rx.residuals


def views_of(s, t, masks=None, keep=None):
    """``rig_exact.pool_views`` of timestamp t: (camera, obj, img) of every camera with rows, ascending; ``keep``: only these cameras."""
    v = rx.pool_views(s, [t], masks)[0]
    return v if keep is None else [x for x in v if x[0] in keep]


def residuals(views, s, X, p):
    """projected - observed of one timestamp's rows at the board pose p (6), cameras ascending -> (M, 2), working precision."""
    return _residuals(s)([views], s, np.asarray(X), np.asarray(p)[None])


def cost(views, s, X, p):
    r = residuals(views, s, X, p)
    return float((r * r).sum())


def jacobian_fd(views, s, X, p):
    """2M x 6 Jacobian of ``residuals`` with respect to p by central differences in the working precision -> float64; X is fixed.
    Steps as rig_exact.jacobian_fd: 1e-6 rad, 1e-6 |t|."""
    p = _w(p)
    cols = []
    for j in range(6):
        h = rx._step(p, j)
        d = _w(np.zeros(6))
        d[j] = h
        cols.append(f64(((residuals(views, s, X, p + d) - residuals(views, s, X, p - d)) / (2 * h)).ravel()))
    return np.stack(cols, 1)


def stationarity(views, s, X, p):
    """-> (cost, |J^T r| / (|J| |r|)) at the board pose p with X fixed."""
    r = f64(residuals(views, s, X, p)).ravel()
    J = jacobian_fd(views, s, X, p)
    nr = np.linalg.norm(r)
    return float(r @ r), (float(np.linalg.norm(J.T @ r) / (np.linalg.norm(J) * nr)) if nr > 0 else 0.0)


def rig_rt(X):
    """X [C - 1, 6] of (rvec, T) -> (R [C, 3, 3], T [C, 3]) with camera 0 the identity, float64: the (R, T) form of a rig."""
    X = np.asarray(X, np.float64)
    R = np.stack([np.eye(3)] + [f64(cx.rotation(x[:3])) for x in X])
    return R, np.r_[np.zeros((1, 3)), X[:, 3:]]


def pose_errors(rvec, tvec, P):
    """(max |R(rvec) - R(P)|, |tvec - t_P| / |t_P|) of one pose against the truth P (6)."""
    return (float(np.abs(f64(cx.rotation(rvec)) - f64(cx.rotation(P[:3]))).max()),
            float(np.linalg.norm(tvec - P[3:]) / np.linalg.norm(P[3:])))
