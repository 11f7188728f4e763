"""The exact statement of the rig pose cost for the rig pose tests: tests/rig_exact.py's cost (cameras of either model) with the rig
X held fixed and a single timestamp, so a finite-difference Jacobian over the 6 parameters of the board pose alone, and
stationarity.  Nothing here imports deepcharuco_amd."""
import numpy as np

import camera_exact as cx
import rig_exact as rx
from camera_exact import f64


def views_of(s, t, masks=None, keep=None):
    """``rig_exact.pool_views`` of timestamp t: (camera, obj, img) of every camera with rows, ascending; ``keep``: only these cameras."""
    v = rx.pool_views(s, [t], masks)[0]
    return v if keep is None else [x for x in v if x[0] in keep]


def residuals(views, s, X, p):
    """projected - observed of one timestamp's rows at the board pose p (6), cameras ascending -> (M, 2), working precision."""
    return rx.residuals([views], s, np.asarray(X), np.asarray(p)[None])


def cost(views, s, X, p):
    r = residuals(views, s, X, p)
    return float((r * r).sum())


def jacobian_fd(views, s, X, p):
    """2M x 6 Jacobian of ``residuals`` with respect to p -> float64 (camera_exact.jacobian_of); X is fixed."""
    return cx.jacobian_of(lambda q: residuals(views, s, X, q), p)


def stationarity(views, s, X, p):
    """-> (cost, |J^T r| / (|J| |r|)) at the board pose p with X fixed."""
    return cx.stationarity_of(residuals(views, s, X, p), jacobian_fd(views, s, X, p))


def rig_rt(X):
    """X [C - 1, 6] of (rvec, T) -> (R [C, 3, 3], T [C, 3]) with camera 0 the identity, float64: the (R, T) form of a rig."""
    X = np.asarray(X, np.float64)
    R = np.stack([np.eye(3)] + [f64(cx.rotation(x[:3])) for x in X])
    return R, np.r_[np.zeros((1, 3)), X[:, 3:]]


def pose_errors(rvec, tvec, P):
    """(max |R(rvec) - R(P)|, |tvec - t_P| / |t_P|) of one pose against the truth P (6)."""
    return (float(np.abs(f64(cx.rotation(rvec)) - f64(cx.rotation(P[:3]))).max()),
            float(np.linalg.norm(tvec - P[3:]) / np.linalg.norm(P[3:])))
