"""The host definition of the rig uncertainty (deepcharuco_amd/rig.py rig_uncertainty_host, stereo.py stereo_uncertainty_host,
_lm.schur_covariance with n = 6 (C - 1)): the Schur form against the inverse of the dense normal matrix and against a pseudo-inverse
of the exact model's finite-difference Jacobian, the two-camera wrapper, the growth along a chain, masks, unused timestamps,
statuses, and the baseline's standard deviation.  No GPU needed.

The gate of the first test is tests/test_calib_cov_host.py's: 1000 * cond(S) * 2^-52 relative to the largest entry compared, the
forward error of inverting a matrix of that condition in float64 with three decimal digits of room; the test computes cond(S)
itself.  The second test widens it by the error the finite differences bring: with e = |J_fd - J| / |J| (spectral norms, J the
analytic Jacobian) a pseudo-inverse moves by cond(J) e to first order and the diagonal of pinv pinv^T by twice that, so the gate is
1000 cond(S) 2^-52 + 2 cond(J) e, all three measured in the test."""
import math

import numpy as np
import pytest

import rig_exact as rx
from deepcharuco_amd import calib, pnp, rig, stereo
from test_calib_cov_host import _same_bits
from test_rig_host import CHAIN4, FAN3

SIGMA = 0.3

SCENES = {
    "fan3": lambda: rx.scene(20, 6, sigma=SIGMA, **FAN3),
    "chain4": lambda: rx.scene(20, 6, visible=rx.chain_visibility(4, 2), sigma=SIGMA, **CHAIN4),
    "two": lambda: rx.scene(20, 6, (0, 30), ("A", "B"), sigma=SIGMA),
}
_SOLVED = {}


def solved(name):
    """One scene and its host calibration per name, shared by the tests (test_gpu_rig_cov.py's too) and left unchanged."""
    if name not in _SOLVED:
        s = SCENES[name]()
        r = rig.rig_calibrate_host_full(s.kps, *s.board, *rx.cam_args(s))
        assert r.status == rig.RIG_OK
        _SOLVED[name] = (s, r)
    return _SOLVED[name]


def host(s, model, **kw):
    return rig.rig_uncertainty_host(s.kps, *s.board, *rx.cam_args(s), model, **kw)


def model_of(r, view_status=None):
    """A RigResult as the explicit tuple."""
    return r.rvec, r.T, r.rvecs, r.tvecs, r.view_status if view_status is None else np.asarray(view_status, np.int32)


def _blocks(s, r):
    """-> (used timestamps, X, P[used], the rows, the cameras of the steps) at the result r."""
    C = len(s.cams)
    usable = r.view_status == pnp.PNP_OK
    used = np.flatnonzero(usable.sum(1) >= 2)
    views = rx.pool_views(s, used)
    rows = stereo._rig_rows([[(c, o, m.astype(np.float32)) for c, o, m in v] for v in views], C)
    return used, np.c_[r.rvec, r.T][1:], np.c_[r.rvecs, r.tvecs][used], views, rows, rig._cameras(*rx.cam_args(s))[0]


@pytest.mark.parametrize("name", list(SCENES))
def test_schur_form_against_the_dense_inverse_and_the_finite_difference_pseudo_inverse(name):
    s, r = solved(name)
    u = host(s, r)
    C = len(s.cams)
    n = 6 * (C - 1)
    used, X, P, views, rows, cams = _blocks(s, r)
    N = used.size
    assert u.status == calib.COV_OK and u.stamps == N == r.stamps_used and u.points == r.points_used
    assert u.dof == 2 * u.points - n - 6 * N and u.cov_rig.shape == (n, n) and u.std_rig.shape == (C, 6)
    U, W, V, _, _, costs = stereo._normal_blocks(rows, cams, X, P, stereo._view_segments(rows))
    assert u.sigma2 == stereo._total(costs) / u.dof
    A = np.zeros((n + 6 * N, n + 6 * N))
    A[:n, :n] = V
    for i in range(N):
        k = slice(n + 6 * i, n + 6 * i + 6)
        A[:n, k], A[k, :n], A[k, k] = W[i], W[i].T, U[i]
    S = V - sum(W[i] @ np.linalg.solve(U[i], W[i].T) for i in range(N))
    cond = float(np.linalg.cond(S))
    gate = 1000.0 * cond * 2.0 ** -52
    dense = u.sigma2 * np.linalg.inv(A)
    blocks = np.array([dense[n + 6 * i:n + 6 * i + 6, n + 6 * i:n + 6 * i + 6] for i in range(N)])
    gaps = {"cov_rig": float(np.abs(dense[:n, :n] - u.cov_rig).max() / np.abs(dense[:n, :n]).max()),
            "cov_poses": float(np.abs(blocks - u.cov_poses[used]).max() / np.abs(blocks).max())}
    print(f"{name}: cond(S) {cond:.3g}, gate {gate:.3g}, against the dense inverse {gaps}")
    assert max(gaps.values()) <= gate, (gaps, gate)

    # the exact model's finite differences, independent of the analytic Jacobian
    J = rx.jacobian_fd(views, s, X, P)
    _, JX, JP = stereo._evaluate(rows, cams, X, P, True)
    Ja = np.zeros_like(J)
    for i in range(rows.obj.shape[0]):
        c, t = int(rows.cam[i]), int(rows.stamp[i])
        if c:
            Ja[2 * i:2 * i + 2, 6 * (c - 1):6 * c] = JX[i]
        Ja[2 * i:2 * i + 2, n + 6 * t:n + 6 * t + 6] = JP[i]
    e_fd = float(np.linalg.norm(J - Ja, 2) / np.linalg.norm(Ja, 2))
    cond_j = float(np.linalg.cond(Ja))
    gate_fd = gate + 2.0 * cond_j * e_fd
    Jp = np.linalg.pinv(J)
    d = u.sigma2 * np.einsum("ij,ij->i", Jp, Jp)                      # diag(pinv(J) pinv(J)^T): no normal equations formed
    mine = np.r_[np.diag(u.cov_rig), np.diagonal(u.cov_poses[used], axis1=1, axis2=2).ravel()]
    gaps = {"pinv diagonal, rig": float(np.abs(d[:n] - mine[:n]).max() / d[:n].max()),
            "pinv diagonal, poses": float(np.abs(d[n:] - mine[n:]).max() / d[n:].max())}
    print(f"{name}: finite-difference error {e_fd:.3g}, cond(J) {cond_j:.3g}, gate {gate_fd:.3g}, gaps {gaps}")
    assert max(gaps.values()) <= gate_fd, (gaps, gate_fd)

    assert np.array_equal(u.std_rig[1:].ravel(), np.sqrt(np.diag(u.cov_rig))) and not u.std_rig[0].any()
    assert np.array_equal(u.std_poses, np.sqrt(np.diagonal(u.cov_poses, axis1=1, axis2=2)))
    assert np.array_equal(u.cov_rig, u.cov_rig.T) and np.array_equal(u.cov_poses, u.cov_poses.transpose(0, 2, 1))
    _same_bits(u, host(s, model_of(r)))                               # the tuple form


def test_two_cameras_through_the_stereo_wrapper():
    s, _ = solved("two")
    (k0, k1), (d0, d1) = rx.cam_args(s)
    r = stereo.stereo_calibrate_host_full(s.kps[0], s.kps[1], *s.board, k0, d0, k1, d1)
    assert r.status == stereo.STEREO_OK
    u = stereo.stereo_uncertainty_host(s.kps[0], s.kps[1], *s.board, k0, d0, k1, d1, r)
    z = np.zeros((1, 3))
    by_rig = host(s, (np.r_[z, r.rvec[None]], np.r_[z, r.T[None]], r.rvecs, r.tvecs, r.view_status))
    assert u.status == calib.COV_OK and u.cov_rig.shape == (6, 6) and u.stamps == r.pairs_used and u.points == r.points_used
    print("stereo: std of X_1", u.std_rig[1].tolist(), "baseline", u.baseline_std[1])
    _same_bits(u, by_rig)
    _same_bits(u, stereo.stereo_uncertainty_host(s.kps[0], s.kps[1], *s.board, k0, d0, k1, d1,
                                                 (np.r_[z, r.rvec[None]], np.r_[z, r.T[None]], r.rvecs, r.tvecs, r.view_status)))
    R = np.stack([np.eye(3), r.R])                                    # rotation matrices in the tuple: through _rvec_of
    by_R = host(s, (R, np.r_[z, r.T[None]], r.rvecs, r.tvecs, r.view_status))
    assert by_R.status == calib.COV_OK and np.allclose(by_R.cov_rig, u.cov_rig, rtol=1e-6, atol=0)


@pytest.mark.parametrize("per_link", [2, 4])
def test_uncertainty_grows_along_a_chain(per_link):
    """Camera 3 of a chain reaches camera 0 through cameras 1 and 2 only.  One component of a vector's standard deviation depends
    on the axes it is written in, so "exceeds" is asserted on what does not: the root of the trace of the rotation block, the root
    of the trace of the translation block, and the baseline's standard deviation.  The component ratios are printed."""
    s = rx.scene(21, 3 * per_link, visible=rx.chain_visibility(4, per_link), sigma=SIGMA, **CHAIN4)
    r = rig.rig_calibrate_host_full(s.kps, *s.board, *rx.cam_args(s))
    assert r.status == rig.RIG_OK and r.parents.tolist() == [-1, 0, 1, 2]
    u = host(s, r)
    assert u.status == calib.COV_OK
    rot = np.sqrt((u.std_rig[:, :3] ** 2).sum(1))
    tra = np.sqrt((u.std_rig[:, 3:] ** 2).sum(1))
    print(f"chain of 4, {per_link} per link: std X_3 / std X_1 by component {(u.std_rig[3] / u.std_rig[1]).round(3).tolist()}, rotation "
          f"{rot[3] / rot[1]:.3f}, translation {tra[3] / tra[1]:.3f}, baseline {u.baseline_std[3] / u.baseline_std[1]:.3f}")
    assert rot[3] > rot[1] and tra[3] > tra[1] and u.baseline_std[3] > u.baseline_std[1]


def test_masks_are_rows_that_are_not_there():
    s, r = solved("fan3")
    rng = np.random.default_rng(5)
    masks = [[rng.random(len(k)) < 0.8 for k in cam] for cam in s.kps]
    masks[1][2][:] = True
    masks[2] = None
    assert all(m.sum() >= 4 for cam in masks[:2] for m in cam)
    cut = [[k[m] for k, m in zip(s.kps[c], masks[c])] if masks[c] is not None else s.kps[c] for c in range(3)]
    u = host(s, r, masks=masks)
    _same_bits(u, rig.rig_uncertainty_host(cut, *s.board, *rx.cam_args(s), r))
    assert u.status == calib.COV_OK and u.points == sum(len(k) for cam in cut for k in cam)
    full = host(s, r)
    assert u.points < full.points and not np.array_equal(u.cov_rig, full.cov_rig)
    _same_bits(full, host(s, r, masks=[None, [None] * 6, [np.ones(len(k), bool) for k in s.kps[2]]]))


def test_unused_timestamps_get_zeros():
    s, r = solved("fan3")
    st = r.view_status.copy()
    st[1, :] = pnp.PNP_DEGENERATE                                     # no usable view
    st[4, :2] = pnp.PNP_TOO_FEW                                       # one usable view: alone at its timestamp
    u = host(s, model_of(r, st))
    used = [0, 2, 3, 5]
    assert u.status == calib.COV_OK and u.stamps == 4
    assert u.points == sum(len(s.kps[c][t]) for t in used for c in range(3))
    assert not u.cov_poses[[1, 4]].any() and not u.std_poses[[1, 4]].any() and (u.std_poses[used] > 0).all()
    sub = s._replace(kps=[[k[t] for t in used] for k in s.kps])
    _same_bits(u._replace(cov_poses=u.cov_poses[used], std_poses=u.std_poses[used]),
               host(sub, (r.rvec, r.T, r.rvecs[used], r.tvecs[used], r.view_status[used])))


def _zero_but_counts(u):
    assert u.sigma2 == 0.0 and not u.cov_rig.any() and not u.std_rig.any() and not u.cov_poses.any() and not u.std_poses.any()
    assert not u.baseline_std.any()


def status_cases():
    """-> name -> (scene, model tuple, the expected (status, dof, points, stamps)); test_gpu_rig_cov.py runs the same cases."""
    out = {}
    s, r = solved("fan3")
    st = np.full_like(r.view_status, pnp.PNP_TOO_FEW)
    st[:, 0] = pnp.PNP_OK                                             # one usable view per timestamp
    out["no timestamp has two usable views"] = (s, model_of(r, st), (calib.COV_NO_VIEWS, -12, 0, 0))
    four = rx.scene(22, 1, rows=4, **FAN3)
    model = (np.r_[np.zeros((1, 3)), four.X[:, :3]], np.r_[np.zeros((1, 3)), four.X[:, 3:]], four.P[:, :3], four.P[:, 3:],
             [[pnp.PNP_OK, pnp.PNP_OK, pnp.PNP_DEGENERATE]])
    out["one timestamp, two views of 4 rows"] = (four, model, (calib.COV_NO_DOF, 16 - 12 - 6, 8, 1))
    st = r.view_status.copy()
    st[:, 2] = pnp.PNP_DEGENERATE                                     # camera 2 never usable: its V block is zero
    pts = sum(len(s.kps[c][t]) for t in range(6) for c in range(2))
    out["camera 2 never usable"] = (s, model_of(r, st), (calib.COV_SINGULAR, 2 * pts - 12 - 36, pts, 6))
    back = r.tvecs.copy()
    back[3, 2] = -back[3, 2]                                          # the board behind the cameras
    out["a board behind the cameras"] = (s, (r.rvec, r.T, r.rvecs, back, r.view_status),
                                         (calib.COV_SINGULAR, 2 * r.points_used - 12 - 36, r.points_used, 6))
    nan = r.T.copy()
    nan[1, 0] = np.nan
    out["a rig that is not finite"] = (s, (r.rvec, nan, r.rvecs, r.tvecs, r.view_status),
                                       (calib.COV_SINGULAR, 2 * r.points_used - 12 - 36, r.points_used, 6))
    return out


@pytest.mark.parametrize("name", ["no timestamp has two usable views", "one timestamp, two views of 4 rows", "camera 2 never usable",
                                  "a board behind the cameras", "a rig that is not finite"])
def test_statuses(name):
    s, model, expect = status_cases()[name]
    u = host(s, model)
    print(f"{name}: status {u.status}, dof {u.dof}, points {u.points}, stamps {u.stamps}")
    assert (u.status, u.dof, u.points, u.stamps) == expect
    _zero_but_counts(u)
    assert u.cov_rig.shape == (12, 12) and u.cov_poses.shape == (len(s.kps[0]), 6, 6)


def test_refusals():
    s, r = solved("fan3")
    with pytest.raises(ValueError, match="failed"):
        host(s, r._replace(status=rig.RIG_DISCONNECTED))
    with pytest.raises(ValueError, match="failed"):
        host(s, r._replace(status=rig.RIG_DEGENERATE))
    with pytest.raises(ValueError):
        host(s, (r.rvec, r.T, r.rvecs, r.tvecs))                      # not the tuple
    with pytest.raises(ValueError):
        host(s, (r.rvec[:2], r.T[:2], r.rvecs, r.tvecs, r.view_status))
    with pytest.raises(ValueError):
        host(s, (r.rvec, r.T, r.rvecs[:5], r.tvecs[:5], r.view_status[:5]))
    with pytest.raises(ValueError):
        rig.rig_uncertainty_host(s.kps[:2], *s.board, *rx.cam_args(s), r)
    two, _ = solved("two")
    (k0, k1), (d0, d1) = rx.cam_args(two)
    sr = stereo.stereo_calibrate_host_full(two.kps[0], two.kps[1], *two.board, k0, d0, k1, d1)
    with pytest.raises(ValueError, match="failed"):
        stereo.stereo_uncertainty_host(two.kps[0], two.kps[1], *two.board, k0, d0, k1, d1, sr._replace(status=stereo.STEREO_DEGENERATE))


@pytest.mark.parametrize("name", list(SCENES))
def test_baseline_std_against_a_central_difference(name):
    """|T_c| differentiated by central differences with steps of 1e-4 |T_c| (truncation 1e-8 of the gradient, rounding 1e-12) and
    propagated through cov_rig's translation block: 1e-7 relative."""
    s, r = solved(name)
    u = host(s, r)
    assert u.baseline_std[0] == 0.0
    for c in range(1, len(s.cams)):
        T = r.T[c]
        h = 1e-4 * np.linalg.norm(T)
        g = np.array([(np.linalg.norm(T + h * e) - np.linalg.norm(T - h * e)) / (2 * h) for e in np.eye(3)])
        k = slice(6 * (c - 1) + 3, 6 * c)
        want = math.sqrt(float(g @ u.cov_rig[k, k] @ g))
        gap = abs(u.baseline_std[c] - want) / want
        print(f"{name} camera {c}: |T| {np.linalg.norm(T):.6f} +- {u.baseline_std[c]:.3g}, gap to the central difference {gap:.3g}")
        assert gap <= 1e-7


def test_sigma2_recovers_the_noise():
    """The device test's scene at one draw: 24 timestamps of three cameras at 0.3 px, dof = 4,618: sigma^2 / 0.09 within
    1 +- 3 sqrt(2 / dof) = +-0.062, three standard deviations of a chi-square over its dof.  (The spread of 120 recalibrations takes
    the host two minutes and is left to tests/test_gpu_rig_cov.py.)"""
    kps, s = renoised(1)
    r = rig.rig_calibrate_host_full(kps[0], *s.board, *rx.cam_args(s))
    u = rig.rig_uncertainty_host(kps[0], *s.board, *rx.cam_args(s), r)
    half = 3.0 * math.sqrt(2.0 / 4618)
    print(f"sigma2 {u.sigma2:.6f}, ratio {u.sigma2 / SIGMA ** 2:.4f}, dof {u.dof}, allowed 1 +- {half:.4f}")
    assert u.status == calib.COV_OK and u.dof == 4618 and u.stamps == 24
    assert abs(u.sigma2 / SIGMA ** 2 - 1.0) <= half


def renoised(draws, angles=(0, 25, -25), cams=("A", "B", "C"), seed=11, sigma=SIGMA):
    """rig_exact.scene(2, 24, sigma=0.0, ...) -> (``draws`` sets of keypoint lists: the clean pixels plus noise of ``sigma`` px from
    default_rng(seed), drawn in order, each rounded to float32; the clean scene)."""
    s = rx.scene(2, 24, sigma=0.0, angles=angles, cams=cams)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(draws):
        out.append([[np.c_[(k[:, :2] + rng.normal(scale=sigma, size=(len(k), 2))).astype(np.float32).astype(np.float64), k[:, 2]]
                     for k in cam] for cam in s.kps])
    return out, s
