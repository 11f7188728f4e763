"""The host definition of the rig calibration with fisheye cameras in the rig (deepcharuco_amd/rig.py, rig_calibrate_host_full with
``models``) against the exact statement of tests/fisheye_rig_exact.py: the defaults unchanged, the Jacobian of
fisheye._project_q and of a mixed rig's rows, truth recovery on five classes of rigs, the stationary point on noisy scenes, and
the bookkeeping of a fisheye view with a pixel outside its model.  No GPU.  Every test prints what it measured.

The truth gates are measured, not imported: a 150 to 230 px lens has fewer pixels per radian than test_stereo_host's cameras, so
float32 pixels leave more of an angle open.  Each is 4 x the largest value the host definition reaches over the five noise-free
scenes of ``CLASSES`` at seed 1 (4 x is test_stereo_host's margin for the float32 rounding of another draw), measured beside it."""
import math

import numpy as np
import pytest

import camera_exact as cx
import fisheye_exact as fx
import fisheye_rig_exact as frx
import rig_exact as rx
import stereo_exact as sx
from deepcharuco_amd import fisheye, pnp, rig, stereo
from test_rig_host import FAN3 as PINHOLE_FAN3

TRUTH_R = 3.8e-7            # 4 x 9.51e-8: max |R_c - R_true| (the eight-camera rig, 8 rows per view)
TRUTH_T = 6.3e-7            # 4 x 1.57e-7: |T_c - T_true| / |T_true| (the same rig)
TRUTH_RMS = 4.1e-5          # 4 x 1.013e-5 px (four fisheye cameras)
TRUTH_POSE_R = 1.12e-6      # 4 x 2.79e-7: max |R(P_t) - R_true| (the pair: a P_t rests on its own timestamp's two views alone)
TRUTH_POSE_T = 4.8e-7       # 4 x 1.18e-7 (the chain)
MARGIN = 1e-6               # test_gpu_stereo's: the host definition's distance from every discrete decision

# five classes of rigs: (angles, cameras of stereo_exact.CAMS, and what else the scene takes)
CLASSES = {
    "fan3 F/P/F": dict(angles=(0, 25, -25), cams=("F", "P", "F0")),                       # a fisheye reference camera
    "pair P/F": dict(angles=(0, 30), cams=("P", "F")),
    "four F": dict(angles=(-30, -10, 10, 30), cams=("F", "F0", "F", "F0")),
    "chain4 P/F/F/P": dict(angles=(0, 20, 40, 60), cams=("P", "F", "F0", "P0"), visible=rx.chain_visibility(4, 2)),
    "eight": dict(angles=tuple(np.linspace(-35, 35, 8).tolist()), cams=("F", "P", "F0", "P0") * 2, rows=8),
}
FAN3 = CLASSES["fan3 F/P/F"]


def class_scene(name, seed, sigma=0.0, n_stamps=6, **kw):
    return frx.scene(seed, n_stamps, sigma=sigma, **{**CLASSES[name], **kw})


def solve(s, **kw):
    return rig.rig_calibrate_host_full(s.kps, *s.board, *frx.cam_args(s), models=frx.models(s), **kw)


def pose_errors(r, s, used):
    eR = max(float(np.abs(pnp._rodrigues(r.rvecs[t]) - cx.f64(cx.rotation(s.P[t, :3]))).max()) for t in used)
    eT = max(float(np.linalg.norm(r.tvecs[t] - s.P[t, 3:]) / np.linalg.norm(s.P[t, 3:])) for t in used)
    return eR, eT


# ------------------------------------------------------------------------------------------------ defaults

def test_no_models_and_all_pinhole_are_the_definition_as_it_was():
    """test_rig_host's fan of three pinholes: ``models=None`` and three times "pinhole" run the same functions on the same values
    (``pnp._solve`` and ``stereo._project_q``, by identity), so the results are equal bit for bit."""
    s = rx.scene(1, 8, **PINHOLE_FAN3)
    cameras, dists = rx.cam_args(s)
    a = rig.rig_calibrate_host_full(s.kps, *s.board, cameras, dists)
    b = rig.rig_calibrate_host_full(s.kps, *s.board, cameras, dists, models=["pinhole"] * 3)
    assert a.status == rig.RIG_OK
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for cams in (rig._cameras(cameras, dists)[0], rig._cameras(cameras, dists, ["pinhole"] * 3)[0]):
        assert all(stereo._model_of(c) == (pnp._solve, stereo._project_q) for c in cams)
    mixed = rig._cameras(cameras, [None, dists[1], np.zeros(4)], ["fisheye", "pinhole", "fisheye"])[0]
    assert [stereo._model_of(c) for c in mixed] == [(fisheye._solve, fisheye._project_q), (pnp._solve, stereo._project_q),
                                                 (fisheye._solve, fisheye._project_q)]
    for bad in (["pinhole"] * 2, ["pinhole", "fisheye", "equidistant"]):
        with pytest.raises(ValueError):
            rig.rig_calibrate_host_full(s.kps, *s.board, cameras, dists, models=bad)
    with pytest.raises(ValueError):                                       # a fisheye camera has four coefficients
        rig.rig_calibrate_host_full(s.kps, *s.board, cameras, dists, models=["pinhole", "fisheye", "pinhole"])


# ------------------------------------------------------------------------------------------------ the Jacobian

def test_project_q_jacobian_matches_exact_finite_differences():
    """d(u, v)/dQ of fisheye._project_q against central differences of the exact model, a point on the optical axis (r = 0) and
    one at r = 1e-12 among them, where the model's series takes over.  Gate: 1e-10 of a column's largest entry, test_rig_host's."""
    rng = np.random.default_rng(8)
    Q = np.c_[rng.uniform(-0.4, 0.4, (12, 2)), rng.uniform(0.2, 0.5, 12)]
    Q[3] *= [2.5, 2.5, 0.3]                                               # a point far off the axis
    Q[0, :2] = 0.0
    Q[1, :2] = [1e-12 * Q[1, 2], 0.0]
    for name in ("F", "F0"):
        K, k = sx.cam(name)
        k = fx.K_ZERO if k is None else k
        res, D = fisheye._project_q(Q, np.zeros((12, 2)), K, k, True)
        exact = lambda q: fx.distort(q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], K, k)
        gap_r = float(np.abs(res - cx.f64(exact(cx._w(Q)))).max())
        J, Jfd = np.empty((24, 3)), np.empty((24, 3))
        for j in range(3):
            h = cx._w(1e-6) * cx._w(np.linalg.norm(Q, axis=1))
            d = cx._w(np.zeros(Q.shape))
            d[:, j] = h
            Jfd[:, j] = cx.f64((exact(cx._w(Q) + d) - exact(cx._w(Q) - d)) / (2 * h)[:, None]).ravel()
            J[:, j] = D[:, :, j].ravel()
        gap = float((np.abs(J - Jfd).max(0) / np.abs(Jfd).max(0)).max())
        axis = float(np.abs(J[:4] - Jfd[:4]).max() / np.abs(Jfd[:4]).max())
        print(f"{name}: pixels within {gap_r:.2e} px, Jacobian columns within {gap:.2e} of their largest entry (the rows at r = 0 "
              f"and 1e-12: {axis:.2e})")
        assert gap_r <= 1e-10 and gap <= 1e-10 and axis <= 1e-10


def test_mixed_rig_jacobian_matches_exact_finite_differences():
    """J_X and J_P of a fisheye, a pinhole and a fisheye camera's rows, away from the solution: test_rig_host's test on a mixed rig."""
    s = class_scene("fan3 F/P/F", 11, n_stamps=3, rows=9)
    rng = np.random.default_rng(5)
    X = s.X + rng.normal(scale=1e-2, size=s.X.shape) * np.r_[1, 1, 1, [np.linalg.norm(s.X[0, 3:])] * 3]
    P = s.P + rng.normal(scale=1e-2, size=s.P.shape) * np.r_[1, 1, 1, [np.linalg.norm(s.P[0, 3:])] * 3]
    views = rx.pool_views(s, range(3))
    rows = rig._rows_of(views, 3)
    cams = rig._cameras(*frx.cam_args(s), frx.models(s))[0]
    res, JX, JP = stereo._evaluate(rows, cams, X, P, True)
    M, N = rows.obj.shape[0], len(views)
    J = np.zeros((2 * M, 12 + 6 * N))
    for c in (1, 2):
        sel = np.repeat(rows.cam == c, 2)
        J[sel, 6 * (c - 1):6 * c] = JX.reshape(2 * M, 6)[sel]
    for i in range(N):
        sel = np.repeat(rows.stamp == i, 2)
        J[sel, 12 + 6 * i:18 + 6 * i] = JP.reshape(2 * M, 6)[sel]
    assert not JX[rows.cam == 0].any() and JX[rows.cam == 2].any()
    Jfd = frx.jacobian_fd(views, s, X, P)
    gap_r = float(np.abs(res - cx.f64(frx.residuals(views, s, X, P))).max())
    gap = float((np.abs(J - Jfd).max(0) / np.abs(Jfd).max(0)).max())
    print(f"{s.tag}: residuals within {gap_r:.2e} px, Jacobian columns within {gap:.2e} of their largest entry")
    assert gap_r <= 1e-10 and gap <= 1e-10


# ------------------------------------------------------------------------------------------------ truth

@pytest.mark.parametrize("name", list(CLASSES))
def test_truth_recovery_noise_free_float32(name):
    """Every X_c and every P_t inside this file's measured gates; the chain's tree is 0 - 1 - 2 - 3, so a fisheye camera is placed
    through a fisheye camera."""
    s = class_scene(name, 1)
    r, margin = solve(s, with_margin=True)
    T = len(s.P)
    eR, eT = rx.rig_errors(r, s)
    pR, pT = pose_errors(r, s, range(T))
    print(f"{s.tag}: |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, board poses {pR:.2e} / {pT:.2e}, rms {r.rms:.2e} px, "
          f"steps {r.iterations} / {r.attempts}, parents {r.parents.tolist()}, margin {margin:.3g}")
    assert r.status == rig.RIG_OK and r.stamps_used == T and margin >= MARGIN
    assert (r.view_status == pnp.PNP_OK).tolist() == s.visible.tolist()
    assert r.points_used == sum(len(k) for kl in s.kps for k in kl) == int(r.view_points.sum()) == int(r.stamp_points.sum())
    assert r.parents.tolist() == ([-1, 0, 1, 2] if name.startswith("chain4") else [-1] + [0] * (len(s.cams) - 1))
    assert np.array_equal(r.R[0], np.eye(3)) and not r.T[0].any() and not r.rvec[0].any()
    assert eR <= TRUTH_R and eT <= TRUTH_T and r.rms <= TRUTH_RMS
    assert pR <= TRUTH_POSE_R and pT <= TRUTH_POSE_T


@pytest.mark.parametrize("name", list(CLASSES))
def test_noisy_scene_ends_at_a_stationary_point_no_higher_than_the_truth(name):
    """sigma = 0.3 px: the cost at the result is no higher than at the truth, |J^T r| <= 1e-6 |J| |r| with the exact model's
    finite-difference Jacobian, and the rms is that cost's."""
    s = class_scene(name, 2, sigma=0.3, n_stamps=6 if name.startswith("chain4") else 4, rows=8 if name == "eight" else 12)
    r, margin = solve(s, with_margin=True)
    assert r.status == rig.RIG_OK and r.stamps_used == len(s.P) and margin >= MARGIN
    used = np.flatnonzero((r.view_status == pnp.PNP_OK).sum(1) >= 2)
    X, P = np.c_[r.rvec, r.T][1:], np.c_[r.rvecs, r.tvecs][used]
    views = rx.pool_views(s, used)
    c_res, grad = frx.stationarity(views, s, X, P)
    c_true = frx.cost(views, s, s.X, s.P)
    print(f"{s.tag}: cost {c_res:.6f} (truth {c_true:.6f}), |Jtr| / (|J||r|) {grad:.2e}, rms {r.rms:.4f} px, rig error "
          f"{rx.rig_errors(r, s)}, steps {r.iterations} / {r.attempts}")
    assert c_res <= c_true and grad <= 1e-6
    assert abs(r.rms - math.sqrt(c_res / r.points_used)) <= 1e-9 * r.rms


# ------------------------------------------------------------------------------------------------ bookkeeping

def outside_scene(sigma=0.0):
    """Four timestamps of a fisheye (the lens whose theta_d has a maximum), a pinhole and a fisheye camera.  One pixel of view
    (camera 0, timestamp 1) and one of view (camera 2, timestamp 2) lie further from the principal point than any direction
    projects; timestamp 2 is seen by cameras 0 and 2 only, so it is left with one usable view.  -> (scene, expected statuses)."""
    vis = np.ones((4, 3), bool)
    vis[2, 1] = False
    s = frx.scene(7, 4, (0, 25, -25), ("FN", "P", "FN"), visible=vis, sigma=sigma, rows=12)
    K = sx.cam_K("FN")
    far = 1.02 * frx.THETA_D_MAX_FN * K[0, 0]
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[0][1][5, :2] = [K[0, 2] + far, K[1, 2]]
    kps[2][2][0, :2] = [K[0, 2], K[1, 2] - far]
    expect = np.where(vis, pnp.PNP_OK, pnp.PNP_TOO_FEW).astype(np.int32)
    expect[1, 0] = expect[2, 2] = pnp.PNP_DEGENERATE
    return s._replace(kps=kps), expect


def test_a_fisheye_view_with_a_pixel_outside_the_model():
    """The view is PNP_DEGENERATE, whatever its other rows say; its timestamp goes on with the two other cameras (1), or is left
    with one usable view, which is reported and takes no part (2).  The rig is the one the other views give, to the bit."""
    s, expect = outside_scene()
    assert np.isnan(fisheye.undistort_points_host(s.kps[0][1][5:6, :2], *sx.cam("FN"))).all()
    r, margin = solve(s, with_margin=True)
    assert r.view_status.tolist() == expect.tolist() and (r.view_points == np.where(s.visible, 12, 0)).all()
    assert r.status == rig.RIG_OK and r.stamps_used == 3 and r.points_used == 12 * 8 and margin >= MARGIN
    assert r.stamp_points.tolist() == [36, 24, 0, 36] and r.view_rms[1, 0] == 0 and not r.view_rms[2].any()
    assert not r.rvecs[2].any() and not r.tvecs[2].any() and r.stamp_rms[2] == 0
    assert r.view_status[2, 0] == pnp.PNP_OK and r.view_points[2, 0] == 12            # the lonely view
    none = np.zeros((0, 3))
    kps = [list(k) for k in s.kps]
    kps[0][1] = none
    kps[2][2] = none
    alone = rig.rig_calibrate_host_full(kps, *s.board, *frx.cam_args(s), models=frx.models(s))
    assert np.array_equal(alone.R, r.R) and np.array_equal(alone.T, r.T) and alone.rms == r.rms
    eR, eT = rx.rig_errors(r, s)
    print(f"outside pixels: 3 of 4 timestamps, |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, rms {r.rms:.2e}")
    assert eR <= TRUTH_R and eT <= TRUTH_T
    with pytest.raises(ValueError):                                       # a view that has rows and cannot be used
        rig.rig_calibrate_host(s.kps, *s.board, *frx.cam_args(s), models=frx.models(s))


def test_no_stamps_and_disconnected_stay_as_they_are():
    s = class_scene("fan3 F/P/F", 4, n_stamps=3, rows=9)
    none = np.zeros((0, 3))
    kps = [[s.kps[0][0], none, none], [none, s.kps[1][1], none], [none, none, s.kps[2][2][:3]]]
    r = rig.rig_calibrate_host_full(kps, *s.board, *frx.cam_args(s), models=frx.models(s))
    assert r.status == rig.RIG_NO_STAMPS and (r.stamps_used, r.points_used, r.rms, r.iterations, r.attempts) == (0, 0, 0.0, 0, 0)
    assert r.view_status.tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 1]] and r.parents.tolist() == [-1, -1, -1]
    r = solve(disconnected_scene())
    assert r.status == rig.RIG_DISCONNECTED and (r.stamps_used, r.points_used, r.iterations, r.attempts, r.rms) == (3, 60, 0, 0, 0.0)
    assert r.parents.tolist() == [-1, 0, -1] and (r.view_status == pnp.PNP_OK).sum() == 8
    for x in (r.R, r.T, r.rvec, r.rvecs, r.tvecs, r.stamp_rms, r.stamp_points, r.view_rms):
        assert not x.any()


def disconnected_scene():
    """Cameras 0 and 1 share timestamps 0 - 2; camera 2 sees timestamps 3 - 4 alone."""
    vis = np.array([[1, 1, 0]] * 3 + [[0, 0, 1]] * 2, bool)
    return class_scene("fan3 F/P/F", 5, n_stamps=5, visible=vis, rows=10)


# ------------------------------------------------------------------------------------------------ the model's edges

def on_axis_scene(sigma=0.0):
    """The fan with, at every timestamp, row 3 of camera 2's view (a fisheye camera behind a rig transform) exactly on that camera's
    optical axis: at r = 0 the model's series branch runs inside the rig's Jacobian."""
    s = class_scene("fan3 F/P/F", 12, rows=14)
    for t in range(6):
        s = frx.on_axis(s, t, 2, 3)
    if sigma:
        rng = np.random.default_rng(12)
        s = s._replace(kps=[[np.c_[(k[:, :2] + rng.normal(scale=sigma, size=(len(k), 2)) * (np.arange(len(k)) != 3)[:, None])
                                   .astype(np.float32).astype(np.float64), k[:, 2]] for k in kl] for kl in s.kps])
    return s


def wide_scene(sigma=0.0):
    """A pinhole and a fisheye camera that looks 58 degrees past the board, so that it sees the board between about 40 and 80 degrees
    from its axis."""
    base = frx.make_rig((0, 0), sx.BOARD_S, ("P", "F"))[0]              # side by side, then camera 1 is turned away
    yaw = rx.AXIS * np.deg2rad(58.0)
    X = np.r_[sx._compose(yaw, base[:3]), cx.f64(cx.rotation(yaw)) @ base[3:]]
    return frx.scene(13, 6, (0, 0), ("P", "F"), sigma=sigma, rows=16, rig=[X])


def test_the_edges_of_the_model():
    s = on_axis_scene()
    K = sx.cam_K(s.cams[2])
    for t in range(6):
        assert s.kps[2][t][3, :2].tolist() == [K[0, 2], K[1, 2]]          # the pixel is the principal point, exactly
    r, margin = solve(s, with_margin=True)
    eR, eT = rx.rig_errors(r, s)
    print(f"on axis: |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, rms {r.rms:.2e}, margin {margin:.3g}")
    assert r.status == rig.RIG_OK and r.stamps_used == 6 and margin >= MARGIN and eR <= TRUTH_R and eT <= TRUTH_T and r.rms <= TRUTH_RMS
    s = wide_scene()
    th = np.rad2deg([frx.theta_max(s, t, 1) for t in range(6)])
    r, margin = solve(s, with_margin=True)
    eR, eT = rx.rig_errors(r, s)
    print(f"wide: the board out to {th.max():.1f} degrees; |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, rms {r.rms:.2e}, "
          f"margin {margin:.3g}")
    assert 78.0 <= th.max() <= 86.0
    assert r.status == rig.RIG_OK and r.stamps_used == 6 and margin >= MARGIN and r.rms <= TRUTH_RMS
    assert eR <= TRUTH_R and eT <= TRUTH_T


# ------------------------------------------------------------------------------------------------ a rectified fisheye pair

SIZE = fx.SIZE
ROWS_PX = 2.0e-4            # 4 x 4.9e-5 px: the largest row disagreement of a rectified noise-free pair over seeds 1 - 3, measured here


def pair_scene(seed, sigma=0.0):
    """Two fisheye cameras 30 degrees apart, 6 timestamps."""
    return frx.scene(seed, 6, (0, 30), ("F", "F0"), sigma=sigma)


def common_rows(s, t):
    """The pixels of the ids both cameras saw at timestamp t -> ((n, 2), (n, 2)), id-sorted."""
    a, b = s.kps[0][t], s.kps[1][t]
    ids = np.intersect1d(a[:, 2], b[:, 2])
    return (np.array([a[a[:, 2] == i][0, :2] for i in ids]).reshape(-1, 2), np.array([b[b[:, 2] == i][0, :2] for i in ids]).reshape(-1, 2))


def rectification_of(s, r):
    cameras, dists = frx.cam_args(s)
    R, T, _, _ = rig.rig_pair(r, 0, 1, *cameras)
    return fisheye.stereo_rectify_fisheye_host(cameras[0], dists[0], cameras[1], dists[1], SIZE, R, T)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_rectified_fisheye_pair_shares_its_rows(seed):
    """The pair's rig from rig_calibrate_host_full, stereo_rectify_fisheye_host, rectify_points_fisheye_host on both cameras' pixels
    of the same corners: they land on the same row."""
    s = pair_scene(seed)
    cameras, dists = frx.cam_args(s)
    rect = rectification_of(s, solve(s))
    worst, n = 0.0, 0
    for t in range(6):
        p0, p1 = common_rows(s, t)
        q0 = fisheye.rectify_points_fisheye_host(p0, cameras[0], dists[0], rect.R1, rect.P1)
        q1 = fisheye.rectify_points_fisheye_host(p1, cameras[1], dists[1], rect.R2, rect.P2)
        worst, n = max(worst, float(np.abs(q0[:, 1] - q1[:, 1]).max())), n + len(p0)
        assert ((q0[:, 0] - q1[:, 0]) * np.sign(-rect.Tn) > 0).all()                  # a positive disparity along the baseline
    print(f"{s.tag}: {n} corners seen by both, rows differ by at most {worst:.2e} px (gate {ROWS_PX:.1e}); Tn {rect.Tn:.4f} m")
    assert rect.axis == 0 and n >= 40 and worst <= ROWS_PX


def test_the_rectifying_rotations_are_the_pinhole_call_s():
    """R1, R2, axis and Tn do not depend on a camera: stereo_rectify_host's bits.  f and the principal point are the documented
    ones, and P1, P2, Q take stereo_rectify_host's forms."""
    from deepcharuco_amd import rectify
    s = pair_scene(1)
    (K0, K1), (k0, k1) = frx.cam_args(s)
    R, T = cx.f64(cx.rotation(s.X[0, :3])), s.X[0, 3:]
    a = fisheye.stereo_rectify_fisheye_host(K0, k0, K1, k1, SIZE, R, T)
    long = fx.camera(600.0)              # (a pinhole of these focal lengths does not hold the turned frame's corners)
    b = rectify.stereo_rectify_host(long, None, long, None, SIZE, R, T)
    assert np.array_equal(a.R1, b.R1) and np.array_equal(a.R2, b.R2) and a.axis == b.axis == 0 and a.Tn == b.Tn
    f, cxy = min(K0[1, 1], K1[1, 1]), ((SIZE[0] - 1) / 2, (SIZE[1] - 1) / 2)
    assert a.P1.tolist() == [[f, 0, cxy[0], 0], [0, f, cxy[1], 0], [0, 0, 1, 0]]
    assert a.P2[0, 3] == a.Tn * f and np.array_equal(np.delete(a.P2, 3, 1), np.delete(a.P1, 3, 1))
    assert a.Q.tolist() == [[1, 0, 0, -cxy[0]], [0, 1, 0, -cxy[1]], [0, 0, 0, f], [0, 0, -1.0 / a.Tn, 0]]
    wide = fisheye.stereo_rectify_fisheye_host(K0, k0, K1, k1, SIZE, R, T, focal=90.0)
    assert wide.P1[0, 0] == wide.P1[1, 1] == 90.0 and np.array_equal(wide.R1, a.R1)
    vertical = fisheye.stereo_rectify_fisheye_host(K0, k0, K1, k1, SIZE, np.eye(3), [0.0, 0.1, 0.01])
    assert vertical.axis == 1 and vertical.P2[1, 3] == vertical.Tn * f
    for kw in (dict(T=[0, 0, 0]), dict(focal=0.0), dict(focal=math.inf), dict(image_size=(1, 480)), dict(dist1=np.zeros(5))):
        args = dict(camera0=K0, dist0=k0, camera1=K1, dist1=k1, image_size=SIZE, R=R, T=T)
        with pytest.raises(ValueError):
            fisheye.stereo_rectify_fisheye_host(**{**args, **kw})


# ------------------------------------------------------------------------------------------------ the two-camera solver

STEREO_PAIRS = [("F", "F0"), ("P", "F"), ("F", "P")]


def stereo_args(s):
    """A two-camera scene's arguments of the ``stereo_calibrate_*`` calls -> (positional, keyword)."""
    (K0, K1), (d0, d1) = frx.cam_args(s)
    return (s.kps[0], s.kps[1], *s.board, K0, d0, K1, d1), dict(models=frx.models(s))


def test_stereo_defaults_are_the_definition_as_it_was():
    """test_stereo_host's first case: ``models=None`` and ("pinhole", "pinhole") give the same bits, F included."""
    s = sx.scene(1, 6, "small", sx.BOARD_S, "A", "B")
    a = stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *sx.cam_args(s))
    b = stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *sx.cam_args(s), models=("pinhole", "pinhole"))
    assert a.status == stereo.STEREO_OK and a.F is not None and a.F[2, 2] == 1.0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for bad in (("pinhole",), ("pinhole", "wide")):
        with pytest.raises(ValueError):
            stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *sx.cam_args(s), models=bad)
    with pytest.raises(ValueError):                                       # camera B's five coefficients are no fisheye's
        stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *sx.cam_args(s), models=("pinhole", "fisheye"))


@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("cams", STEREO_PAIRS, ids=["/".join(c) for c in STEREO_PAIRS])
def test_two_cameras_are_the_stereo_definition(cams, sigma):
    """A two-camera rig with ``models`` equals stereo_calibrate_host_full(models=...) to 1e-9 (test_rig_host's gate), a TOO_FEW
    view included; F is None with a fisheye camera in the pair, E is [T]x R."""
    s = frx.scene(3, 6, (0, 30), cams, sigma=sigma)
    kps = [list(s.kps[0]), list(s.kps[1])]
    kps[0][2] = kps[0][2][:3]
    s = s._replace(kps=kps)
    r = solve(s)
    args, kw = stereo_args(s)
    h, margin = stereo.stereo_calibrate_host_full(*args, with_margin=True, **kw)
    g = {"R": float(np.abs(r.R[1] - h.R).max()), "T": float(np.linalg.norm(r.T[1] - h.T) / np.linalg.norm(h.T)),
         "P": float(max(np.abs(r.rvecs - h.rvecs).max(), (np.linalg.norm(r.tvecs - h.tvecs, axis=1)).max() / np.linalg.norm(h.tvecs[0]))),
         "rms": abs(r.rms - h.rms) / h.rms, "view rms": float(np.abs(r.view_rms - h.view_rms).max())}
    print(f"{s.tag}: rig - stereo gaps {g}; steps rig {r.iterations} / {r.attempts}, stereo {h.iterations} / {h.attempts}, margin {margin:.3g}")
    assert (r.status, r.stamps_used, r.points_used) == (h.status, h.pairs_used, h.points_used) == (rig.RIG_OK, 5, h.points_used)
    assert r.view_status.tolist() == h.view_status.tolist() and r.view_points.tolist() == h.view_points.tolist()
    assert r.stamp_points.tolist() == h.pair_points.tolist() and margin >= MARGIN
    assert max(g["R"], g["T"], g["P"]) <= 1e-9 and g["rms"] <= 1e-9 and g["view rms"] <= 1e-9 * 400
    assert h.F is None and np.array_equal(h.E, pnp._skew(h.T) @ h.R)
    with pytest.raises(ValueError):                                       # the 3-row view
        stereo.stereo_calibrate_host(*args, **kw)
    ok = stereo.stereo_calibrate_host(*[a[:2] if i < 2 else a for i, a in enumerate(args)], **kw)
    assert len(ok) == 9 and ok[8] is None and ok[0] > 0
