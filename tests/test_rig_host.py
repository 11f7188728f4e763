"""The host definition of the rig calibration (deepcharuco_amd/rig.py, rig_calibrate_host_full) against the exact camera model of
tests/camera_exact.py, on the C-camera scenes of tests/rig_exact.py: the analytic Jacobian, truth recovery on fans and on a chain
whose far cameras never see the board together with camera 0, the stationary point on noisy scenes, C = 2 against the stereo
definition, the bookkeeping of unusable views and of rigs that fall apart, the epipolar constraint of a pair taken out of the
rig, and the masks that compose it with the consensus solvers.  No GPU.  The gates are test_stereo_host's, imported.  Every test
prints what it measured."""
import math

import numpy as np
import pytest

import camera_exact as cx
import rig_exact as rx
import stereo_exact as sx
from deepcharuco_amd import pnp, rig, stereo
from test_stereo_host import EPI_PX, RANSAC, TRUTH_R, TRUTH_RMS, TRUTH_T

FAN3 = dict(angles=(0, 25, -25), cams=("A", "B", "C"))
FAN4 = dict(angles=(0, 20, -20, 40), cams=("A", "B", "C", "A4"))
CHAIN4 = dict(angles=(0, 20, 40, 60), cams=("A", "B", "C", "A4"))


def _solve(s, **kw):
    return rig.rig_calibrate_host_full(s.kps, *s.board, *rx.cam_args(s), **kw)


def _xp(r):
    used = np.flatnonzero((r.view_status == pnp.PNP_OK).sum(1) >= 2)
    return np.c_[r.rvec, r.T][1:], np.c_[r.rvecs, r.tvecs][used], used


def chain_scene(seed=1, sigma=0.0, rows=cx.n_ids(sx.BOARD_S)):
    """Cameras at 0 / 20 / 40 / 60 degrees, 12 timestamps: four seen by (0, 1) only, four by (1, 2) only, four by (2, 3) only.
    Every view holds the whole board: a P_t is fixed by the two views of its own timestamp alone, and it is held to a gate that
    was measured on a rig rotation, which pools every row of a scene; with the 6 .. 60 rows per view the fans draw, a 9- or
    14-row view leaves its timestamp's rotation at 2.0e-7, the float32 rounding of so few image points and no solver's error."""
    return rx.scene(seed, 12, visible=rx.chain_visibility(4, 4), sigma=sigma, rows=rows, **CHAIN4)


# ------------------------------------------------------------------------------------------------ the Jacobian

def test_analytic_jacobian_matches_exact_finite_differences():
    """J_X and J_P of three cameras' rows against central differences of the exact model, away from the solution.  Gate: 1e-10 of
    the column's largest entry, test_stereo_host's."""
    s = rx.scene(11, 3, rows=9, **FAN3)
    rng = np.random.default_rng(5)
    X = s.X + rng.normal(scale=1e-2, size=s.X.shape) * np.r_[1, 1, 1, [np.linalg.norm(s.X[0, 3:])] * 3]
    P = s.P + rng.normal(scale=1e-2, size=s.P.shape) * np.r_[1, 1, 1, [np.linalg.norm(s.P[0, 3:])] * 3]
    views = rx.pool_views(s, range(3))
    rows = rig._rows_of(views, 3)
    cams = [(pnp._camera(K), pnp._dist(d)) for K, d in zip(*rx.cam_args(s))]
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
    Jfd = rx.jacobian_fd(views, s, X, P)
    gap_r = float(np.abs(res - cx.f64(rx.residuals(views, s, X, P))).max())
    gap = float((np.abs(J - Jfd).max(0) / np.abs(Jfd).max(0)).max())
    print(f"{s.tag}: residuals within {gap_r:.2e} px, Jacobian columns within {gap:.2e} of their largest entry")
    assert gap_r <= 1e-10 and gap <= 1e-10


# ------------------------------------------------------------------------------------------------ truth

def _pose_errors(r, s, used):
    eR = max(float(np.abs(pnp._rodrigues(r.rvecs[t]) - cx.f64(cx.rotation(s.P[t, :3]))).max()) for t in used)
    eT = max(float(np.linalg.norm(r.tvecs[t] - s.P[t, 3:]) / np.linalg.norm(s.P[t, 3:])) for t in used)
    return eR, eT


@pytest.mark.parametrize("name", ["fan3", "fan4", "chain4"])
def test_truth_recovery_noise_free_float32(name):
    """Every X_c and every P_t (on the chain also those of the timestamps camera 0 never saw) inside test_stereo_host's truth
    gates; the chain's tree is 0 - 1 - 2 - 3."""
    s = {"fan3": lambda: rx.scene(1, 8, **FAN3), "fan4": lambda: rx.scene(1, 8, **FAN4), "chain4": chain_scene}[name]()
    r = _solve(s)
    T = len(s.P)
    eR, eT = rx.rig_errors(r, s)
    pR, pT = _pose_errors(r, s, range(T))
    print(f"{s.tag}: |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, board poses {pR:.2e} / {pT:.2e}, rms {r.rms:.2e} px, "
          f"steps {r.iterations} / {r.attempts}, parents {r.parents.tolist()}")
    assert r.status == rig.RIG_OK and r.stamps_used == T
    assert (r.view_status == pnp.PNP_OK).tolist() == s.visible.tolist()
    assert r.points_used == sum(len(k) for kl in s.kps for k in kl) == int(r.view_points.sum()) == int(r.stamp_points.sum())
    assert r.parents.tolist() == ([-1, 0, 1, 2] if name == "chain4" else [-1] + [0] * (len(s.cams) - 1))
    assert np.array_equal(r.R[0], np.eye(3)) and not r.T[0].any() and not r.rvec[0].any()
    assert eR <= TRUTH_R and eT <= TRUTH_T and r.rms <= TRUTH_RMS
    assert pR <= TRUTH_R and pT <= TRUTH_T


@pytest.mark.parametrize("name", ["fan3", "fan4", "chain4"])
def test_noisy_scene_ends_at_a_stationary_point_no_higher_than_the_truth(name):
    """sigma = 0.3 px: the cost at the result is no higher than at the truth, |J^T r| <= 1e-6 |J| |r| with the exact model's
    finite-difference Jacobian, and the rms is that cost's."""
    s = {"fan3": lambda: rx.scene(2, 5, sigma=0.3, rows=14, **FAN3), "fan4": lambda: rx.scene(2, 4, sigma=0.3, rows=12, **FAN4),
         "chain4": lambda: rx.scene(2, 6, visible=rx.chain_visibility(4, 2), sigma=0.3, rows=14, **CHAIN4)}[name]()
    r = _solve(s)
    assert r.status == rig.RIG_OK and r.stamps_used == len(s.P)
    X, P, used = _xp(r)
    views = rx.pool_views(s, used)
    c_res, grad = rx.stationarity(views, s, X, P)
    c_true = rx.cost(views, s, s.X, s.P)
    print(f"{s.tag}: cost {c_res:.6f} (truth {c_true:.6f}), |Jtr| / (|J||r|) {grad:.2e}, rms {r.rms:.4f} px, rig error "
          f"{rx.rig_errors(r, s)}, steps {r.iterations} / {r.attempts}")
    assert c_res <= c_true and grad <= 1e-6
    assert abs(r.rms - math.sqrt(c_res / r.points_used)) <= 1e-9 * r.rms


# ------------------------------------------------------------------------------------------------ C = 2

@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_two_cameras_are_the_stereo_definition(sigma):
    s = rx.scene(3, 6, (0, 30), ("A", "B"), sigma=sigma)
    kps = [list(s.kps[0]), list(s.kps[1])]
    kps[0][2] = kps[0][2][:3]                                            # TOO_FEW: the timestamp is not used by either
    r = rig.rig_calibrate_host_full(kps, *s.board, *rx.cam_args(s))
    h = stereo.stereo_calibrate_host_full(kps[0], kps[1], *s.board, *sx.cam("A"), *sx.cam("B"))
    g = {"R": float(np.abs(r.R[1] - h.R).max()), "T": float(np.linalg.norm(r.T[1] - h.T) / np.linalg.norm(h.T)),
         "P": float(max(np.abs(r.rvecs - h.rvecs).max(), (np.linalg.norm(r.tvecs - h.tvecs, axis=1)).max() / np.linalg.norm(h.tvecs[0]))),
         "rms": abs(r.rms - h.rms) / h.rms, "view rms": float(np.abs(r.view_rms - h.view_rms).max())}
    print(f"C = 2 sigma {sigma}: rig - stereo gaps {g}; steps rig {r.iterations} / {r.attempts}, stereo {h.iterations} / {h.attempts}")
    assert (r.status, r.stamps_used, r.points_used) == (h.status, h.pairs_used, h.points_used) == (rig.RIG_OK, 5, h.points_used)
    assert r.view_status.tolist() == h.view_status.tolist() and r.view_points.tolist() == h.view_points.tolist()
    assert r.stamp_points.tolist() == h.pair_points.tolist() and r.parents.tolist() == [-1, 0]
    assert not r.rvecs[2].any() and not r.stamp_rms[2].any()
    assert max(g["R"], g["T"], g["P"]) <= 1e-9 and g["rms"] <= 1e-9 and g["view rms"] <= 1e-9 * 400


# ------------------------------------------------------------------------------------------------ bookkeeping

def _bookkeeping_scene():
    """Three cameras, 8 timestamps: 0 fine, 1 camera 0 with 3 rows, 2 camera 1 with an id outside the board, 3 a 4-row view of
    camera 2, 4 seen by camera 0 only (usable and alone), 5 by cameras 1 and 2 only, 6 - 7 fine."""
    rows = [[12, 9, 10]] * 3 + [[12, 9, 4]] + [[12, 9, 10]] * 4
    vis = np.ones((8, 3), bool)
    vis[4, 1:] = False
    vis[5, 0] = False
    s = rx.scene(4, 8, visible=vis, rows=rows, **FAN3)
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[0][1] = kps[0][1][:3]
    kps[1][2][5, 2] = cx.n_ids(s.board)
    expect = np.where(vis, pnp.PNP_OK, pnp.PNP_TOO_FEW).astype(np.int32)
    expect[1, 0], expect[2, 1] = pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID
    return s._replace(kps=kps), expect


def test_bookkeeping_of_unusable_and_lonely_views():
    s, expect = _bookkeeping_scene()
    r = _solve(s)
    n = np.array([[len(s.kps[c][t]) for c in range(3)] for t in range(8)])
    assert r.view_status.tolist() == expect.tolist() and r.view_points.tolist() == n.tolist()
    used = [0, 1, 2, 3, 5, 6, 7]                                          # (1 and 2 keep two usable views each)
    part = (expect == pnp.PNP_OK) & np.isin(np.arange(8), used)[:, None]
    assert r.status == rig.RIG_OK and r.stamps_used == 7
    assert r.stamp_points.tolist() == (n * part).sum(1).tolist() and r.points_used == int((n * part).sum())
    # the lonely view: usable, reported, unused, zero outputs
    assert r.view_status[4, 0] == pnp.PNP_OK and r.view_points[4, 0] == 12
    assert not r.rvecs[4].any() and not r.tvecs[4].any() and r.stamp_rms[4] == 0 and r.stamp_points[4] == 0 and not r.view_rms[4].any()
    assert (r.view_rms[part] > 0).all() and not r.view_rms[~part].any() and (r.stamp_rms[used] > 0).all()
    eR, eT = rx.rig_errors(r, s)
    pR, pT = _pose_errors(r, s, used)
    print(f"bookkeeping: 7 of 8 timestamps, |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, board poses {pR:.2e} / {pT:.2e}")
    assert eR <= TRUTH_R and eT <= TRUTH_T and pR <= TRUTH_R and pT <= TRUTH_T
    # the used timestamps alone give the same bits: a timestamp left out leaves no trace
    alone = rig.rig_calibrate_host_full([[kl[t] for t in used] for kl in s.kps], *s.board, *rx.cam_args(s))
    assert np.array_equal(alone.R, r.R) and np.array_equal(alone.T, r.T) and alone.rms == r.rms
    with pytest.raises(IndexError):
        rig.rig_calibrate_host(s.kps, *s.board, *rx.cam_args(s))
    with pytest.raises(ValueError):
        rig.rig_calibrate_host([kl[:2] for kl in s.kps], *s.board, *rx.cam_args(s))          # a 3-row view
    ok = rig.rig_calibrate_host([[kl[t] for t in (0, 4, 5, 6)] for kl in s.kps], *s.board, *rx.cam_args(s))   # empty views are fine
    assert len(ok) == 3 and ok[0] > 0 and ok[1].shape == (3, 3, 3) and ok[2].shape == (3, 3, 1)


def test_views_without_a_common_id_recover_the_rig():
    s = rx.scene(3, 8, rows=20, **FAN3)
    ids = np.random.default_rng(3).permutation(cx.n_ids(s.board))
    share = [set(ids[:20].tolist()), set(ids[20:40].tolist()), set(ids[40:].tolist())]
    full = rx.scene(3, 8, rows=cx.n_ids(s.board), **FAN3)
    kps = [[k[np.isin(k[:, 2], list(share[c]))] for k in full.kps[c]] for c in range(3)]
    for t in range(8):
        assert not set(kps[0][t][:, 2]) & set(kps[1][t][:, 2]) and not set(kps[1][t][:, 2]) & set(kps[2][t][:, 2])
    r = rig.rig_calibrate_host_full(kps, *s.board, *rx.cam_args(s))
    eR, eT = rx.rig_errors(r, full)
    print(f"disjoint ids: |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, rms {r.rms:.2e}")
    assert r.status == rig.RIG_OK and r.stamps_used == 8 and eR <= TRUTH_R and eT <= TRUTH_T


def test_no_stamps():
    s = rx.scene(4, 3, rows=9, **FAN3)
    none = np.zeros((0, 3))
    kps = [[s.kps[0][0], none, none], [none, s.kps[1][1], none], [none, none, s.kps[2][2][:3]]]
    r = rig.rig_calibrate_host_full(kps, *s.board, *rx.cam_args(s))
    assert r.status == rig.RIG_NO_STAMPS and (r.stamps_used, r.points_used, r.rms, r.iterations, r.attempts) == (0, 0, 0.0, 0, 0)
    assert r.view_status.tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 1]] and r.view_points.tolist() == [[9, 0, 0], [0, 9, 0], [0, 0, 3]]
    assert r.parents.tolist() == [-1, -1, -1]
    for x in (r.R, r.T, r.rvec, r.rvecs, r.tvecs, r.stamp_rms, r.stamp_points, r.view_rms):
        assert not x.any()
    with pytest.raises(ValueError):
        rig.rig_calibrate_host(kps, *s.board, *rx.cam_args(s))


def disconnected_scene():
    """Cameras 0 and 1 share timestamps 0 - 2; camera 2 sees timestamps 3 - 4 alone."""
    vis = np.array([[1, 1, 0]] * 3 + [[0, 0, 1]] * 2, bool)
    return rx.scene(5, 5, visible=vis, rows=10, **FAN3)


def test_disconnected():
    r = _solve(disconnected_scene())
    assert r.status == rig.RIG_DISCONNECTED and (r.stamps_used, r.points_used, r.iterations, r.attempts, r.rms) == (3, 60, 0, 0, 0.0)
    assert r.parents.tolist() == [-1, 0, -1] and (r.view_status == pnp.PNP_OK).sum() == 8
    for x in (r.R, r.T, r.rvec, r.rvecs, r.tvecs, r.stamp_rms, r.stamp_points, r.view_rms):
        assert not x.any()


# ------------------------------------------------------------------------------------------------ a pair out of the rig

def test_rig_pair_meets_the_epipolar_constraint():
    """Cameras 1 and 2 of the noise-free chain, which the initialisation links directly: exact, undistorted pixel coordinates of the
    same board points in both, their distance from the other's epipolar line through rig_pair's F, in pixels."""
    s = chain_scene()
    r = _solve(s)
    K1, K2 = sx.cam_K(s.cams[1]), sx.cam_K(s.cams[2])
    R, T, E, F = rig.rig_pair(r, 1, 2, K1, K2)
    obj = cx.board_points(np.arange(cx.n_ids(s.board)), *s.board)
    w = 0.0
    for P in s.P[4:8]:                                                    # the timestamps both of them saw
        x1 = np.c_[cx.f64(sx.project_rig(obj, P, s.X[0], K1, None)), np.ones(len(obj))]
        x2 = np.c_[cx.f64(sx.project_rig(obj, P, s.X[1], K2, None)), np.ones(len(obj))]
        e = np.abs(np.einsum("ni,ij,nj->n", x2, F, x1))
        w = max(w, float((e / np.linalg.norm((x1 @ F.T)[:, :2], axis=1)).max()), float((e / np.linalg.norm((x2 @ F)[:, :2], axis=1)).max()))
    back = rig.rig_pair(r, 2, 1, K2, K1)
    print(f"rig_pair(1, 2): worst point-to-line distance {w:.3e} px (gate {EPI_PX:.1e})")
    assert F[2, 2] == 1.0 and np.array_equal(E, pnp._skew(T) @ R) and w <= EPI_PX
    assert np.abs(back[0] - R.T).max() <= 1e-15 and np.abs(back[1] + R.T @ T).max() <= 1e-12
    R01, T01, _, _ = rig.rig_pair(r, 0, 1, sx.K_A, K1)
    assert np.array_equal(R01, r.R[1]) and np.array_equal(T01, r.T[1])
    with pytest.raises(ValueError):
        rig.rig_pair(r, 1, 1, K1, K1)
    with pytest.raises(ValueError):
        rig.rig_pair(_solve(disconnected_scene()), 0, 1, sx.K_A, K1)


# ------------------------------------------------------------------------------------------------ masks, errors

def planted_scene():
    """sigma = 0.3 px, three cameras, 6 timestamps, 20 rows per view; in every view two pairs of rows exchange their ids (at least
    two grid steps apart) -> (scene, good-row masks per camera)."""
    s = rx.scene(5, 6, sigma=0.3, rows=20, **FAN3)
    rng = np.random.default_rng(77)
    good = [[], [], []]
    for c in range(3):
        for kp in s.kps[c]:
            g = np.ones(20, bool)
            grid = cx.grid_xy(kp[:, 2], s.board[1])
            done = 0
            while done < 2:
                a, b = rng.choice(20, 2, replace=False)
                if g[a] and g[b] and np.abs(grid[a] - grid[b]).max() >= 2:
                    kp[[a, b], 2] = kp[[b, a], 2]
                    g[[a, b]] = False
                    done += 1
            good[c].append(g)
    return s, good


def test_masks_from_the_consensus_solver():
    s, good = planted_scene()
    cameras, dists = rx.cam_args(s)
    masks = [[pnp.solve_pnp_ransac_host(kp, *s.board, cameras[c], dists[c], **RANSAC)[3] for kp in s.kps[c]] for c in range(3)]
    assert all(np.array_equal(m, g) for c in range(3) for m, g in zip(masks[c], good[c]))
    masked = _solve(s, masks=masks)
    true_rows = rig.rig_calibrate_host_full([[k[g] for k, g in zip(s.kps[c], good[c])] for c in range(3)], *s.board, cameras, dists)
    for a, b in zip(masked, true_rows):
        assert np.array_equal(a, b)
    plain = _solve(s)
    eM, eP = rx.rig_errors(masked, s), rx.rig_errors(plain, s)
    print(f"planted: masked rms {masked.rms:.3f} px, rig error {eM}; unmasked rms {plain.rms:.3f} px (status {plain.status}), rig "
          f"error {eP}")
    assert masked.status == rig.RIG_OK and (masked.view_points == 16).all() and masked.points_used == 6 * 48
    # the planted rows are ~25 px off: they hurt the plain solve (if it ends at all) by more than ten times the masked rms, which is
    # the noise's; the masked rig is right to the noise
    assert plain.status != rig.RIG_OK or (plain.rms >= 10 * masked.rms and eP[0] >= 10 * eM[0])
    assert masked.rms <= 0.45 and eM[0] <= 1e-2
    ones = _solve(s, masks=[[np.ones(20, bool)] * 6, None, None])
    for a, b in zip(ones, plain):
        assert np.array_equal(a, b)
    short = [m.copy() for m in masks[1]]
    short[2][:] = False
    short[2][:3] = True
    r = _solve(s, masks=[masks[0], short, masks[2]])
    assert r.view_status[2].tolist() == [pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_OK] and r.stamps_used == 6 and r.view_points[2, 1] == 3
    assert r.stamp_points[2] == 32


def test_argument_errors():
    s = rx.scene(1, 2, rows=9, **FAN3)
    cameras, dists = rx.cam_args(s)
    skew = sx.K_A.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError):
        rig.rig_calibrate_host_full(s.kps, *s.board, [skew] + cameras[1:], dists)
    with pytest.raises(ValueError):
        rig.rig_calibrate_host_full(s.kps, *s.board, cameras, [np.zeros(12)] + dists[1:])
    with pytest.raises(ValueError):
        rig.rig_calibrate_host_full(s.kps[:1], *s.board, cameras[:1], dists[:1])            # one camera
    with pytest.raises(ValueError):
        rig.rig_calibrate_host_full([s.kps[0]] * 9, *s.board, [cameras[0]] * 9, None)       # nine
    with pytest.raises(ValueError):
        rig.rig_calibrate_host_full(s.kps[:2], *s.board, cameras, dists)                    # two lists for three cameras
    with pytest.raises(ValueError):
        rig.rig_calibrate_host_full([s.kps[0], s.kps[1][:1], s.kps[2]], *s.board, cameras, dists)
    with pytest.raises(ValueError):
        _solve(s, masks=[[np.ones(3, bool), None], None, None])
    with pytest.raises(ValueError):
        _solve(s, masks=[None, None])
    assert rig.RIG_DISCONNECTED == 4 and (rig.RIG_OK, rig.RIG_NO_STAMPS, rig.RIG_DEGENERATE, rig.RIG_NONFINITE) == (0, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ one text for both definitions

def test_stereo_and_rig_tables_run_through_one_evaluate_and_one_normal_blocks():
    """Two timestamps, four rows per view, a distorted pinhole and a plain one.  The row table built the stereo way (per pair) and
    the rig way (per timestamp its views) is one table, res / J_X / J_P come out of the one ``_evaluate`` equal bit for bit
    whether X is stereo's [6] or the rig's [1, 6], and ``_normal_blocks`` under the two segmentations of the J_X sums (per pair,
    per view) gives the same bits wherever no J_X enters: U, g_b and the costs.  (W, V and g_a may differ by rounding: numpy adds a
    pair's rows in another order than its two views' rows, which is why the segmentation is an argument.)"""
    s = rx.scene(21, 2, (0, 30), ("B", "A"), rows=4)
    stamps = rx.pool_views(s, range(2))
    by_view = rig._rows_of(stamps, 2)
    by_pair = stereo._rows_of([(v[0][1], v[0][2], v[1][1], v[1][2]) for v in stamps])
    assert by_view.obj.shape == (16, 3) and by_view.n_cams == by_pair.n_cams == 2
    for a, b in zip(by_view[:-1], by_pair[:-1]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    cams = [(pnp._camera(K), pnp._dist(d)) for K, d in zip(*rx.cam_args(s))]
    rng = np.random.default_rng(6)
    X = s.X[0] + rng.normal(scale=1e-3, size=6)
    P = s.P + rng.normal(scale=1e-3, size=s.P.shape)
    one, two = stereo._evaluate(by_pair, cams, X, P, True), stereo._evaluate(by_view, cams, X[None], P, True)
    assert all(np.array_equal(a, b) for a, b in zip(one, two))
    assert not one[1][by_pair.cam == 0].any() and one[1][by_pair.cam == 1].any()
    pair = stereo._normal_blocks(by_pair, cams, X, P, stereo._pair_segments(by_pair))
    view = stereo._normal_blocks(by_view, cams, X[None], P, stereo._view_segments(by_view))
    for i, name in ((0, "U"), (4, "gb"), (5, "costs")):
        assert np.array_equal(pair[i], view[i]), name
    gaps = {name: float(np.abs(pair[i] - view[i]).max()) for i, name in ((1, "W"), (2, "V"), (3, "ga"))}
    print(f"per pair against per view: U, gb, costs equal; largest gaps {gaps}")
    assert pair[1].shape == (2, 6, 6) and pair[2].shape == (6, 6) and pair[5].shape == (2, 2)


def test_the_row_table_of_a_rig_with_absent_cameras():
    """Three cameras, three timestamps; camera 1 is absent at timestamp 1 and camera 0 at timestamp 2.  The per-view loop and
    ``_rows_of`` that both definitions call give the table ``rig_calibrate_host_full`` has always built: written out here."""
    vis = np.ones((3, 3), bool)
    vis[1, 1] = vis[2, 0] = False
    s = rx.scene(22, 3, visible=vis, rows=[[4, 5, 6], [5, 4, 6], [6, 5, 4]], **FAN3)
    cams = rig._cameras(*rx.cam_args(s))[0]
    view_status, view_points, poses, obj_l, img_l = stereo._view_poses(s.kps, [None] * 3, cams, s.board, False)
    few = pnp.PNP_TOO_FEW
    assert view_status.tolist() == [[0, 0, 0], [0, few, 0], [few, 0, 0]] and view_status.dtype == np.int32
    assert view_points.tolist() == [[4, 5, 6], [5, 0, 6], [0, 5, 4]]
    assert obj_l[1][1] is None and img_l[2][0] is None and not poses[1, 1].any() and not poses[2, 0].any()
    assert poses.shape == (3, 3, 6) and all(poses[t, c].any() for t in range(3) for c in range(3) if vis[t, c])
    usable = view_status == pnp.PNP_OK
    rows = rig._rows_of([[(c, obj_l[t][c], img_l[t][c]) for c in range(3) if usable[t, c]] for t in range(3)], 3)
    assert rows.vstamp.tolist() == [0, 0, 0, 1, 1, 2, 2] and rows.vcam.tolist() == [0, 1, 2, 0, 2, 1, 2]
    assert rows.starts.tolist() == [0, 15, 26] and rows.vstarts.tolist() == [0, 4, 9, 15, 20, 26, 31]
    assert rows.cam.tolist() == [0] * 4 + [1] * 5 + [2] * 6 + [0] * 5 + [2] * 6 + [1] * 5 + [2] * 4
    assert rows.stamp.tolist() == [0] * 15 + [1] * 11 + [2] * 9 and rows.n_cams == 3
    assert rows.obj.dtype == rows.img.dtype == np.float64 and rows.obj.shape == (35, 3) and rows.img.shape == (35, 2)
    want = rx.pool_views(s, range(3))                                     # the rows themselves, in pool order
    assert np.array_equal(rows.obj, np.concatenate([o for v in want for _, o, _ in v]).astype(np.float64))
    assert np.array_equal(rows.img, np.concatenate([m for v in want for _, _, m in v]))
    r = _solve(s)
    assert r.status == rig.RIG_OK and r.stamps_used == 3 and r.points_used == 35 and r.view_status.tolist() == view_status.tolist()
