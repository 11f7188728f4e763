"""The host definition of the stereo calibration (deepcharuco_amd/stereo.py, stereo_calibrate_host_full) against the exact camera
model of tests/camera_exact.py, on the two-camera scenes of tests/stereo_exact.py: the analytic Jacobian, truth recovery, the
stationary point on noisy scenes, views without a common id, the bookkeeping of unusable views, the epipolar constraint and the
masks that compose it with the consensus solvers.  No GPU.  Every test prints what it measured."""
import math

import numpy as np
import pytest

import camera_exact as cx
import stereo_exact as sx
from deepcharuco_amd import pnp, stereo

RIGS = ("small", "toe90", "r170")
# camera pairs: K0 != K1 with fx != fy in every one; distortion none / 5 / 8, mixed between the cameras
CAM_PAIRS = (("A", "B"), ("B", "C"), ("C", "A"))

# Noise-free truth recovery: the host definition's own worst errors over TRUTH_CASES, measured by this test on the CPU
# (DESIGN 3.10's table): rotation 4.17e-8 -> 4.2e-8 (max |R - R_true|), translation 8.58e-8 -> 8.6e-8 (relative), rms 5.81e-6 -> 5.9e-6 px (the float32 rounding of
# the image points).  The gates are those x 4, for libm and summation differences between numpy builds.
TRUTH_R, TRUTH_T, TRUTH_RMS = 4 * 4.2e-8, 4 * 8.6e-8, 4 * 5.9e-6
TRUTH_CASES = [(rig, c0, c1, board) for rig in RIGS for (c0, c1), board in zip(CAM_PAIRS, (sx.BOARD_S, sx.BOARD_L, sx.BOARD_S))]


def _solve(s, **kw):
    return stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *sx.cam_args(s), **kw)


def _xp(r, used=None):
    used = np.flatnonzero((r.view_status == pnp.PNP_OK).all(1)) if used is None else used
    return np.r_[r.rvec, r.T], np.c_[r.rvecs, r.tvecs][used]


# ------------------------------------------------------------------------------------------------ the Jacobian

@pytest.mark.parametrize("rig,c0,c1", [("small", "A", "B"), ("toe90", "B", "C"), ("r170", "C", "A4")])
def test_analytic_jacobian_matches_exact_finite_differences(rig, c0, c1):
    """J_X and J_P of both cameras' rows against central differences of the exact model, away from the solution (so that no
    column is small by accident).  Gate: 1e-10 of the column's largest entry; the finite differences themselves are good to
    ~1e-12 (truncation) + 1e-13 (rounding) of a column's size (camera_exact.jacobian_fd)."""
    s = sx.scene(11, 3, rig, sx.BOARD_S, c0, c1, rows=9)
    rng = np.random.default_rng(5)
    X = s.X + rng.normal(scale=1e-2, size=6) * np.r_[1, 1, 1, [np.linalg.norm(s.X[3:])] * 3]
    P = s.P + rng.normal(scale=1e-2, size=s.P.shape) * np.r_[1, 1, 1, [np.linalg.norm(s.P[0, 3:])] * 3]
    views = sx.pool_views(s)
    rows = stereo._rows_of(views)
    cams = [(pnp._camera(K), pnp._dist(d)) for K, d in (sx.cam(c0), sx.cam(c1))]
    res, JX, JP = stereo._evaluate(rows, cams, X, P, True)
    M, N = rows.obj.shape[0], len(views)
    J = np.zeros((2 * M, 6 + 6 * N))
    J[:, :6] = JX.reshape(2 * M, 6)
    for i in range(N):
        sel = np.repeat(rows.pair == i, 2)
        J[sel, 6 + 6 * i:12 + 6 * i] = JP.reshape(2 * M, 6)[sel]
    assert not JX[rows.cam == 0].any()
    Jfd = sx.jacobian_fd(views, s, X, P)
    gap_r = float(np.abs(res - cx.f64(sx.residuals(views, s, X, P))).max())
    gap = float((np.abs(J - Jfd).max(0) / np.abs(Jfd).max(0)).max())
    print(f"{s.tag}: residuals within {gap_r:.2e} px, Jacobian columns within {gap:.2e} of their largest entry")
    assert gap_r <= 1e-10 and gap <= 1e-10


# ------------------------------------------------------------------------------------------------ truth

@pytest.mark.parametrize("rig,c0,c1,board", TRUTH_CASES)
def test_truth_recovery_noise_free_float32(rig, c0, c1, board):
    s = sx.scene(1, 6, rig, board, c0, c1)
    r = _solve(s)
    eR, eT = sx.rig_error(r, s)
    eP = max(cx.rot_gap(a, b) for a, b in zip(r.rvecs, s.P[:, :3]))
    print(f"{s.tag}: |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, board rotations {eP:.2e}, rms {r.rms:.2e} px, steps "
          f"{r.iterations} / {r.attempts}")
    assert r.status == stereo.STEREO_OK and (r.view_status == pnp.PNP_OK).all() and r.pairs_used == 6
    assert r.points_used == sum(len(k) for k in s.kps0 + s.kps1) == int(r.view_points.sum())
    assert eR <= TRUTH_R and eT <= TRUTH_T and r.rms <= TRUTH_RMS


@pytest.mark.parametrize("rig,c0,c1", [("small", "A", "B"), ("toe90", "B", "C"), ("r170", "C", "A")])
def test_noisy_scene_ends_at_a_stationary_point_no_higher_than_the_truth(rig, c0, c1):
    """sigma = 0.3 px: the cost at the result is no higher than at the truth, and |J^T r| <= 1e-6 |J| |r| with the exact model's
    finite-difference Jacobian (DESIGN 3.8's gate)."""
    s = sx.scene(2, 5, rig, sx.BOARD_S, c0, c1, sigma=0.3)
    r = _solve(s)
    assert r.status == stereo.STEREO_OK and r.pairs_used == 5
    views = sx.pool_views(s)
    X, P = _xp(r)
    c_res, grad = sx.stationarity(views, s, X, P)
    c_true = sx.cost(views, s, s.X, s.P)
    print(f"{s.tag}: cost {c_res:.6f} (truth {c_true:.6f}), |Jtr| / (|J||r|) {grad:.2e}, rms {r.rms:.4f} px, rig error "
          f"{sx.rig_error(r, s)}")
    assert c_res <= c_true and grad <= 1e-6
    assert abs(r.rms - math.sqrt(c_res / r.points_used)) <= 1e-9 * r.rms


def test_views_without_a_common_id_recover_the_rig():
    s = sx.scene(3, 6, "toe90", sx.BOARD_S, "A", "B", disjoint=True)
    for a, b in zip(s.kps0, s.kps1):
        assert not set(a[:, 2].tolist()) & set(b[:, 2].tolist())
    r = _solve(s)
    eR, eT = sx.rig_error(r, s)
    print(f"disjoint ids: |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}, rms {r.rms:.2e}")
    assert r.status == stereo.STEREO_OK and r.pairs_used == 6
    assert eR <= TRUTH_R and eT <= TRUTH_T


# ------------------------------------------------------------------------------------------------ bookkeeping

def _bookkeeping_scene():
    """8 timestamps: 0 fine, 1 camera 0 with 3 rows, 2 camera 1 with an id outside the board, 3 a 4-row view of camera 1, 4 seen by
    camera 0 only, 5 - 7 fine."""
    s = sx.scene(4, 8, "small", sx.BOARD_S, "A", "B", rows=[(12, 9)] * 3 + [(12, 4)] + [(12, 9)] * 4)
    kps0, kps1 = [k.copy() for k in s.kps0], [k.copy() for k in s.kps1]
    kps0[1] = kps0[1][:3]
    kps1[2][5, 2] = cx.n_ids(s.board)
    kps1[4] = np.zeros((0, 3))
    expect = np.zeros((8, 2), np.int32)
    expect[1, 0], expect[2, 1], expect[4, 1] = pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_TOO_FEW
    return s._replace(kps0=kps0, kps1=kps1), expect


def test_bookkeeping_of_unusable_views():
    s, expect = _bookkeeping_scene()
    r = _solve(s)
    assert r.view_status.tolist() == expect.tolist()
    used = [0, 3, 5, 6, 7]
    assert r.status == stereo.STEREO_OK and r.pairs_used == 5
    assert r.view_points.tolist() == [[len(a), len(b)] for a, b in zip(s.kps0, s.kps1)]
    assert r.pair_points.tolist() == [len(s.kps0[t]) + len(s.kps1[t]) if t in used else 0 for t in range(8)]
    assert r.points_used == int(r.pair_points.sum()) and r.view_points[3, 1] == 4
    out = [t for t in range(8) if t not in used]
    assert not r.rvecs[out].any() and not r.tvecs[out].any() and not r.pair_rms[out].any() and not r.view_rms[out].any()
    assert (r.pair_rms[used] > 0).all() and (r.view_rms[used] > 0).all()
    eR, eT = sx.rig_error(r, s)
    print(f"bookkeeping: 5 of 8 pairs, |R - R_true| {eR:.2e}, |T - T_true| / |T| {eT:.2e}")
    assert eR <= TRUTH_R and eT <= TRUTH_T
    # the same pairs alone give the same bits: a timestamp left out leaves no trace
    alone = stereo.stereo_calibrate_host_full([s.kps0[t] for t in used], [s.kps1[t] for t in used], *s.board, *sx.cam_args(s))
    assert np.array_equal(alone.R, r.R) and np.array_equal(alone.T, r.T) and alone.rms == r.rms
    with pytest.raises(IndexError):
        stereo.stereo_calibrate_host(s.kps0, s.kps1, *s.board, *sx.cam_args(s))
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_host(s.kps0[:2], s.kps1[:2], *s.board, *sx.cam_args(s))
    ok = stereo.stereo_calibrate_host([s.kps0[t] for t in used], [s.kps1[t] for t in used], *s.board, *sx.cam_args(s))
    assert len(ok) == 9 and ok[0] == r.rms and ok[6].shape == (3, 1) and np.array_equal(ok[5], r.R)


def test_nothing_pairs():
    s, _ = _bookkeeping_scene()
    kps0 = [s.kps0[0][:3], s.kps0[1], np.zeros((0, 3))]
    kps1 = [s.kps1[0], np.zeros((0, 3)), s.kps1[3]]
    r = stereo.stereo_calibrate_host_full(kps0, kps1, *s.board, *sx.cam_args(s))
    assert r.status == stereo.STEREO_NO_PAIRS and r.pairs_used == 0 and r.points_used == 0 and r.rms == 0.0
    assert r.view_status.tolist() == [[pnp.PNP_TOO_FEW, pnp.PNP_OK], [pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW], [pnp.PNP_TOO_FEW, pnp.PNP_OK]]
    assert not r.R.any() and not r.T.any() and not r.F.any() and not r.rvecs.any() and not r.pair_points.any()
    assert r.view_points.tolist() == [[3, len(s.kps1[0])], [3, 0], [0, 4]]


@pytest.mark.parametrize("n", [4, 5])
def test_rig_init_takes_the_lower_median(n):
    """Pairs whose relative translations differ: the init's T is element (n - 1) // 2 of the sorted values in every coordinate, on
    an even and on an odd number of pairs, never the mean of two."""
    assert stereo.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0 and stereo.lower_median([5.0, 1.0, 3.0]) == 3.0
    assert stereo.lower_median([7.0]) == 7.0 and stereo.lower_median([2.0, 1.0]) == 1.0
    rng = np.random.default_rng(n)
    rx = np.array([0.1, -0.7, 0.2])
    RX = pnp._rodrigues(rx)
    Tt = rng.normal(size=(n, 3))
    p0 = np.c_[rng.normal(scale=0.3, size=(n, 3)), rng.normal(size=(n, 3))]
    p1 = np.array([np.r_[pnp._rvec_of(RX @ pnp._rodrigues(p[:3])), RX @ p[3:] + T] for p, T in zip(p0, Tt)])
    st, X0, _ = stereo._rig_init(p0, p1)
    want = np.sort(Tt, 0)[(n - 1) // 2]
    print(f"{n} pairs: init T {X0[3:]}, lower medians {want}")
    assert st == stereo.STEREO_OK
    assert np.abs(X0[3:] - want).max() <= 1e-14 and np.abs(X0[:3] - rx).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ epipolar

# the largest distance (px) of an exact image point of camera 1 from the epipolar line F x0 of its partner, measured by
# test_epipolar_constraint_on_noise_free_points on the CPU: 3.94e-6 px; gated x 4 like the truth recovery it follows from
EPI_PX = 4 * 3.94e-6


def test_epipolar_constraint_on_noise_free_points():
    """Exact, undistorted pixel coordinates of the same board points in both cameras: the distance of x1 from the line F x0
    (|x1^T F x0| over the norm of the line's first two coefficients) and of x0 from F^T x1, in pixels, at the scale the
    recovered rig's error gives it.  For scale: F transposed, K0 / K1 exchanged or R [T]x in place of [T]x R are tens of pixels
    off on this scene."""
    s = sx.scene(1, 6, "toe90", sx.BOARD_S, "A", "B")
    r = _solve(s)
    (K0, _), (K1, _) = sx.cam(s.cam0), sx.cam(s.cam1)
    obj = cx.board_points(np.arange(cx.n_ids(s.board)), *s.board)

    def worst(F):
        w = 0.0
        for P in s.P:
            x0 = np.c_[cx.f64(sx.project_rig(obj, P, None, K0, None)), np.ones(len(obj))]
            x1 = np.c_[cx.f64(sx.project_rig(obj, P, s.X, K1, None)), np.ones(len(obj))]
            e = np.abs(np.einsum("ni,ij,nj->n", x1, F, x0))
            l1, l0 = x0 @ F.T, x1 @ F
            w = max(w, float((e / np.linalg.norm(l1[:, :2], axis=1)).max()), float((e / np.linalg.norm(l0[:, :2], axis=1)).max()))
        return w
    got = worst(r.F)
    wrong = {"F^T": worst(r.F.T), "K swapped": worst(stereo.essential_fundamental(r.R, r.T, K1, K0)[1]),
             "R [T]x": worst(np.linalg.inv(K1).T @ (r.R @ pnp._skew(r.T)) @ np.linalg.inv(K0))}
    print(f"epipolar: worst point-to-line distance {got:.3e} px (gate {EPI_PX:.1e}); wrong constructions {wrong}")
    assert r.F[2, 2] == 1.0 and np.array_equal(r.E, pnp._skew(r.T) @ r.R)
    assert got <= EPI_PX
    assert min(wrong.values()) >= 1.0                       # (the gate separates them by many orders)


# ------------------------------------------------------------------------------------------------ masks

RANSAC = dict(iterations=100, reproj_error=3.0, min_inliers=6, seed=7)
# The unmasked solve on the planted scene, measured by test_masks_from_the_consensus_solver: status OK, rms 35.0 px against the
# masked 0.394 px (factor 88.9), the rig's rotation off by 0.909 (max |R - R_true|).  Both are asserted at HALF the measured
# value, not at x 1 / 4 like an error bound: the unmasked result is where LM stops on a cost with 20 % wrong rows, a point that
# moves with the libm and the summation order by far more than rounding, while half of either figure is still 44 x the masked
# rms and 1,000 x the masked rotation error.
PLANTED_RMS_FACTOR, PLANTED_ROT_ERROR = 88.9 / 2, 0.909 / 2


def planted_scene():
    """sigma = 0.3 px, 6 pairs, 20 rows per view; in every view two pairs of rows exchange their ids (at least two grid steps
    apart: ~25 px against the 3 px threshold) -> (scene, good-row masks per camera)."""
    s = sx.scene(5, 6, "toe90", sx.BOARD_S, "A", "B", sigma=0.3, rows=20)
    rng = np.random.default_rng(77)
    good = ([], [])
    for c, kps in enumerate((s.kps0, s.kps1)):
        for t in range(len(kps)):
            kp, g = kps[t], np.ones(20, bool)
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
    masks = ([], [])
    for c, (kps, (K, d)) in enumerate(zip((s.kps0, s.kps1), (sx.cam(s.cam0), sx.cam(s.cam1)))):
        for kp in kps:
            ret, _, _, m = pnp.solve_pnp_ransac_host(kp, *s.board, K, d, **RANSAC)
            assert ret
            masks[c].append(m)
    assert all(np.array_equal(m, g) for c in range(2) for m, g in zip(masks[c], good[c]))
    masked = _solve(s, masks=masks)
    true_rows = stereo.stereo_calibrate_host_full([k[g] for k, g in zip(s.kps0, good[0])], [k[g] for k, g in zip(s.kps1, good[1])],
                                                  *s.board, *sx.cam_args(s))
    for a, b in zip(masked, true_rows):
        assert np.array_equal(a, b)
    plain = _solve(s)
    print(f"planted: masked rms {masked.rms:.3f} px, rig error {sx.rig_error(masked, s)}; unmasked rms {plain.rms:.3f} px (status "
          f"{plain.status}), rig error {sx.rig_error(plain, s)}; factor {plain.rms / masked.rms:.1f}")
    assert masked.status == stereo.STEREO_OK and (masked.view_points == 16).all() and masked.points_used == 6 * 32
    assert plain.status == stereo.STEREO_OK and plain.rms >= PLANTED_RMS_FACTOR * masked.rms
    assert sx.rig_error(plain, s)[0] >= PLANTED_ROT_ERROR and sx.rig_error(masked, s)[0] <= 1e-2
    ones = _solve(s, masks=([np.ones(20, bool)] * 6, None))
    for a, b in zip(ones, plain):
        assert np.array_equal(a, b)
    short = [m.copy() for m in masks[1]]
    short[2][:] = False
    short[2][:3] = True
    r = _solve(s, masks=(masks[0], short))
    assert r.view_status[2].tolist() == [pnp.PNP_OK, pnp.PNP_TOO_FEW] and r.pairs_used == 5 and r.view_points[2, 1] == 3


def test_a_failed_solve_still_counts_its_pairs():
    """Every status but OK zeroes the continuous outputs and the per-pair rows; the pairs found and their rows are reported
    (what the kernels write on their failure paths)."""
    vs = np.array([[0, 0], [0, 1], [0, 0]], np.int32)
    vp = np.array([[9, 7], [9, 3], [5, 6]], np.int64)
    for status in (stereo.STEREO_DEGENERATE, stereo.STEREO_NONFINITE):
        r = stereo._result(status, None, sx.K_A, sx.K_B, vs, vp, np.array([0, 2]), None, None, 3, 25)
        assert (r.status, r.pairs_used, r.points_used, r.iterations, r.attempts, r.rms) == (status, 2, 27, 3, 25, 0.0)
        assert not r.pair_points.any() and not r.R.any() and not r.rvecs.any() and r.view_points.tolist() == vp.tolist()


def test_argument_errors():
    s = sx.scene(1, 2, "small", sx.BOARD_S, "A", "B")
    skew = sx.K_A.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, skew, None, sx.K_B, None)
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, sx.K_A, None, sx.K_B, np.zeros(12))
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_host_full(s.kps0, s.kps1[:1], *s.board, *sx.cam_args(s))
    with pytest.raises(ValueError):
        _solve(s, masks=([np.ones(3, bool), None], None))
