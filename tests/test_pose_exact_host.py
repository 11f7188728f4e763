"""The host definitions of the pose and calibration solvers (deepcharuco_amd/pnp.py, calib.py) against an exact restatement of the
camera model (tests/camera_exact.py) on the inputs the other tests leave out: non-square boards, fx != fy, every distortion
model, boards that face the camera or stand upside down in the image plane, and 4 / 5 / 63 / 64 / 65 / 129 rows.  No GPU needed.

The frames are made by camera_exact.project (extended precision, its own rotation, no code of pnp.py), so a deviation of
pnp._project from the documented camera model shows here even though host and device agree with each other;
tests/test_gpu_pose_edges.py runs the same grid on the device.  Where cv2 is absent this is the stand-in for
test_pnp_host.test_matches_cv2_where_available."""
import collections
import functools
import math
import os

import numpy as np

import camera_exact as A
from conftest import GOLDEN
from deepcharuco_amd import calib, pnp

# Accepted LM steps on noise-free frames.  Levenberg-Marquardt heals a wrong start, so the initialisation (homography
# decomposition, matrix -> vector conversion, undistortion) shows in the step count only.  Measured on the CPU over the 300
# noise-free frames of the grid: 4- and 5-row frames 1 x15, 2 x108, 3 x37; frames of 36 rows and more 1 x72, 2 x68.
STEPS_MAX = 3
BRANCH = 1e-5                      # the sine at which cvRodrigues2's (and pnp._rvec_of's) matrix -> vector conversion switches arms


@functools.lru_cache(maxsize=None)
def _host_run():
    """solve_pnp_host_full on every frame of the grid, with the matrix each solve hands to pnp._rvec_of recorded on the way."""
    seen, orig = [], pnp._rvec_of

    def spy(Q):
        seen.append(Q.copy())
        return orig(Q)
    pnp._rvec_of = spy
    try:
        res = [pnp.solve_pnp_host_full(f.kp, *f.board, A.K_EDGE, A.MODELS[f.model]) for f in A.grid()]
    finally:
        pnp._rvec_of = orig
    assert len(seen) == len(res)                     # one conversion per solve: the planar initialisation's
    return res, seen


def host_results():
    """-> list of (status, pose[8]), one per frame of the grid."""
    return _host_run()[0]


def branch_margin():
    """-> per-frame (s, c), the sine and cosine of the rotation angle of the orthonormalised matrix the planar initialisation
    converts to a vector; asserts that no frame of the grid stands within a factor 10 of the switch at s = 1e-5."""
    out = []
    for f, Q in zip(A.grid(), _host_run()[1]):
        s = math.sqrt(((Q[2, 1] - Q[1, 2]) ** 2 + (Q[0, 2] - Q[2, 0]) ** 2 + (Q[1, 0] - Q[0, 1]) ** 2) * 0.25)
        c = (np.trace(Q) - 1) * 0.5
        assert s < BRANCH / 10 or s > BRANCH * 10, (f.tag, s, c)
        out.append((s, c))
    return out


def check_recovery(f, pose):
    """Noise-free frame: the rotation matrix and tvec recover the truth to the project's own numbers (1e-4 for >= 6 rows,
    test_pnp_host.test_recovery_noise_free; 1e-3 for 4 and 5, test_point_counts_and_distortion_models).  -> the two gaps."""
    tol = 1e-4 if f.n >= 6 else 1e-3
    gr, gt = A.rot_gap(pose[:3], f.r), float(np.linalg.norm(pose[3:6] - f.t) / np.linalg.norm(f.t))
    assert gr <= tol and gt <= tol, (f.tag, gr, gt)
    return gr, gt


def check_optimality(f, pose):
    """Noisy frame that stopped by the rule: test_pnp_host.test_optimality_with_noise's two numbers with camera_exact's
    residuals and finite-difference Jacobian.  -> the stationarity measure."""
    obj, img, _ = A.pool_rows(f)
    dist = A.MODELS[f.model]
    cost, grad = A.stationarity(obj, img, pose[:6], A.K_EDGE, dist)
    cost_true = A.cost(obj, img, np.r_[f.r, f.t], A.K_EDGE, dist)
    assert cost <= cost_true * (1 + 1e-9), (f.tag, cost, cost_true)
    assert grad <= 1e-6, (f.tag, grad)
    assert abs(pose[6] - math.sqrt(cost / f.n)) <= 1e-9 * max(pose[6], 1e-6), (f.tag, pose[6], cost)
    return grad


# ------------------------------------------------------------------------------------------------ the restatement itself

def test_extended_precision_model_matches_mpmath():
    """camera_exact.project (long double arrays, closed-form rotation) against project_mp (40 digits, mpmath.expm) on a point
    of one frame of every view class: 1e-17 relative to the larger of the coordinate and the focal length."""
    import mpmath
    assert A.HAVE_LD, "no 64-bit-mantissa long double here: camera_exact runs on mpmath objects (slow)"
    worst = 0.0
    for view in A.VIEWS:
        f = next(f for f in A.grid() if f.view == view and f.model == "8" and f.n > 5 and f.sigma == 0)
        obj = A.board_points(f.kp[:3, 2], *f.board)
        p = np.r_[f.r, f.t]
        got = A.project(obj, p, A.K_EDGE, A.DIST8)
        for i in range(3):
            want = A.project_mp(obj[i], p, A.K_EDGE, A.DIST8)
            for c in range(2):
                with mpmath.workdps(40):
                    rel = float(abs(A.to_mp(got[i, c]) - want[c]) / max(abs(want[c]), 310))
                worst = max(worst, rel)
    print("long double vs 40-digit mpmath, worst relative gap %.3g" % worst)
    assert worst <= 1e-17
    # rotations: orthonormal to the working precision at 0, 1e-7, 1 and pi - 1e-8 rad; exp(0) = I exactly
    assert np.array_equal(A.f64(A.rotation(np.zeros(3))), np.eye(3))
    for th in (1e-7, 1.0, np.pi - 1e-8):
        R = A.rotation(np.array([0.1, 0.25, 0.96]) / np.linalg.norm([0.1, 0.25, 0.96]) * th)
        assert float(np.abs(R @ R.T - np.eye(3)).max()) <= 1e-18


def test_board_points_equal_the_reference_construction():
    """camera_exact's id -> board point rule against outputs of the reference's own construction (the committed fixture holds
    (4, 7) and (7, 4) boards besides square ones), and pnp.object_points against it on the grid's boards."""
    fx = np.load(os.path.join(GOLDEN, "solve_pnp_points.npz"))
    shapes = set()
    for i in range(int(fx["n_cases"])):
        kp, (cc, rc, sq) = fx[f"kp{i}"], fx[f"board{i}"]
        got = A.board_points(kp[:, 2], int(cc), int(rc), float(sq))
        assert got.dtype == np.float32 and np.array_equal(got, fx[f"objp{i}"])
        shapes.add((int(cc), int(rc)))
    assert any(c < r for c, r in shapes) and any(c > r for c, r in shapes)
    for board in A.BOARDS:
        ids = np.arange(A.n_ids(board))
        assert np.array_equal(pnp.object_points(ids, *board).view(np.uint32), A.board_points(ids, *board).view(np.uint32))
    a, b = A.board_points(np.arange(40), 9, 6, 0.02), A.board_points(np.arange(40), 6, 9, 0.02)
    assert not np.array_equal(a, b) and a[:, 0].max() < a[:, 1].max() and b[:, 0].max() > b[:, 1].max()


def test_grid_covers_what_it_says():
    G = A.grid()
    assert len(G) == 600 and len({f.tag for f in G}) == 600
    assert {f.board for f in G} == set(A.BOARDS) and all(b[0] != b[1] for b in A.BOARDS) and max(map(A.n_ids, A.BOARDS)) > 300
    assert abs(A.K_EDGE[0, 0] / A.K_EDGE[1, 1] - 1) >= 0.05
    for board in A.BOARDS:
        for model in A.MODELS:
            sub = [f for f in G if f.board == board and f.model == model]
            assert {f.view for f in sub} == set(A.VIEWS) and {f.sigma for f in sub} == set(A.SIGMAS)
            assert {f.n for f in sub} == {min(n, A.n_ids(board)) for n in A.ROWS}
    assert {f.n for f in G if f.board == A.BOARDS[3]} == set(A.ROWS)
    for f in G:
        assert len(set(f.kp[:, 2])) == f.n and (f.n > 5 or A.general_position(f.kp[:, 2], f.board))
        if f.n > 5:
            assert not np.array_equal(f.kp[:, 2], np.sort(f.kp[:, 2]))                  # scrambled row order
        assert np.array_equal(f.kp[:, :2], f.kp[:, :2].astype(np.float32))
    assert all(np.abs(f.kp[:, :2] - A.K_EDGE[:2, 2]).max() <= 160 for f in G)           # roughly +-100 px
    assert max(np.abs(f.kp[:, :2] - A.K_EDGE[:2, 2]).max() for f in G) >= 90
    # the views rolled by 180 degrees: every sign pattern of the axis' x and y components, and the optical axis itself
    signs = {(int(np.sign(f.r[0])), int(np.sign(f.r[1]))) for f in G if f.view == "pi"}
    assert signs == {(0, 0), (1, 1), (1, -1), (-1, -1), (-1, 1)}
    assert all(np.pi - 1e-7 <= np.linalg.norm(f.r) <= np.pi for f in G if f.view == "pi")
    assert all(not f.r.any() for f in G if f.view == "fronto")


# ------------------------------------------------------------------------------------------------ the pose solver

def test_every_frame_is_solved_and_few_run_into_the_step_cap():
    res = host_results()
    for f, (st, pose) in zip(A.grid(), res):
        assert st == pnp.PNP_OK, (f.tag, st)
    cap = [f.tag for f, (_, pose) in zip(A.grid(), res) if pose[7] >= pnp.LM_MAX_ITER]
    print(f"{len(cap)} of {len(res)} frames ran into the {pnp.LM_MAX_ITER}-step cap:", cap)
    assert len(cap) <= 0.05 * len(res)


def test_branch_selection_is_no_coin_toss():
    sc = branch_margin()
    tally = collections.Counter()
    for f, (s, c) in zip(A.grid(), sc):
        tally[(f.view, "ordinary" if s > BRANCH else "zero" if c > 0 else "pi")] += 1
    print("arm of the matrix -> vector conversion per view class:", sorted(tally.items()))
    for view, arm in (("fronto", "zero"), ("tiny", "zero"), ("pi", "pi"), ("tilt", "ordinary"), ("near_pi", "ordinary")):
        assert tally[(view, arm)] >= 40, (view, arm, tally)                        # every arm decides many frames
    assert tally[("pi", "zero")] == 0 and tally[("fronto", "pi")] == 0


def test_noise_free_frames_recover_the_truth_in_few_steps():
    worst, steps = collections.defaultdict(float), collections.defaultdict(collections.Counter)
    for f, (st, pose) in zip(A.grid(), host_results()):
        if f.sigma:
            continue
        gr, gt = check_recovery(f, pose)
        worst[f.n >= 6] = max(worst[f.n >= 6], gr, gt)
        steps[f.n >= 6][int(pose[7])] += 1
        assert pose[7] <= STEPS_MAX, (f.tag, pose[7])
    print("worst recovery gap: >= 6 rows %.3g, 4 and 5 rows %.3g; accepted steps: >= 6 rows %s, 4 and 5 rows %s" % (
        worst[True], worst[False], sorted(steps[True].items()), sorted(steps[False].items())))


def test_noisy_frames_end_in_a_least_squares_minimum_of_the_exact_model():
    worst = collections.defaultdict(float)
    n = 0
    for f, (st, pose) in zip(A.grid(), host_results()):
        if f.sigma and pose[7] < pnp.LM_MAX_ITER:
            worst[f.n] = max(worst[f.n], check_optimality(f, pose))
            n += 1
    print(f"{n} noisy frames stopped by the rule; worst |J^T r| / (|J| |r|) by row count:",
          {k: float("%.3g" % v) for k, v in sorted(worst.items())})
    assert n >= 250


def test_project_matches_the_exact_model_and_its_finite_differences():
    """pnp._project's residuals (1e-9 px) and analytic Jacobian (1e-6 of each column's largest entry) on a noisy frame of
    every distortion model x view class, at the true pose: r = 0 exactly for the fronto-parallel frames, |r| ~ 1e-7 for the
    tiny ones (the right Jacobian's series arm), |r| within 1e-7 of pi."""
    worst_r, worst_j = 0.0, 0.0
    for model, dist in A.MODELS.items():
        for view in A.VIEWS:
            for f in [f for f in A.grid() if f.model == model and f.view == view and f.sigma and f.n > 5][:2]:
                obj, img, _ = A.pool_rows(f)
                p = np.r_[f.r, f.t]
                res, cost, J = pnp._project(obj.astype(np.float64), img, p, pnp._camera(A.K_EDGE), pnp._dist(dist), True)
                want = A.f64(A.residuals(obj, img, p, A.K_EDGE, dist))
                Jw = A.jacobian_fd(obj, img, p, A.K_EDGE, dist)
                worst_r = max(worst_r, float(np.abs(res - want).max()))
                assert np.abs(res - want).max() <= 1e-9, (f.tag, np.abs(res - want).max())
                assert abs(cost - float((want * want).sum())) <= 1e-9 * cost
                for j in range(6):
                    gap = float(np.abs(J[:, j] - Jw[:, j]).max() / np.abs(Jw[:, j]).max())
                    worst_j = max(worst_j, gap)
                    assert gap <= 1e-6, (f.tag, j, gap)
    print("pnp._project vs the exact model: residuals %.3g px, Jacobian columns %.3g relative" % (worst_r, worst_j))


def test_undistort_inverts_the_exact_distortion():
    """pnp._undistort, then camera_exact's distortion, returns the pixel.  Five fixed-point rounds leave an error of their
    own: it is measured on camera_exact alone (its own five-round inverse in extended precision), and the host gets twice
    that."""
    gx, gy = np.meshgrid(np.linspace(-100, 100, 9), np.linspace(-100, 100, 9))
    pix = np.c_[gx.ravel() + A.K_EDGE[0, 2], gy.ravel() + A.K_EDGE[1, 2]]
    for model, dist in A.MODELS.items():
        own = A.undistort5(pix, A.K_EDGE, dist)
        floor = float(np.abs(A.f64(A.distort(own[:, 0], own[:, 1], A.K_EDGE, A.dist8(dist))) - pix).max())
        xy = A._w(pnp._undistort(pix, pnp._camera(A.K_EDGE), pnp._dist(dist)))
        gap = float(np.abs(A.f64(A.distort(xy[:, 0], xy[:, 1], A.K_EDGE, A.dist8(dist))) - pix).max())
        print(f"undistort round trip at +-100 px, dist {model}: exact five rounds {floor:.3g} px, host {gap:.3g} px")
        assert gap <= 2 * floor + 1e-12, (model, gap, floor)          # 1e-12 px: float64 rounding of a 250 px coordinate
        assert floor <= 1e-3
    # converged, the exact inverse is an inverse
    own = A.undistort5(pix, A.K_EDGE, A.DIST8, rounds=60)
    assert float(np.abs(A.f64(A.distort(own[:, 0], own[:, 1], A.K_EDGE, A.DIST8)) - pix).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ RANSAC

def ransac_args(**kw):
    return dict(dict(iterations=100, reproj_error=A.RANSAC_REPROJ, min_inliers=4, seed=A.RANSAC_SEED), **kw)


def test_ransac_finds_planted_wrong_ids_on_every_board_and_model():
    worst = np.inf
    for f, good in A.planted_frames():
        dist = A.MODELS[f.model]
        st, pose, mask, winner, margin = pnp.solve_pnp_ransac_host_full(f.kp, *f.board, A.K_EDGE, dist, with_margin=True,
                                                                        **ransac_args())
        assert st == pnp.PNP_OK and np.array_equal(mask, good), (f.tag, st, mask.sum(), good.sum())
        assert margin >= 1e-6, (f.tag, margin)
        worst = min(worst, margin)
        kept = f.kp[good]
        st_good, pose_good = pnp.solve_pnp_host_full(kept[np.argsort(kept[:, 2], kind="stable")], *f.board, A.K_EDGE, dist)
        assert st_good == pnp.PNP_OK and np.array_equal(pose, pose_good), f.tag
        assert A.rot_gap(pose[:3], f.r) <= 0.02 and np.linalg.norm(pose[3:6] - f.t) <= 0.02 * np.linalg.norm(f.t), f.tag
    print("smallest margin %.3g over %d planted frames" % (worst, len(A.planted_frames())))


def test_ransac_keeps_clean_frames_of_four_and_five_rows():
    """A noise-free frame of exactly 4 rows has one sample; with min_inliers = 4 it is the consensus, and the refit is the plain
    solve.  With sigma = 0.3 px a hypothesis (the pose decomposed from the exact homography of its four rows, no LM) need not
    reproject all of its own rows within 3 px, so such a frame may end without consensus: that is the definition
    (solve_pnp_ransac_host_full), and what is asserted is that a consensus, where there is one, is refitted like the plain solve."""
    n, none = 0, []
    for f in A.grid():
        if f.n <= 5 and f.model in ("none", "8") and f.board in A.BOARDS[1:3]:
            dist = A.MODELS[f.model]
            st, pose, mask, winner = pnp.solve_pnp_ransac_host_full(f.kp, *f.board, A.K_EDGE, dist, **ransac_args())
            n += 1
            if f.sigma and st == pnp.PNP_NO_CONSENSUS:
                none.append(f.tag)
                continue
            assert st == pnp.PNP_OK and winner >= 0 and mask.sum() >= 4 and (f.sigma or mask.all()), (f.tag, st, mask, winner)
            kept = f.kp[mask]
            hs, hp = pnp.solve_pnp_host_full(kept[np.argsort(kept[:, 2], kind="stable")], *f.board, A.K_EDGE, dist)   # pool order
            assert hs == pnp.PNP_OK and np.array_equal(pose, hp), f.tag
    print(f"{len(none)} of {n // 2} noisy frames without consensus at {A.RANSAC_REPROJ} px:", none)
    assert n == 80


# ------------------------------------------------------------------------------------------------ calibration

def check_calibration_recovers(r, poses, tol=1e-5):
    """test_calib_host.test_truth_recovery_float32's tolerances; poses compared as rotation matrices."""
    assert r.status == calib.CALIB_OK and (r.view_status == pnp.PNP_OK).all() and r.views_used == len(poses)
    gk = float(np.abs(r.camera_matrix - A.CALIB_K).max() / A.CALIB_K[0, 0])
    gd = float(np.abs(r.dist_coeffs.ravel() - A.CALIB_DIST).max())
    gr = max(A.rot_gap(r.rvecs[i], poses[i, :3]) for i in range(len(poses)))
    gt = max(float(np.linalg.norm(r.tvecs[i] - poses[i, 3:]) / np.linalg.norm(poses[i, 3:])) for i in range(len(poses)))
    print("calibration vs the truth: K %.3g relative, distortion %.3g, rotation matrices %.3g, tvec %.3g relative; rms %.3g px" % (
        gk, gd, gr, gt, r.rms))
    assert gk <= tol and gd <= tol and gr <= tol and gt <= tol and r.rms <= 2e-5
    return gk, gd, gr, gt


def test_calibration_recovers_the_truth_from_exact_views():
    """32 noise-free float32 views of a 7 x 11 board in a 400 x 240 image made by the exact model; every fourth one
    fronto-parallel or rolled by 180 degrees."""
    objs, imgs, _, poses = A.calib_views(11, 32)
    assert sum(1 for p in poses if not p[:3].any()) == 4 and sum(1 for p in poses if abs(np.linalg.norm(p[:3]) - np.pi) < 1e-6) == 4
    check_calibration_recovers(calib.calibrate_camera_host_full(objs, imgs, A.CALIB_SIZE), poses)
