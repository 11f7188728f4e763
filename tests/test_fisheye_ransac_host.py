"""The host definition of the consensus pose on a fisheye camera (deepcharuco_amd/fisheye.py, solve_pnp_fisheye_ransac_host_full:
pnp.solve_pnp_ransac_host_full's search run through the fisheye model) on the exact views of tests/fisheye_exact.py: clean views,
views with three of their 28 ids exchanged, a sample with a pixel outside the model, the statuses, and its masks in front of a
rig with fisheye cameras in it.  No GPU.  The gates are test_pnp_ransac_host's: the pose is the plain fisheye solve on the kept
rows, bit for bit (the same function on the same rows)."""
import numpy as np
import pytest

import camera_exact as cx
import fisheye_exact as fx
import fisheye_rig_exact as frx
import rig_exact as rx
import stereo_exact as sx
from deepcharuco_amd import fisheye, pnp, rig
from test_fisheye_rig_host import class_scene, solve
from test_stereo_host import RANSAC

K, KD = fx.camera(230.0, off=(3.0, -2.0)), fx.K_LENS
REPROJ, SEED = 3.0, 7
ARGS = dict(iterations=100, reproj_error=REPROJ, min_inliers=4, seed=SEED)


def swapped_views(n_views=6, sigma=0.3, seed=5):
    """Views of all 28 corners with the ids of three rows exchanged in a cycle (each at least two grid steps from the next:
    ~50 px against a 3 px threshold) -> list of (keypoints, good-row mask, true pose)."""
    _, imgs, ids_l, poses = fx.make_views(seed, n_views, K, KD, sigma=sigma)
    rng = np.random.default_rng(seed)
    out = []
    for kp, p in zip(fx.keypoints(imgs, ids_l), poses):
        grid = cx.grid_xy(kp[:, 2], fx.BOARD[1])
        while True:
            a, b, c = rng.choice(len(kp), 3, replace=False)
            if min(np.abs(grid[a] - grid[b]).max(), np.abs(grid[b] - grid[c]).max(), np.abs(grid[c] - grid[a]).max()) >= 2:
                break
        kp = kp.copy()
        kp[[a, b, c], 2] = kp[[b, c, a], 2]
        good = np.ones(len(kp), bool)
        good[[a, b, c]] = False
        out.append((kp, good, p))
    return out


def _ransac(kp, **kw):
    return fisheye.solve_pnp_fisheye_ransac_host_full(kp, *fx.BOARD, K, KD, **{**ARGS, **kw})


def test_clean_views_keep_every_row_and_the_plain_pose():
    _, imgs, ids_l, _ = fx.make_views(3, 6, K, KD, sigma=0.0)
    rng = np.random.default_rng(3)
    for i, kp in enumerate(fx.keypoints(imgs, ids_l)):
        kp = kp[rng.permutation(len(kp))]                                 # the caller's row order: not id-sorted
        st, pose, mask, winner = _ransac(kp, reproj_error=8.0)
        assert st == pnp.PNP_OK and mask.all() and mask.shape == (28,) and winner >= 0
        st0, pose0 = fisheye.solve_pnp_fisheye_host_full(kp[np.argsort(kp[:, 2], kind="stable")], *fx.BOARD, K, KD)
        assert st0 == pnp.PNP_OK and np.array_equal(pose, pose0)
        ret, rvec, tvec, inl = fisheye.solve_pnp_fisheye_ransac_host(kp, *fx.BOARD, K, KD, seed=SEED)
        assert ret is True and rvec.shape == (3, 1) and np.array_equal(np.r_[rvec.ravel(), tvec.ravel()], pose[:6]) and inl.all()


def test_three_exchanged_ids_are_found_and_the_pose_is_recovered():
    worst = np.inf
    for i, (kp, good, truth) in enumerate(swapped_views()):
        st, pose, mask, winner, margin = _ransac(kp, with_margin=True)
        assert st == pnp.PNP_OK and np.array_equal(mask, good) and int(mask.sum()) == 25, (i, st, mask)
        st_good, pose_good = fisheye.solve_pnp_fisheye_host_full(kp[good], *fx.BOARD, K, KD)
        assert st_good == pnp.PNP_OK and np.array_equal(pose, pose_good)             # the same function on the same rows
        assert 0 <= winner < 100 and margin >= 1e-6, (i, winner, margin)
        worst = min(worst, margin)
        terr = np.linalg.norm(pose[3:6] - truth[3:]) / np.linalg.norm(truth[3:])
        st_plain, pose_plain = fisheye.solve_pnp_fisheye_host_full(kp, *fx.BOARD, K, KD)
        terr_plain = np.linalg.norm(pose_plain[3:6] - truth[3:]) / np.linalg.norm(truth[3:]) if st_plain == pnp.PNP_OK else np.inf
        print(f"view {i}: translation error {terr:.2e} with consensus, {terr_plain:.2e} without; winner {winner}, margin {margin:.3g}")
        assert terr_plain > terr                                          # test_pnp_ransac_host's condition: the plain fit over every row is worse
    print("smallest margin %.3g" % worst)


def _outside_view():
    """A view through the lens whose theta_d has a maximum, 12 rows, row 0 (lowest id) moved to a pixel no direction projects to."""
    Kn, kn = sx.cam("FN")
    _, imgs, ids_l, _ = fx.make_views(11, 1, Kn, kn, rows=12)
    kp = fx.keypoints(imgs, ids_l)[0]
    kp[0, :2] = [Kn[0, 2] + 1.02 * frx.THETA_D_MAX_FN * Kn[0, 0], Kn[1, 2]]
    assert np.isnan(fisheye.undistort_points_host(kp[:1, :2], Kn, kn)).all()
    return kp, Kn, kn


def test_a_sample_with_an_outside_pixel_has_no_hypothesis():
    """One hypothesis, the seed chosen so that its sample holds the outside row: no hypothesis at all (DEGENERATE, winner -1); a
    seed whose sample avoids the row gives hypothesis 0, and the row is an outlier of it.  Over 100 hypotheses the winner's sample
    never holds the row."""
    kp, Kn, kn = _outside_view()
    ids, rm1 = kp[:, 2].astype(np.int64), fx.BOARD[1] - 1
    samples = {seed: pnp._ransac_sample(seed, 12, 0, ids, rm1) for seed in range(40)}
    hit = next(seed for seed, s in samples.items() if s is not None and 0 in s)
    miss = next(seed for seed, s in samples.items() if s is not None and 0 not in s)
    call = lambda **kw: fisheye.solve_pnp_fisheye_ransac_host_full(kp, *fx.BOARD, Kn, kn, reproj_error=REPROJ, **kw)
    st, pose, mask, winner = call(iterations=1, seed=hit)
    assert (st, winner) == (pnp.PNP_DEGENERATE, -1) and not pose.any() and not mask.any()
    st, pose, mask, winner = call(iterations=1, seed=miss)
    assert (st, winner) == (pnp.PNP_OK, 0) and mask.tolist() == [False] + [True] * 11
    st, pose, mask, winner = call(iterations=100, seed=SEED)
    assert st == pnp.PNP_OK and mask.tolist() == [False] + [True] * 11
    assert 0 not in pnp._ransac_sample(SEED, 12, winner, ids, rm1)
    # without consensus the view is refused: a pixel outside the model
    assert fisheye.solve_pnp_fisheye_host_full(kp, *fx.BOARD, Kn, kn)[0] == pnp.PNP_DEGENERATE


def test_too_few_rows_no_consensus_and_refused_arguments():
    kp, good, _ = swapped_views(1)[0]
    st, pose, mask, winner = _ransac(kp[:3])
    assert (st, winner) == (pnp.PNP_TOO_FEW, -1) and mask.shape == (3,) and not mask.any() and not pose.any()
    st, pose, mask, winner = _ransac(kp, min_inliers=26)                  # 25 rows agree
    assert st == pnp.PNP_NO_CONSENSUS and winner >= 0 and not mask.any() and not pose.any()
    assert fisheye.solve_pnp_fisheye_ransac_host(kp[:3], *fx.BOARD, K, KD)[0] is False
    for kw in (dict(iterations=0), dict(iterations=pnp.RANSAC_MAX_ITERATIONS + 1), dict(reproj_error=0.0), dict(reproj_error=np.inf)):
        with pytest.raises(ValueError):
            _ransac(kp, **kw)
    with pytest.raises(ValueError):
        fisheye.solve_pnp_fisheye_ransac_host_full(kp, *fx.BOARD, K, np.zeros(5))


def planted_mixed_scene():
    """test_rig_host's planted scene on the mixed fan: sigma = 0.3 px, 6 timestamps, 20 rows per view, in every view two pairs of
    rows exchange their ids -> (scene, good-row masks per camera)."""
    s = class_scene("fan3 F/P/F", 5, 0.3, rows=20)
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


def consensus_masks(s, ransac=RANSAC):
    """Per camera and view the consensus mask of that camera's model (the host definitions)."""
    cameras, dists = frx.cam_args(s)
    fn = {"pinhole": pnp.solve_pnp_ransac_host, "fisheye": fisheye.solve_pnp_fisheye_ransac_host}
    return [[fn[m](kp, *s.board, cameras[c], dists[c], **ransac)[3] for kp in s.kps[c]] for c, m in enumerate(frx.models(s))]


def test_masks_from_the_consensus_solvers_clean_a_mixed_rig():
    s, good = planted_mixed_scene()
    masks = consensus_masks(s)
    assert all(np.array_equal(m, g) for c in range(3) for m, g in zip(masks[c], good[c]))
    masked, plain = solve(s, masks=masks), solve(s)
    true_rows = rig.rig_calibrate_host_full([[k[g] for k, g in zip(s.kps[c], good[c])] for c in range(3)], *s.board, *frx.cam_args(s),
                                            models=frx.models(s))
    for a, b in zip(masked, true_rows):
        assert np.array_equal(a, b)
    eM, eP = rx.rig_errors(masked, s), rx.rig_errors(plain, s)
    print(f"planted: masked rms {masked.rms:.3f} px, rig error {eM}; unmasked rms {plain.rms:.3f} px (status {plain.status}), rig error {eP}")
    assert masked.status == rig.RIG_OK and (masked.view_points == 16).all() and masked.points_used == 6 * 48
    assert plain.status != rig.RIG_OK or (plain.rms >= 10 * masked.rms and eP[0] >= 10 * eM[0])      # test_rig_host's conditions
    assert masked.rms <= 0.45 and eM[0] <= 1e-2
