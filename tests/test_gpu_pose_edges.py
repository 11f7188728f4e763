"""The device pose and calibration kernels (csrc/dcx_pnp.hip, dcx_pnp_ransac.hip, dcx_calib.hip: three copies of csrc/dcx_pnp_dev.h)
on the scenario grid of tests/camera_exact.py: non-square boards, fx != fy, no / 4 / 5 / 8 distortion coefficients, boards that
face the camera or stand upside down in the image plane, and 4 / 5 / 63 / 64 / 65 / 129 rows.

Each frame is held twice: to the host definition with the gates of test_gpu_pnp.py / test_gpu_pnp_ransac.py / test_gpu_calib.py
(their helpers, imported unchanged), and to the exact camera model itself with the assertions of tests/test_pose_exact_host.py
applied to the device's own numbers.  The initialisation shows only in the accepted LM steps (Levenberg-Marquardt heals a wrong
start), so on noise-free frames the device's count may exceed the host's for the same frame by at most one."""
import collections

import numpy as np
import pytest
import torch

import camera_exact as A
import pool_cases
from deepcharuco_amd import calib, corner_pool, pnp
from test_gpu_calib import ABS_DIST, REL_K, REL_POSE, REL_RMS, _gaps
from test_gpu_pnp import REL, _agree
from test_gpu_pnp_ransac import MARGIN, _check_frame
from test_pose_exact_host import (branch_margin, check_calibration_recovers, check_optimality, check_recovery, host_results,
                                  ransac_args)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


ROT_VIEWS = ("fronto", "tiny", "pi", "near_pi")


def _agree_rot(dev8, host8, tally):
    """test_gpu_pnp._agree with the same numbers, for views where the relative gap of the rotation *vectors* measures nothing.
    Near a half turn r and r (1 - 2 pi / |r|) are one rotation, and a half turn about the optical axis leaves the sign of its
    vector to the rounding of a matrix entry near zero.  At r = 0 the gap is divided by |r| itself: on the first device run of
    this grid a fronto-parallel frame recovered |r| = 1.7e-7 on both sides, 3e-15 rad apart, which is 1.6e-8 of |r|.  So the
    vectors' relative gap is replaced by max |R(dev) - R(host)|; the tvec gap, the step-cap rule and the cost rule are
    _agree's."""
    d = max(A.rot_gap(dev8[:3], host8[:3]), np.linalg.norm(dev8[3:6] - host8[3:6]) / np.linalg.norm(host8[3:6]))
    if d <= REL:
        tally[0] += 1
        return
    assert max(dev8[7], host8[7]) < pnp.LM_MAX_ITER or dev8[7] == host8[7] == pnp.LM_MAX_ITER, (dev8, host8)
    if dev8[7] == host8[7] == pnp.LM_MAX_ITER:
        tally[2] += 1
        return
    assert d <= 1e-6 and abs(dev8[6] - host8[6]) <= 1e-12 * host8[6], (d, dev8, host8)
    tally[1] += 1


def _agree_any(f_view, dev8, host8, tally):
    (_agree_rot if f_view in ROT_VIEWS else _agree)(dev8, host8, tally)


def _check_rot(d, h, name, rms_floor=0.0):
    """test_gpu_calib._check for view sets that hold fronto-parallel and half-turn views: every assertion and number is its, but
    the poses' rotation gap is max |R(dev) - R(host)| over the used views in place of the vectors' relative gap (_agree_rot)."""
    assert d.view_status.tolist() == h.view_status.tolist(), name
    assert d.status == h.status == calib.CALIB_OK, (name, d.status, h.status)
    assert (d.views_used, d.points_used) == (h.views_used, h.points_used)
    assert d.view_points.tolist() == h.view_points.tolist()
    g = _gaps(d, h)
    g["rvec"] = max(A.rot_gap(d.rvecs[i], h.rvecs[i]) for i in np.flatnonzero(h.view_status == pnp.PNP_OK))
    print(f"{name}: device - host gaps {g}; steps / attempts device {d.iterations} / {d.attempts}, host {h.iterations} / "
          f"{h.attempts}")
    assert g["K"] <= REL_K and g["dist"] <= ABS_DIST, (name, g)
    assert g["rvec"] <= REL_POSE and g["tvec"] <= REL_POSE, (name, g)
    floor = g["rms"] > REL_RMS
    assert not floor or abs(d.rms - h.rms) <= rms_floor, (name, g, d.rms, h.rms)
    unused = np.flatnonzero(d.view_status != pnp.PNP_OK)
    assert not d.rvecs[unused].any() and not d.tvecs[unused].any() and not d.view_rms[unused].any()
    return g, floor


def _check_frame_rot(got, kp, board, cam, dist, ransac, tally, tag):
    """test_gpu_pnp_ransac._check_frame with _agree_rot as its pose gate; every discrete assertion is the same."""
    st, pose, mask, winner = got
    hs, hp, hm, hw, margin = pnp.solve_pnp_ransac_host_full(kp, *board, cam, dist, with_margin=True, **ransac)
    print(tag, "host status", hs, "winner", hw, "inliers", int(hm.sum()), "margin %.3g" % margin, "| device", st, winner, int(mask.sum()))
    assert margin >= MARGIN, (tag, margin)
    assert st == hs and winner == hw, (tag, st, hs, winner, hw)
    assert mask.dtype == bool and np.array_equal(mask, hm), (tag, mask, hm)
    if hs == pnp.PNP_OK:
        _agree_rot(pose, hp, tally)
    else:
        assert not pose.any() and not mask.any()
    return hs


def _check_frame_any(f_view, *args):
    return (_check_frame_rot if f_view in ROT_VIEWS else _check_frame)(*args)


# ------------------------------------------------------------------------------------------------ the plain solver

def test_plain_solver_on_the_grid(dev):
    G, host = A.grid(), host_results()
    branch_margin()                                      # asserts: no frame within a factor 10 of the conversion's switch
    tallies = collections.defaultdict(lambda: [0, 0, 0])
    total, n_ok, worst_grad, steps_over = [0, 0, 0], 0, 0.0, collections.Counter()
    worst_rec, dev_steps, dev_cap = collections.defaultdict(float), collections.defaultdict(collections.Counter), 0
    for board in A.BOARDS:
        for model, dist in A.MODELS.items():
            idx = [i for i, f in enumerate(G) if f.board == board and f.model == model]
            frames = [G[i].kp for i in idx]
            packed, b, pool = corner_pool.pack_keypoints(frames, dev)
            st, pose = pnp.solve_pnp_pool(packed, b, pool, True, *board, A.K_EDGE, dist)
            st, pose = st.cpu().numpy(), pose.cpu().numpy()
            got = pnp.solve_pnp_batch_device(frames, *board, A.K_EDGE, dist)        # the list form is the pool form, unpacked
            for j, i in enumerate(idx):
                f, (hs, hp) = G[i], host[i]
                assert st[j] == hs == pnp.PNP_OK, (f.tag, st[j], hs)
                assert got[j][0] is True and np.array_equal(np.r_[got[j][1].ravel(), got[j][2].ravel()], pose[j, :6]), f.tag
                n_ok += 1
                before = list(total)
                _agree_any(f.view, pose[j], hp, total)
                for c in range(3):
                    tallies[(f"{board[0]}x{board[1]}", model, f.view)][c] += total[c] - before[c]
                # and the device's own numbers against the exact model
                if not f.sigma:
                    worst_rec[f.n >= 6] = max(worst_rec[f.n >= 6], *check_recovery(f, pose[j]))
                    dev_steps[f.n >= 6][int(pose[j, 7])] += 1
                    steps_over[int(pose[j, 7] - hp[7])] += 1
                    assert pose[j, 7] <= hp[7] + 1, (f.tag, pose[j, 7], hp[7])
                elif pose[j, 7] < pnp.LM_MAX_ITER:
                    worst_grad = max(worst_grad, check_optimality(f, pose[j]))
                else:
                    dev_cap += 1
    for key in sorted(tallies):
        print("%-6s dist %-4s %-8s within 1e-9 / fallback / cap: %s" % (*key, tallies[key]))
    print("all frames: within 1e-9 / stopping-rule fallback / 20-step cap:", total, "of", n_ok)
    print("noise-free frames, device steps minus host steps:", sorted(steps_over.items()),
          "; noisy frames, worst |J^T r| / (|J| |r|) of the device pose by the exact model: %.3g" % worst_grad)
    print("device against the truth, noise-free: worst gap >= 6 rows %.3g, 4 and 5 rows %.3g; accepted steps >= 6 rows %s, 4 and 5 rows %s; "
          "%d device frames ran into the step cap" % (worst_rec[True], worst_rec[False], sorted(dev_steps[True].items()),
                                                      sorted(dev_steps[False].items()), dev_cap))
    assert n_ok == len(G) and sum(total) == n_ok and total[0] >= 0.75 * n_ok
    assert total[2] <= 0.05 * n_ok and dev_cap <= 0.05 * n_ok


# ------------------------------------------------------------------------------------------------ RANSAC

def test_ransac_planted_and_clean_edge_frames(dev):
    planted = A.planted_frames()
    clean = [f for f in A.grid() if f.n <= 5 and f.model in ("none", "8") and f.board in A.BOARDS[1:3]]
    groups = collections.defaultdict(list)
    for f, good in planted:
        groups[(f.board, f.model)].append((f, good))
    for f in clean:
        groups[(f.board, f.model)].append((f, None))
    tally, n_ok, statuses = [0, 0, 0], 0, collections.Counter()
    for (board, model), items in groups.items():
        dist = A.MODELS[model]
        got = pnp.solve_pnp_ransac_batch_device([f.kp for f, _ in items], *board, A.K_EDGE, dist, full=True, **ransac_args())
        for (f, good), g in zip(items, got):
            hs = _check_frame_any(f.view, g, f.kp, board, A.K_EDGE, dist, ransac_args(), tally, f.tag)
            statuses[hs] += 1
            n_ok += hs == pnp.PNP_OK
            if good is not None:
                assert g[0] == pnp.PNP_OK and np.array_equal(g[2], good), f.tag               # the planted rows, exactly
            elif not f.sigma:
                assert g[0] == pnp.PNP_OK and g[2].all(), f.tag
    print("statuses", dict(statuses), "; within 1e-9 / stopping-rule fallback / 20-step cap:", tally, "of", n_ok)
    assert sum(tally) == n_ok and tally[0] >= 0.75 * n_ok and n_ok >= len(planted) + len(clean) // 2


@pytest.mark.parametrize("iterations", [1, 64, 65, 4096])
def test_ransac_iteration_counts(dev, iterations):
    """1 (a single hypothesis), 64 / 65 (a full wave of hypotheses and one more) and the maximum, on a 63-row and a 30-row
    planted frame and a clean 5-row frame."""
    planted = A.planted_frames()
    items = [planted[0][0], planted[17][0], next(f for f in A.grid() if f.n == 5 and f.model == "8" and not f.sigma)]
    tally = [0, 0, 0]
    for f in items:
        args = ransac_args(iterations=iterations)
        dist = A.MODELS[f.model]
        g = pnp.solve_pnp_ransac_batch_device([f.kp], *f.board, A.K_EDGE, dist, full=True, **args)[0]
        _check_frame_any(f.view, g, f.kp, f.board, A.K_EDGE, dist, args, tally, f"{iterations} iterations, {f.tag}")
        assert 0 <= g[3] < iterations or g[3] == -1


# ------------------------------------------------------------------------------------------------ calibration

def _kps(imgs, ids_l):
    return [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]


@pytest.mark.parametrize("seed,n_views,sigma", [(11, 32, 0.0), (12, 64, 0.3)])
def test_calibration_matches_host_on_exact_views(dev, seed, n_views, sigma):
    """The view sets of test_pose_exact_host (7 x 11 board, 400 x 240 image, a quarter of the views fronto-parallel or rolled by
    180 degrees) with test_gpu_calib's gates; the noise-free set also recovers the truth."""
    objs, imgs, ids_l, poses = A.calib_views(seed, n_views, sigma)
    h = calib.calibrate_camera_host_full(objs, imgs, A.CALIB_SIZE)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *A.CALIB_BOARD, A.CALIB_SIZE)
    _check_rot(d, h, f"{n_views} exact views sigma {sigma}", rms_floor=1e-12 if sigma == 0.0 else 0.0)
    if not sigma:
        check_calibration_recovers(d, poses)


def test_calibration_recovers_the_truth_from_256_exact_views(dev):
    objs, imgs, ids_l, poses = A.calib_views(13, 256)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *A.CALIB_BOARD, A.CALIB_SIZE)
    print("256 views: steps / attempts", d.iterations, d.attempts)
    check_calibration_recovers(d, poses)


# ------------------------------------------------------------------------------------------------ the pool forms

POOL_BOARD, OTHER_BOARD, POOL_SIZE = (9, 6, 0.02), (6, 9, 0.02), (316, 248)     # 40 ids each; the init's principal point (157.5, 123.5)


def hand_built_pool(board=POOL_BOARD):
    """16 noise-free views of the board (camera K_EDGE, 5 coefficients), a view with id 40 (one past the board's last) and a
    3-row view, in scrambled pool order with gaps -> (keypoints, true poses, packed, B, pool, expected status)."""
    objs, imgs, ids_l, poses = A.calib_views(21, 16, board=board, K=A.K_EDGE, dist=A.DIST8[:5], tz=(0.15, 0.2))
    kps = _kps(imgs, ids_l)
    assert all(k[-1, 2] == 39 for k in kps[::4])                                       # the board's last id is in use
    bad = kps[1].copy()
    bad[-1, 2] = 40
    kps += [bad, kps[2][:3].copy()]
    B = len(kps)
    order = list(np.random.default_rng(5).permutation(B))
    gap = 3
    pool = sum(len(k) + gap for k in kps)
    packed, _ = pool_cases.lay_frames(kps, pool, order, gap=gap, filler=-9)
    expect = [pnp.PNP_OK] * 16 + [pnp.PNP_BAD_ID, pnp.PNP_TOO_FEW]
    return kps, poses, packed, B, pool, expect


def _rint(kp):
    return np.c_[np.rint(kp[:, :2]).astype(np.int64), kp[:, 2].astype(np.int64)]


@pytest.mark.parametrize("refined", [True, False])
def test_pool_forms_on_non_square_boards(dev, refined):
    """The launchers' own row_count - 1 and id-count arguments.  On a 9 x 6 and on a 6 x 9 board id 39 is valid and 40 is
    BAD_ID, and each board's views recover their true poses.  The 9 x 6 pool read as a 6 x 9 board: the same ids are other
    board points, no rigid pose fits them, and the rms the kernel reports is the one the exact model gives at its pose."""
    dist = A.DIST8[:5]
    view = (lambda kp: kp) if refined else _rint
    tally = [0, 0, 0]
    for board in (POOL_BOARD, OTHER_BOARD):
        kps, poses, packed, B, pool, expect = hand_built_pool(board)
        d = torch.from_numpy(packed).to(dev)
        st, pose = (t.cpu().numpy() for t in pnp.solve_pnp_pool(d, B, pool, refined, *board, A.K_EDGE, dist))
        assert st.tolist() == expect and not pose[16:].any(), (board, st.tolist())
        for b in range(16):
            hs, hp = pnp.solve_pnp_host_full(view(kps[b]), *board, A.K_EDGE, dist)
            assert hs == pnp.PNP_OK
            _agree_rot(pose[b], hp, tally)
            if refined:                                                              # noise-free: the truth, by the exact model
                f = A.Frame(kps[b], poses[b, :3], poses[b, 3:], board, "5", "", len(kps[b]), 0.0, f"{board} pool view {b}")
                check_recovery(f, pose[b])
    print(f"refined={refined}: within 1e-9 / fallback / cap:", tally)
    assert tally[0] >= 0.75 * sum(tally)
    kps, poses, packed, B, pool, expect = hand_built_pool(POOL_BOARD)
    d = torch.from_numpy(packed).to(dev)
    st9, pose9 = (t.cpu().numpy() for t in pnp.solve_pnp_pool(d, B, pool, refined, *POOL_BOARD, A.K_EDGE, dist))
    st2, pose2 = (t.cpu().numpy() for t in pnp.solve_pnp_pool(d, B, pool, refined, *OTHER_BOARD, A.K_EDGE, dist))
    assert st2.tolist()[16:] == expect[16:]
    n_cross = 0
    for b in range(16):
        hs, _ = pnp.solve_pnp_host_full(view(kps[b]), *OTHER_BOARD, A.K_EDGE, dist)
        assert st2[b] == hs, (b, st2[b], hs)
        if hs == pnp.PNP_OK:
            srt = view(kps[b])[np.argsort(kps[b][:, 2], kind="stable")]
            obj = A.board_points(srt[:, 2], *OTHER_BOARD)
            rms = np.sqrt(A.cost(obj, srt[:, :2].astype(np.float32), pose2[b, :6], A.K_EDGE, dist) / len(obj))
            assert abs(rms - pose2[b, 6]) <= 1e-9 * rms and rms > 1.0 > pose9[b, 6], (b, rms, pose2[b, 6], pose9[b, 6])
            assert not np.array_equal(pose2[b, :6], pose9[b, :6])
            n_cross += 1
    assert n_cross >= 8
    # RANSAC
    args = ransac_args(min_inliers=6)
    st, pose_r, info, inl = (t.cpu().numpy() for t in pnp.solve_pnp_ransac_pool(d, B, pool, refined, *POOL_BOARD, A.K_EDGE, dist, **args))
    assert st.tolist() == expect
    counts, starts = packed[:B], packed[B:2 * B]
    rt = [0, 0, 0]
    for b in range(16):
        mask = inl[starts[b]:starts[b] + counts[b]].astype(bool)
        assert info[b, 0] == mask.sum()
        got = (int(st[b]), pose_r[b], mask, int(info[b, 1]))
        hs = _check_frame_rot(got, view(kps[b]), POOL_BOARD, A.K_EDGE, dist, args, rt, f"refined={refined} view {b}")
        assert hs == pnp.PNP_OK
        if refined:
            assert mask.all()
    assert not pose_r[16:].any() and (info[16:, 1] == -1).all() and rt[0] >= 12, rt
    # calibration
    c = calib.calibrate_charuco_pool(d, B, pool, refined, *POOL_BOARD, POOL_SIZE)
    assert c.view_status.tolist() == expect and c.view_points.tolist() == [len(k) for k in kps]
    use = list(range(16)) + [17]
    objs = [pnp.object_points(kps[b][:, 2], *POOL_BOARD) for b in use]
    imgs = [view(kps[b])[:, :2].astype(np.float32) for b in use]
    h = calib.calibrate_camera_host_full(objs, imgs, POOL_SIZE)
    sel = np.array(use)
    sub = c._replace(view_status=c.view_status[sel], rvecs=c.rvecs[sel], tvecs=c.tvecs[sel], view_rms=c.view_rms[sel],
                     view_points=c.view_points[sel])
    _check_rot(sub, h, f"9x6 pool refined={refined}", rms_floor=1e-12 if refined else 0.0)
    assert not c.rvecs[16:].any()
