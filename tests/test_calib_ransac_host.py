"""The robust calibration's host definition (deepcharuco_amd/calib.py, calibrate_camera_ransac_host_full): clean views give the
plain solve bit for bit, planted wrong ids are found exactly, true rows a tight consensus threshold drops are re-admitted by
the re-mask, a view whose winner holds a planted row is left out, every status, position independence, argument handling and
the C ABI's argument checks.  No GPU needed.

The scenes are test_calib_host's (24 views of the 8x8 board, 320x240, all five distortion terms non-zero).  Planting
(``planted_views``): in every second view with >= 8 rows, 1-3 disjoint pairs of rows (one pair per 8 rows at most) exchange
their image points, seeded by 1000 + the scene's seed; that makes 4.5-4.8 % of the rows wrong.  Scene seeds 3 / 4 / 5 at sigma
0 / 0.05 / 0.2 are the ones the definition was run on when this file was written; with the default parameters it returns the
planted truth on all three."""
import ctypes
import functools

import numpy as np
import pytest

from deepcharuco_amd import calib, pnp
from test_calib_host import BOARD, K_TRUE, SIZE, make_views

SCENES = ((3, 0.0), (4, 0.05), (5, 0.2))


def keypoints(imgs, ids_l):
    return [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]


def planted_views(seed, n_views, sigma, f32=True):
    """-> (keypoint arrays [x, y, id], truth masks, true poses): make_views(seed, n_views, sigma) with exchanged image points."""
    _, imgs, ids_l, poses = make_views(seed, n_views, sigma=sigma, f32=f32)
    rng = np.random.default_rng(1000 + seed)
    kps, truth = [], []
    for v, (m, ids) in enumerate(zip(imgs, ids_l)):
        m, good = m.copy(), np.ones(len(ids), bool)
        if len(ids) >= 8 and v % 2 == 1:
            pairs = min(int(rng.integers(1, 4)), len(ids) // 8)
            for a, b in rng.choice(len(ids), 2 * pairs, replace=False).reshape(-1, 2):
                m[[a, b]] = m[[b, a]]
                good[[a, b]] = False
        kps.append(np.c_[m.astype(np.float64), ids])
        truth.append(good)
    return kps, truth, poses


def plain(kps, masks=None):
    """calibrate_camera_host_full on the (masked) rows of keypoint arrays."""
    masks = [np.ones(len(k), bool) for k in kps] if masks is None else masks
    return calib.calibrate_camera_host_full([pnp.object_points(k[m, 2], *BOARD) for k, m in zip(kps, masks)],
                                            [k[m, :2].astype(np.float32) for k, m in zip(kps, masks)], SIZE)


def same_solution(r, ref):
    return (np.array_equal(r.camera_matrix, ref.camera_matrix) and np.array_equal(r.dist_coeffs, ref.dist_coeffs)
            and np.array_equal(r.rvecs, ref.rvecs) and np.array_equal(r.tvecs, ref.tvecs) and r.rms == ref.rms)


def same_masks(a, b):
    return len(a) == len(b) and all(x.dtype == bool and np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def scene(seed, sigma):
    return planted_views(seed, 24, sigma)


def test_clean_views_give_the_plain_solve_bit_for_bit():
    objs, imgs, ids_l, _ = make_views(3, 24)
    ref = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    r = calib.calibrate_camera_ransac_host_full(keypoints(imgs, ids_l), *BOARD, SIZE)
    assert r.status == ref.status == calib.CALIB_OK and same_solution(r, ref)
    assert all(m.all() for m in r.inliers) and r.view_inliers.tolist() == [len(i) for i in ids_l] == r.view_points.tolist()
    assert r.solves == 1 and r.stable is True and (r.winners >= 0).all()
    assert (r.iterations, r.attempts, r.views_used, r.points_used) == (ref.iterations, ref.attempts, ref.views_used, ref.points_used)
    # cv2's 5-tuple and the masks
    rms, K, dist, rvecs, tvecs, inl = calib.calibrate_camera_ransac_host(keypoints(imgs, ids_l), *BOARD, SIZE)
    assert rms == r.rms and np.array_equal(K, r.camera_matrix) and dist.shape == (1, 5) and same_masks(inl, r.inliers)
    assert len(rvecs) == 24 and rvecs[0].shape == (3, 1) and np.array_equal(tvecs[5].ravel(), r.tvecs[5])


@pytest.mark.parametrize("seed,sigma", SCENES)
def test_planted_rows_are_found_exactly(seed, sigma):
    kps, truth, _ = scene(seed, sigma)
    n_bad = sum(int((~t).sum()) for t in truth)
    assert 30 <= n_bad and sum(not t.all() for t in truth) >= 10
    broken = plain(kps)                                              # the need: success reported, a wrong model returned
    print(f"seed {seed}: plain solve on the planted views: status {broken.status}, rms {broken.rms:.3f} px, fx off by "
          f"{broken.camera_matrix[0, 0] - K_TRUE[0, 0]:.2f} px")
    assert broken.status == calib.CALIB_OK and broken.rms > 10.0
    r, margin = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, with_margin=True)
    print(f"seed {seed}: robust rms {r.rms:.3g} px, solves {r.solves}, margin {margin:.3g}")
    assert r.status == calib.CALIB_OK and (r.view_status == pnp.PNP_OK).all() and same_masks(r.inliers, truth)
    assert margin > 0 and r.stable
    ref = plain(kps, truth)
    assert same_solution(r, ref) and r.points_used == ref.points_used == sum(int(t.sum()) for t in truth)
    assert r.view_points.tolist() == [len(k) for k in kps] and r.view_inliers.tolist() == [int(t.sum()) for t in truth]
    assert np.array_equal(r.view_rms, ref.view_rms)


def test_rows_dropped_by_a_tight_consensus_are_readmitted():
    kps, truth, _ = scene(3, 0.0)
    tight = dict(consensus_error=2.0, min_inliers=4)
    step_b = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, rounds=0, **tight)      # rounds=0: step B's masks
    dropped = sum(int((t & ~m).sum()) for t, m in zip(truth, step_b.inliers))
    print("true rows dropped by the 2 px homography consensus:", dropped)
    assert dropped > 0 and step_b.solves == 1 and step_b.stable is False
    assert not any((m & ~t).any() for t, m in zip(truth, step_b.inliers))                       # (no planted row got in)
    r = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, **tight)
    assert same_masks(r.inliers, truth) and r.solves == 2 and r.stable and same_solution(r, plain(kps, truth))
    # the documented rule: a view lost at step B stays lost
    r6 = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, consensus_error=2.0, min_inliers=6)
    lost = np.flatnonzero(r6.view_status == pnp.PNP_NO_CONSENSUS)
    assert lost.size == 1 and not r6.inliers[lost[0]].any() and r6.views_used == 23
    keep = [b for b in range(24) if b != lost[0]]
    assert same_masks([r6.inliers[b] for b in keep], [truth[b] for b in keep])


def small_view_batch():
    """12 clean views around one view of 8 rows, 3 of them displaced by 15-60 px -> (views, index of the small one, the
    displaced rows).  Under SMALL_SEED the winning sample holds displaced row 6 and the consensus takes it in."""
    _, imgs, ids_l, _ = make_views(11, 13)
    kps = keypoints(imgs, ids_l)
    rng = np.random.default_rng(77)
    small = kps[0][np.sort(rng.choice(len(kps[0]), 8, replace=False))].copy()
    bad = np.array([1, 4, 6])
    ang, mag = rng.uniform(0, 2 * np.pi, 3), rng.uniform(15, 60, 3)
    small[bad, 0] += mag * np.cos(ang)
    small[bad, 1] += mag * np.sin(ang)
    return kps[1:7] + [small] + kps[7:], 6, bad


SMALL_SEED = 17


def test_a_view_whose_winner_holds_a_planted_row_is_left_out():
    views, at, bad = small_view_batch()
    small = views[at]
    obj = pnp.object_points(small[:, 2], *BOARD).astype(np.float64)
    img = small[:, :2].astype(np.float32).astype(np.float64)
    ids = small[:, 2].astype(np.int64)
    st, mask, winner, score, _ = calib._view_consensus(obj, img, ids, BOARD[1], 100, 8.0, 6, SMALL_SEED)
    sample = pnp._ransac_sample(SMALL_SEED, 8, winner, ids, BOARD[1] - 1)
    assert st == pnp.PNP_OK and set(sample) & set(bad.tolist()) and mask[list(set(sample) & set(bad.tolist()))].all()
    assert score == int(mask.sum()) >= 6
    r = calib.calibrate_camera_ransac_host_full(views, *BOARD, SIZE, seed=SMALL_SEED)
    assert r.status == calib.CALIB_OK and r.view_status[at] == pnp.PNP_NO_CONSENSUS and not r.inliers[at].any()
    assert r.winners[at] == winner and r.view_inliers[at] == 0 and r.view_points[at] == 8
    assert not r.rvecs[at].any() and not r.tvecs[at].any() and r.view_rms[at] == 0.0
    assert r.solves == 2 and r.stable and r.views_used == 12
    others = [b for b in range(13) if b != at]
    assert (r.view_status[others] == pnp.PNP_OK).all() and all(r.inliers[b].all() for b in others)
    assert np.abs(r.camera_matrix - K_TRUE).max() <= 1e-5 * 400                # test_truth_recovery_float32's gate
    assert same_solution(r._replace(rvecs=r.rvecs[others], tvecs=r.tvecs[others]), plain([views[b] for b in others]))


def every_status_batch(seed=30):
    """-> (views, expected view status): OK views, 3 rows, an empty view, a bad id, a board column, scattered corners, and a clean
    5-row view that only min_inliers = 6 turns away."""
    _, imgs, ids_l, _ = make_views(seed, 10, sigma=0.3)
    kps = keypoints(imgs, ids_l)
    rng = np.random.default_rng(seed)
    bad = kps[3].copy()
    bad[1, 2] = 49
    scattered = kps[4].copy()[:12]
    scattered[:, :2] = np.c_[rng.uniform(5, 315, 12), rng.uniform(5, 235, 12)]
    column = np.c_[np.linspace(20, 300, 7), np.linspace(30, 200, 7), np.arange(7) * 7]
    five = kps[5][[0, 2, 3, 5, 6]].copy() if len(kps[5]) >= 7 else kps[5][:5].copy()
    views = kps[:2] + [kps[0][:3].copy(), np.zeros((0, 3))] + kps[2:6] + [bad, column, scattered, five] + kps[6:]
    expect = [pnp.PNP_OK] * 2 + [pnp.PNP_TOO_FEW] * 2 + [pnp.PNP_OK] * 4 + [pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE,
                                                                          pnp.PNP_NO_CONSENSUS, pnp.PNP_NO_CONSENSUS] + [pnp.PNP_OK] * 4
    return views, expect


def test_every_status_in_one_batch():
    views, expect = every_status_batch()
    r = calib.calibrate_camera_ransac_host_full(views, *BOARD, SIZE)
    assert r.view_status.tolist() == expect and r.status == calib.CALIB_OK
    out = [b for b, e in enumerate(expect) if e != pnp.PNP_OK]
    assert r.view_points.tolist() == [len(v) for v in views]
    assert all(r.inliers[b].shape == (len(views[b]),) and not r.inliers[b].any() for b in out) and not r.view_inliers[out].any()
    assert not r.rvecs[out].any() and not r.tvecs[out].any() and not r.view_rms[out].any()
    assert r.winners[[2, 3, 8, 9]].tolist() == [-1] * 4 and (r.winners[[10, 11]] >= 0).all()
    ok = [b for b, e in enumerate(expect) if e == pnp.PNP_OK]
    assert r.views_used == len(ok) == 10 and same_solution(
        r._replace(rvecs=r.rvecs[ok], tvecs=r.tvecs[ok]), plain([views[b] for b in ok], [r.inliers[b] for b in ok]))
    # the 5-row view stands with min_inliers = 5 (4 is the floor: max(min_inliers, 4))
    r5 = calib.calibrate_camera_ransac_host_full(views, *BOARD, SIZE, min_inliers=5)
    assert r5.view_status[11] == pnp.PNP_OK and r5.inliers[11].all() and r5.view_status[10] == pnp.PNP_NO_CONSENSUS
    with pytest.raises(IndexError):
        calib.calibrate_camera_ransac_host(views, *BOARD, SIZE)
    with pytest.raises(ValueError):
        calib.calibrate_camera_ransac_host(views[:8], *BOARD, SIZE)
    none = calib.calibrate_camera_ransac_host_full([views[2], views[3], views[9]], *BOARD, SIZE)
    assert none.status == calib.CALIB_NO_VIEWS and none.views_used == 0 and none.solves == 1 and not none.camera_matrix.any()


def test_step_b_does_not_depend_on_the_position_in_the_batch():
    kps, truth, _ = scene(4, 0.05)
    at = 5                                                            # a planted view
    assert not truth[at].all()
    want = None
    for batch, pos in (([kps[at]] + kps[:4], 0), (kps[8:12] + [kps[at]], 4), (kps[20:22] + [kps[at]] + kps[12:14], 2)):
        r = calib.calibrate_camera_ransac_host_full(batch, *BOARD, SIZE, rounds=0)
        got = (int(r.winners[pos]), int(r.view_inliers[pos]), r.inliers[pos].tolist(), int(r.view_status[pos]))
        want = want or got
        assert got == want and got[3] == pnp.PNP_OK and r.inliers[pos].tolist() == truth[at].tolist()
    # rows handed over in another order: the pool holds them id-sorted, so the sampler sees the same slots
    perm = np.random.default_rng(0).permutation(len(kps[at]))
    r = calib.calibrate_camera_ransac_host_full([kps[at][perm]] + kps[:4], *BOARD, SIZE, rounds=0)
    assert int(r.winners[0]) == want[0] and r.inliers[0].tolist() == truth[at][perm].tolist()
    as_is = calib.calibrate_camera_ransac_host_full([kps[at]] + kps[:4], *BOARD, SIZE, rounds=0, pool_order=True)
    assert int(as_is.winners[0]) == want[0]                           # (make_views' rows are id-sorted already)


def test_argument_errors_and_rounds():
    _, imgs, ids_l, _ = make_views(40, 6)
    kps = keypoints(imgs, ids_l)
    for kw in (dict(iterations=0), dict(iterations=4097), dict(consensus_error=0.0), dict(consensus_error=float("nan")),
               dict(consensus_error=float("inf")), dict(reproj_error=0.0), dict(reproj_error=-1.0), dict(reproj_error=float("nan")),
               dict(rounds=-1), dict(rounds=9)):
        with pytest.raises(ValueError):
            calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, **kw)
        with pytest.raises(ValueError):
            calib.calibrate_camera_ransac_host(kps, *BOARD, SIZE, **kw)
    for size in ((0, 240), (320, -1)):
        with pytest.raises(ValueError):
            calib.calibrate_camera_ransac_host_full(kps, *BOARD, size)
    r0 = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, rounds=0)
    assert r0.solves == 1 and r0.stable is False and r0.status == calib.CALIB_OK
    r8 = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, rounds=8)
    assert r8.solves == 1 and r8.stable is True and np.array_equal(r8.camera_matrix, r0.camera_matrix)
    for name in ("RobustCalibResult", "calibrate_camera_ransac_host", "calibrate_camera_ransac_host_full",
                 "calibrate_charuco_ransac_pool", "calibrate_charuco_ransac_device", "ransac_workspace_bytes"):
        assert name in calib.__all__ and hasattr(calib, name)
    assert calib.RobustCalibResult._fields[:len(calib.CalibResult._fields)] == calib.CalibResult._fields


def test_null_abi_arguments_are_rejected_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    size = lib.dcx_calibrate_ransac_workspace_bytes
    for bad in ((0, 16, 100), (4, -1, 100), (4, 16, 0), (4, 16, 4097)):
        assert size(*bad) == 0
    ws = size(4, 16, 100)
    assert ws > lib.dcx_calibrate_workspace_bytes(4) + 4 * 100 * 4 + 16 * 25 and ws % 8 == 0
    assert size(8, 16, 100) > ws and size(4, 32, 100) > ws and size(4, 16, 200) > ws
    assert calib.ransac_workspace_bytes(4, 16) == ws
    with pytest.raises(ValueError):
        calib.ransac_workspace_bytes(4, 16, 0)
    res = (ctypes.c_double * 16)()
    p = 4096              # a non-null address that is never read: every call below fails a check before any device access
    # counts starts rows xy | batch pool col row square w h | iterations consensus reproj min_inliers rounds seed | ws bytes |
    # view_status pose info inliers h_result stream
    args = [p, p, p, p, 4, 16, 8, 8, 0.02, 320, 240, 100, 8.0, 3.0, 6, 2, 0, p, ws, p, p, p, p, res, None]
    for i in (0, 1, 2, 17, 19, 20, 21, 23):            # null counts, starts, rows, workspace, status, pose, info, h_result
        a = list(args)
        a[i] = None
        assert lib.dcx_calibrate_ransac_pool(*a) == -1, i
    nan, inf = float("nan"), float("inf")
    for i, v in ((4, 0), (5, -1), (6, 1), (7, 1), (8, nan), (9, 0), (10, 0), (11, 0), (11, 4097), (12, 0.0), (12, -1.0), (12, nan),
                 (12, inf), (13, 0.0), (13, nan), (13, inf), (15, -1), (15, 9), (17, p + 4)):
        a = list(args)
        a[i] = v
        assert lib.dcx_calibrate_ransac_pool(*a) == -1, (i, v)
    a = list(args)
    a[18] = ws - 8                                     # workspace too small
    assert lib.dcx_calibrate_ransac_pool(*a) == -3
