"""The device robust calibration (csrc/dcx_calib_ransac.hip through deepcharuco_amd/calib.py) against its host definition
calibrate_camera_ransac_host_full: planted scenes, a hand-built corner pool with every view status, the corner pool
infer_batch_device leaves in HBM, determinism, all-true masks against the plain device solve, 1,024 views, and the errors.

The discrete outputs (view status, winners, inlier counts, masks, number of solves, stable) must be EQUAL to the host's.  That is
fair because every scene compared here has a margin >= 1e-6, asserted from the host run first (no row of a hypothesis scoring
within one of its view's winner, and no row at any re-mask, lies closer than that, relatively, to its threshold): the bar of
tests/test_gpu_pnp_ransac.py, five orders above the ~1e-9 at which device and host agree.  With equal masks the inner solve is
dcx_calibrate_pool's kernels on the same rows, so the continuous outputs pass tests/test_gpu_calib.py's gates unchanged.  The
hand-built pool (10 standing views, one of 7 and one of 10 rows) is held to more than those gates: its continuous outputs are
the plain device solve's on the surviving rows BIT FOR BIT.  (Against the host that small set measured 3.2e-8 in k3 with refined
xy, the plain solver's own device-host gap there: section 3.9 of DESIGN.md reports 7e-8 on its small sets.)"""
import numpy as np
import pytest
import torch

import pool_cases
from conftest import GoldenCase
from deepcharuco_amd import _lib, calib, corner_pool, pnp
from test_calib_host import BOARD, DIST_TRUE, K_TRUE, SIZE, make_views
from test_calib_ransac_host import SMALL_SEED, every_status_batch, keypoints, planted_views, small_view_batch
from test_gpu_calib import _check, _gaps
from test_gpu_pnp_ransac import _pool_frames

pytestmark = pytest.mark.gpu

MARGIN = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _same_discrete(d, h, name):
    print(f"{name}: view status {h.view_status.tolist()}, inliers {h.view_inliers.tolist()} of {h.view_points.tolist()}, "
          f"solves {h.solves}, stable {h.stable} | device solves {d.solves}, stable {d.stable}")
    assert d.view_status.tolist() == h.view_status.tolist(), name
    assert d.winners.tolist() == h.winners.tolist() and d.view_inliers.tolist() == h.view_inliers.tolist(), name
    assert len(d.inliers) == len(h.inliers) and all(a.dtype == bool and np.array_equal(a, b) for a, b in zip(d.inliers, h.inliers))
    assert (d.solves, d.stable, d.status) == (h.solves, h.stable, h.status), name
    assert d.view_points.tolist() == h.view_points.tolist()


@pytest.mark.parametrize("seed,n_views,sigma", [(201, 8, 0.0), (202, 64, 0.3)])
def test_device_matches_host(dev, seed, n_views, sigma):
    kps, truth, _ = planted_views(seed, n_views, sigma)
    h, margin = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, with_margin=True)
    print(f"{n_views} views sigma {sigma}: host margin {margin:.3g}, planted rows {sum(int((~t).sum()) for t in truth)}")
    assert margin >= MARGIN
    rng = np.random.default_rng(seed)
    shuffled = [k[rng.permutation(len(k))] for k in kps]                 # the caller's row order is not the pool's
    hs = calib.calibrate_camera_ransac_host_full(shuffled, *BOARD, SIZE)
    d = calib.calibrate_charuco_ransac_device(shuffled, *BOARD, SIZE)
    _same_discrete(d, hs, f"{n_views} views")
    assert hs.winners.tolist() == h.winners.tolist() and hs.rms == h.rms   # (the host sorts as the pool does)
    assert not any((m & ~t).any() for m, t in zip(h.inliers, truth))     # no planted row survives
    # noise-free: the absolute 1e-12 px rms floor of test_gpu_calib.test_device_matches_host, for its stated reason
    _check(d, hs, f"{n_views} views sigma {sigma}", rms_floor=1e-12 if sigma == 0.0 else 0.0)


@pytest.mark.parametrize("name", ["readmitted", "rounds run out", "view lost at B", "view lost at D"])
def test_second_solves_match_host(dev, name):
    """The scenes of test_calib_ransac_host in which the re-mask changes a mask, so the device solves twice: rows a 2 px consensus
    dropped come back; the same with one round (two solves, nothing confirms the second); a view min_inliers turns away at step B
    stays away; a view whose winner held a displaced row falls to the re-mask."""
    if name == "view lost at D":
        kps, kw = small_view_batch()[0], dict(seed=SMALL_SEED)
    else:
        kps = planted_views(3, 24, 0.0)[0]
        kw = dict(consensus_error=2.0, min_inliers=6 if name == "view lost at B" else 4, rounds=1 if name == "rounds run out" else 2)
    h, margin = calib.calibrate_camera_ransac_host_full(kps, *BOARD, SIZE, with_margin=True, **kw)
    print(f"{name}: host margin {margin:.3g}")
    assert margin >= MARGIN and h.solves == 2 and h.stable is (name != "rounds run out")
    assert (pnp.PNP_NO_CONSENSUS in h.view_status.tolist()) is name.startswith("view lost")
    d = calib.calibrate_charuco_ransac_device(kps, *BOARD, SIZE, **kw)
    _same_discrete(d, h, name)
    _check(d, h, name, rms_floor=1e-12)                                  # (noise-free scenes: see test_device_matches_host)


def hand_built_pool(refined):
    """test_calib_ransac_host.every_status_batch plus a view cut by the end of the pool, scrambled, with gaps ->
    (the rows each view holds in the pool, packed, B, pool, slots that belong to a view)."""
    views, _ = every_status_batch()
    views = [v.copy() for v in views] + [views[0].copy()]                # TRUNCATED: placed last, cut
    if not refined:
        for v in views:
            v[:, :2] = np.rint(v[:, :2])
    B = len(views)
    order = list(np.random.default_rng(5).permutation(B - 1)) + [B - 1]
    gap = 3
    pool = sum(len(v) + gap for v in views) - gap - 4
    packed, owned = pool_cases.lay_frames(views, pool, order, gap=gap, filler=-9)
    if not refined:
        corner_pool.views(packed, B, pool)[3][:] = np.nan                # xy: not read
    return views, packed, B, pool, owned


@pytest.mark.parametrize("refined", [True, False])
def test_pool_hand_built_every_status(dev, refined):
    views, packed, B, pool, owned = hand_built_pool(refined)
    h, margin = calib.calibrate_camera_ransac_host_full(views[:-1], *BOARD, SIZE, with_margin=True, pool_order=True)
    print(f"refined={refined}: host margin {margin:.3g}")
    assert margin >= MARGIN
    assert set(h.view_status.tolist()) == {pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE, pnp.PNP_NO_CONSENSUS}
    inl = torch.full((pool,), 7, dtype=torch.uint8, device=dev)
    d = calib.calibrate_charuco_ransac_pool(torch.from_numpy(packed).to(dev), B, pool, refined, *BOARD, SIZE, out_inliers=inl)
    # the view cut by the pool: TRUNCATED, nothing of it used; it changes nothing for the others
    assert d.view_status[-1] == pnp.PNP_TRUNCATED and d.view_points[-1] == len(views[-1]) and d.winners[-1] == -1
    assert not d.inliers[-1].any() and d.inliers[-1].shape == (len(views[-1]),) and not d.rvecs[-1].any() and d.view_inliers[-1] == 0
    sub = d._replace(view_status=d.view_status[:-1], rvecs=d.rvecs[:-1], tvecs=d.tvecs[:-1], view_rms=d.view_rms[:-1],
                     view_points=d.view_points[:-1], inliers=d.inliers[:-1], view_inliers=d.view_inliers[:-1], winners=d.winners[:-1])
    _same_discrete(sub, h, f"hand-built pool refined={refined}")
    # the continuous outputs: the plain device solve over the rows the host kept, every view in its place (an empty view where
    # one was left out), gives the same bits: the consensus steps add nothing to the solve but the choice of rows
    kept = [v[m] if st == pnp.PNP_OK else v[:0] for v, m, st in zip(views[:-1], h.inliers, h.view_status)] + [views[-1][:0]]
    p = calib.calibrate_charuco_pool(*corner_pool.pack_keypoints(kept, dev), True, *BOARD, SIZE)
    assert p.status == calib.CALIB_OK and p.view_points.tolist() == d.view_inliers.tolist()
    _bits_equal([d.rms, d.camera_matrix, d.dist_coeffs, d.rvecs, d.tvecs, d.view_rms, d.iterations, d.attempts, d.views_used,
                 d.points_used], [p.rms, p.camera_matrix, p.dist_coeffs, p.rvecs, p.tvecs, p.view_rms, p.iterations, p.attempts,
                                  p.views_used, p.points_used])
    print(f"hand-built pool refined={refined}: device - host gaps {_gaps(sub, h)}")
    # the mask by slot: 7 where no view lives, the views' masks elsewhere (zeros over the cut view's slots inside the pool)
    got = inl.cpu().numpy()
    assert (got[~owned] == 7).all() and (got[owned] <= 1).all()
    for b in range(B):
        n, s0 = int(packed[b]), int(packed[B + b])
        assert np.array_equal(got[s0:min(s0 + n, pool)].astype(bool), d.inliers[b][:max(min(n, pool - s0), 0)])


REAL_CONSENSUS = 7.3


@pytest.mark.parametrize("name", ["diverse_ids_240x320", "board_240x320"])
def test_real_detections_pool(dev, name):
    """The unmodified tensor infer_batch_device returns (a frame's corners in raster order), against the host definition on the
    same rows in the same order.  Synthetic weights put the corners on no board, so what is pinned is the pool addressing and the
    order the sampler's slots count in: whatever the statuses are, they, the winners and the masks are the host's.  (Measured:
    every view of the diverse-ids frames scores hypotheses and ends NO_CONSENSUS; the board frames carry one id each, so no sample
    exists: DEGENERATE.)

    consensus_error is 7.3 px here, not the default 8: these pools hold the same id in neighbouring cells of the detector's
    8 px grid, 8.000 px apart, so a hypothesis through one of the two puts the other exactly on an 8 px threshold (host margin
    0 to 2e-16 on four of the six diverse-ids views) and rounding decides.  At 7.3 px the host margin of these pools is 1.2e-2;
    it is asserted like everywhere else."""
    from deepcharuco_amd.inference import infer_batch_device
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    case = GoldenCase(name)
    dc, rn = lModel(dcModel(case.n_ids, case.sd_dc, dev)), lRefineNet(RefineNet(case.sd_rn, dev))
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1], np.zeros_like(f), np.roll(f, 40, axis=1)])
    B, pool = len(frames), 64 * len(frames)
    packed = infer_batch_device(torch.from_numpy(np.ascontiguousarray(frames)).to(dev), case.n_ids, dc, rn, pool=pool)
    slots = _pool_frames(packed.cpu().numpy(), B, pool)
    assert max(len(s) for s in slots) >= 6
    h, margin = calib.calibrate_camera_ransac_host_full(slots, 5, 5, 0.01, (320, 240), consensus_error=REAL_CONSENSUS,
                                                        with_margin=True, pool_order=True)
    print(f"{name}: host margin {margin:.3g}, calibration status {h.status}")
    assert margin >= MARGIN
    d = calib.calibrate_charuco_ransac_pool(packed, B, pool, True, 5, 5, 0.01, (320, 240), consensus_error=REAL_CONSENSUS)
    _same_discrete(d, h, name)
    if name.startswith("diverse"):
        assert (h.winners[h.view_points >= 4] >= 0).all()                # hypotheses were scored on these rows
    if h.status == calib.CALIB_OK:
        _check(d, h, name)
    else:
        assert d.rms == 0.0 and not d.camera_matrix.any() and not d.rvecs.any() and not d.tvecs.any()


def _bits_equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def test_two_calls_give_the_same_bits(dev):
    kps, _, _ = planted_views(203, 96, 0.5)
    a = calib.calibrate_charuco_ransac_device(kps, *BOARD, SIZE)
    b = calib.calibrate_charuco_ransac_device(kps, *BOARD, SIZE)
    assert a.status == calib.CALIB_OK and a.view_inliers.sum() < a.view_points.sum()
    _bits_equal(a, b)


def test_all_true_masks_give_the_plain_device_solve(dev):
    """Clean views: every mask is all true, one solve, and the filtered pool is the pool: calibrate_charuco_pool's bits."""
    _, imgs, ids_l, _ = make_views(204, 48)
    kps = keypoints(imgs, ids_l)
    packed, b, pool = corner_pool.pack_keypoints(kps, dev)
    r = calib.calibrate_charuco_ransac_pool(packed, b, pool, True, *BOARD, SIZE)
    p = calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE)
    assert p.status == calib.CALIB_OK and r.solves == 1 and r.stable and all(m.all() for m in r.inliers)
    assert r.view_inliers.tolist() == r.view_points.tolist() == [len(k) for k in kps]
    _bits_equal(r[:len(p)], p)


def test_1024_views_recover_the_truth(dev):
    """Noise-free float32 views, wrong ids planted in half of them: test_gpu_calib.test_4096_views_recover_the_truth's gates
    (float32 image points move the least-squares solution by well under 1e-6 relative).  No host run at this size."""
    kps, truth, poses = planted_views(205, 1024, 0.0)
    d = calib.calibrate_charuco_ransac_device(kps, *BOARD, SIZE)
    planted = sum(int((~t).sum()) for t in truth)
    kept = sum(int((m & ~t).sum()) for m, t in zip(d.inliers, truth))
    lost = sum(int((t & ~m).sum()) for m, t in zip(d.inliers, truth))
    print(f"1024 views: rms {d.rms:.3g}, solves {d.solves}, stable {d.stable}, views used {d.views_used}, planted rows {planted}, "
          f"of them kept {kept}, true rows left out {lost}")
    assert d.status == calib.CALIB_OK and planted > 1000
    assert np.abs(d.camera_matrix - K_TRUE).max() <= 1e-5 * 400
    assert np.abs(d.dist_coeffs.ravel() - DIST_TRUE).max() <= 1e-5
    used = d.view_status == pnp.PNP_OK
    assert used.sum() == d.views_used >= 1000
    assert np.all(np.linalg.norm(d.rvecs - poses[:, :3], axis=1)[used] <= 1e-5 * np.linalg.norm(poses[:, :3], axis=1)[used])
    assert np.all(np.linalg.norm(d.tvecs - poses[:, 3:], axis=1)[used] <= 1e-5 * np.linalg.norm(poses[:, 3:], axis=1)[used])


def test_device_errors(dev):
    _, imgs, ids_l, _ = make_views(206, 4)
    kps = keypoints(imgs, ids_l)
    bad = [k.copy() for k in kps]
    bad[2][0, 2] = 49
    with pytest.raises(IndexError):
        calib.calibrate_charuco_ransac_device(bad, *BOARD, SIZE)
    for kw in (dict(iterations=0), dict(iterations=4097), dict(consensus_error=0.0), dict(reproj_error=float("nan")),
               dict(rounds=9), dict(rounds=-1)):
        with pytest.raises(ValueError):
            calib.calibrate_charuco_ransac_device(kps, *BOARD, SIZE, **kw)
    with pytest.raises(ValueError):
        calib.calibrate_charuco_ransac_device(kps, *BOARD, (0, 240))
    with pytest.raises(ValueError):
        calib.calibrate_charuco_ransac_device([], *BOARD, SIZE)
    r = calib.calibrate_charuco_ransac_device([k[:3] for k in kps], *BOARD, SIZE)
    assert r.status == calib.CALIB_NO_VIEWS and (r.view_status == pnp.PNP_TOO_FEW).all() and r.rms == 0.0 and r.solves == 1
    # two views that share slots are refused before anything is written
    packed, b, pool = corner_pool.pack_keypoints(kps, dev)
    packed[b + 1] -= 2                                                   # view 1 starts inside view 0
    inl = torch.full((pool,), 7, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.DcxError) as e:
        calib.calibrate_charuco_ransac_pool(packed, b, pool, True, *BOARD, SIZE, out_inliers=inl)
    assert e.value.code == -1 and (inl == 7).all()
    with pytest.raises(ValueError):
        calib.calibrate_charuco_ransac_pool(packed, b, pool, True, *BOARD, SIZE, out_inliers=inl[:pool - 1])
    with pytest.raises(ValueError):
        calib.calibrate_charuco_ransac_pool(packed.float(), b, pool, True, *BOARD, SIZE)
