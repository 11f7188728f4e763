"""The device stereo calibration (csrc/dcx_stereo.hip through deepcharuco_amd/stereo.py) against its host definition
stereo_calibrate_host_full, on the two-camera scenes of tests/stereo_exact.py.

The gates are DESIGN 3.8's, unchanged: 1e-9 relative in T and in the P_t translations, rotations as max |R_dev - R_host| <= 1e-9;
where the last LM steps are decided by rounding (two exact implementations may stop a step apart) 1e-6 with an equal cost, and
every test prints how many scenes took that fallback.  The discrete outputs (statuses, pairs used, points used, row counts)
must be equal; before comparing, the host definition's own margin to every discrete decision is asserted (>= 1e-6).

The host definition is the module as shipped, run in full for every case (the pair-count cases are prefixes of one scene, each
solved from scratch); nothing in it is patched or cached."""
import os
import re

import numpy as np
import pytest
import torch

import camera_exact as cx
import pool_cases
import stereo_exact as sx
from deepcharuco_amd import calib, corner_pool, pnp, stereo
from stereo_exact import FALLBACK, MARGIN, REL

pytestmark = pytest.mark.gpu

OK, FELL = 0, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _host(s, sl=slice(None), **kw):
    return stereo.stereo_calibrate_host_full(s.kps0[sl], s.kps1[sl], *s.board, *sx.cam_args(s), with_margin=True, **kw)


def _device(s, sl=slice(None), **kw):
    return stereo.stereo_calibrate_device(s.kps0[sl], s.kps1[sl], *s.board, *sx.cam_args(s), **kw)


def _agree(d, h, name, noise_free=False):
    """Device against host -> OK or FELL (the stopping-rule fallback).  Discrete outputs first."""
    assert d.view_status.tolist() == h.view_status.tolist(), name
    assert (d.status, d.pairs_used, d.points_used) == (h.status, h.pairs_used, h.points_used), name
    assert d.view_points.tolist() == h.view_points.tolist() and d.pair_points.tolist() == h.pair_points.tolist(), name
    assert h.status == stereo.STEREO_OK, name
    used = np.flatnonzero((h.view_status == pnp.PNP_OK).all(1))
    out = np.setdiff1d(np.arange(len(h.view_status)), used)
    assert not d.rvecs[out].any() and not d.tvecs[out].any() and not d.pair_rms[out].any() and not d.view_rms[out].any(), name
    g = {"R": float(np.abs(d.R - h.R).max()), "T": float(np.linalg.norm(d.T - h.T) / np.linalg.norm(h.T)),
         "P rot": max(cx.rot_gap(d.rvecs[t], h.rvecs[t]) for t in used),
         "P t": float(np.max(np.linalg.norm(d.tvecs[used] - h.tvecs[used], axis=1) / np.linalg.norm(h.tvecs[used], axis=1))),
         "rms": abs(d.rms - h.rms) / h.rms}
    worst = max(g["R"], g["T"], g["P rot"], g["P t"])
    print(f"{name}: device - host gaps {g}; steps / attempts device {d.iterations} / {d.attempts}, host {h.iterations} / "
          f"{h.attempts}")
    if worst <= REL:
        # a pose gap of 1e-9 (relative) moves a projected point by at most 1e-9 of the image's extent (< 400 px here), and a
        # view's rms by no more than its points: an absolute gate, because a noise-free view's rms is ~5e-6 px
        vr = np.abs(d.view_rms[used] - h.view_rms[used])
        assert vr.max() <= REL * 400, (name, vr.max())
        return OK
    # the fallback: 1e-6 and an equal cost.  Noise-free float32 scenes: the rms (~5e-6 px) is a sum of differences of ~300 px
    # values, whose fp64 rounding is ~1e-8 of it, so there the equal-cost gate is test_gpu_calib's absolute 1e-12 px
    assert worst <= FALLBACK, (name, g)
    assert abs(d.rms - h.rms) <= max(1e-12 * h.rms, 1e-12 if noise_free else 0.0), (name, g, d.rms, h.rms)
    return FELL


def _compare(s, name, sl=slice(None), noise_free=False, **kw):
    h, margin = _host(s, sl, **kw)
    assert margin >= MARGIN, (name, margin)
    return _agree(_device(s, sl, **kw), h, name, noise_free), h


# ------------------------------------------------------------------------------------------------ device against host

@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("rig,c0,c1,board", [("small", "A", "B", sx.BOARD_S), ("toe90", "B", "C", sx.BOARD_L),
                                              ("r170", "C", "A", sx.BOARD_S)])
def test_device_matches_host(dev, rig, c0, c1, board, sigma):
    """Six scenes per class (rig x cameras x board x noise); no class below 5 of 6 within 1e-9."""
    tally = [0, 0]
    for seed in range(6):
        s = sx.scene(20 + seed, 6, rig, board, c0, c1, sigma=sigma)
        tally[_compare(s, f"{s.tag} #{seed}", noise_free=not sigma)[0]] += 1
    print(f"{rig} {c0}/{c1} sigma {sigma}: within 1e-9 / stopping-rule fallback: {tally}")
    assert tally[OK] >= 5


@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_row_counts_at_the_evaluate_stride(dev, sigma):
    """24x17 board, rows per view chosen independently for the two cameras: 4, 5, one short of / exactly / one past the evaluate
    loop's 64-row stride, and two strides plus one."""
    rows = [(4, 129), (5, 65), (63, 64), (64, 63), (65, 5), (129, 4), (64, 64), (129, 129)]
    s = sx.scene(31, len(rows), "toe90", sx.BOARD_L, "B", "C", sigma=sigma, rows=rows)
    assert [(len(a), len(b)) for a, b in zip(s.kps0, s.kps1)] == rows
    fell, h = _compare(s, f"row counts sigma {sigma}", noise_free=not sigma)
    print("row counts: stopping-rule fallback taken:", fell)
    assert h.pairs_used == len(rows) and h.view_points.tolist() == [list(r) for r in rows]


def test_a_rejected_step_is_retried(dev):
    """The smallest scene the kernels take, 3 pairs of 8 rows per view, with a seed at which the host definition alone rejects
    steps (9 accepted steps in 24 attempts): the device must report rejected steps too, so the retry launch (Schur, the two
    reductions, trial and decide without an evaluate, more damping) has run, and still meet this file's gates."""
    s = sx.scene(300, 3, "small", sx.BOARD_S, "A", "B", sigma=0.3, rows=8)
    h, margin = _host(s)
    assert margin >= MARGIN and h.status == stereo.STEREO_OK and h.pairs_used == 3 and h.view_points.tolist() == [[8, 8]] * 3
    assert h.attempts > h.iterations                                        # a condition on the input
    d = _device(s)
    assert d.attempts > d.iterations, (d.iterations, d.attempts)
    print("3 pairs of 8 rows: stopping-rule fallback taken:", _agree(d, h, "3 pairs of 8 rows"))


def _fan_ins():
    src = open(os.path.join(os.path.dirname(stereo.__file__), "csrc", "dcx_stereo.hip")).read()
    chunk = int(re.search(r"constexpr int kChunk = (\d+);", src).group(1))
    slices = int(re.search(r"constexpr int kSlices = (\d+);", src).group(1))
    return chunk, slices


def test_the_fan_ins_are_the_kernels():
    assert _fan_ins() == (stereo.REDUCE_CHUNK, stereo.REDUCE_SLICES) == (16, 16)


@pytest.fixture(scope="module")
def many_pairs():
    """257 noisy pairs of 8 rows per view: one past kChunk * kSlices."""
    return sx.scene(41, stereo.REDUCE_CHUNK * stereo.REDUCE_SLICES + 1, "small", sx.BOARD_S, "A", "B", sigma=0.3, rows=8)


C, CS = stereo.REDUCE_CHUNK, stereo.REDUCE_CHUNK * stereo.REDUCE_SLICES


@pytest.mark.parametrize("n", [1, 2, C - 1, C, C + 1, CS - 1, CS, CS + 1])
def test_pair_counts_at_the_reduction_fan_ins(dev, many_pairs, n):
    """1, 2, and one short of / exactly / one past kChunk (timestamps per first-level block) and kChunk * kSlices (where a
    second-level slice starts to sum two blocks)."""
    fell, h = _compare(many_pairs, f"{n} pairs", slice(0, n))
    print(f"{n} pairs: stopping-rule fallback taken:", fell)
    assert h.pairs_used == n


def test_no_pairs(dev):
    s = sx.scene(4, 3, "small", sx.BOARD_S, "A", "B", rows=9)
    kps0 = [s.kps0[0][:3], s.kps0[1], np.zeros((0, 3))]
    kps1 = [s.kps1[0], np.zeros((0, 3)), s.kps1[2]]
    d = stereo.stereo_calibrate_device(kps0, kps1, *s.board, *sx.cam_args(s))
    h = stereo.stereo_calibrate_host_full(kps0, kps1, *s.board, *sx.cam_args(s))
    assert d.status == h.status == stereo.STEREO_NO_PAIRS
    assert d.view_status.tolist() == h.view_status.tolist() == [[1, 0], [0, 1], [1, 0]]
    assert d.view_points.tolist() == h.view_points.tolist() == [[3, 9], [9, 0], [0, 9]]
    for x in (d.R, d.T, d.rvec, d.E, d.F, d.rvecs, d.tvecs, d.pair_rms, d.pair_points, d.view_rms):
        assert not x.any()
    assert (d.rms, d.iterations, d.attempts, d.pairs_used, d.points_used) == (0.0, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ masks

def test_masks_made_on_the_device_compose(dev):
    """The planted-exchange scene of test_stereo_host: each pool's mask comes from solve_pnp_ransac_pool on the device and goes
    straight into stereo_calibrate_pool; the host's come from solve_pnp_ransac_host_full."""
    from test_stereo_host import RANSAC, planted_scene
    s, good = planted_scene()
    cams = (sx.cam(s.cam0), sx.cam(s.cam1))
    packs, dmasks, hmasks = [], [], ([], [])
    for c, kps in enumerate((s.kps0, s.kps1)):
        packed, b, pool = corner_pool.pack_keypoints(kps, dev)
        st, _, info, inl = pnp.solve_pnp_ransac_pool(packed, b, pool, True, *s.board, *cams[c], **RANSAC)
        assert (st.cpu().numpy() == pnp.PNP_OK).all()
        packs.append((packed, pool))
        dmasks.append(inl)
        for kp in kps:
            hs, _, m, _, margin = pnp.solve_pnp_ransac_host_full(kp, *s.board, *cams[c], with_margin=True, **RANSAC)
            assert hs == pnp.PNP_OK and margin >= MARGIN
            hmasks[c].append(m)
        assert all(np.array_equal(m, g) for m, g in zip(hmasks[c], good[c]))
    d = stereo.stereo_calibrate_pool(packs[0][0], packs[1][0], 6, packs[0][1], packs[1][1], True, *s.board, *sx.cam_args(s),
                                     masks=tuple(dmasks))
    h, margin = _host(s, masks=hmasks)
    assert margin >= MARGIN
    _agree(d, h, "device masks")
    assert (d.view_points == 16).all() and d.points_used == 6 * 32
    # a mask that leaves 3 rows
    short = [m.copy() for m in hmasks[1]]
    short[2][:] = False
    short[2][np.argsort(s.kps1[2][:, 2])[:3]] = True
    d3 = _device(s, masks=(hmasks[0], short))
    h3, _ = _host(s, masks=(hmasks[0], short))
    assert d3.view_status[2].tolist() == [pnp.PNP_OK, pnp.PNP_TOO_FEW] and d3.view_points[2, 1] == 3 and d3.pairs_used == 5
    _agree(d3, h3, "3-row mask")


def _same_bits(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def test_null_and_all_ones_masks_give_the_same_bits(dev):
    s = sx.scene(51, 9, "toe90", sx.BOARD_L, "A", "B", sigma=0.3, rows=[(70, 20)] * 9)
    plain = _device(s)
    ones0, ones1 = [np.ones(70, bool)] * 9, [np.ones(20, bool)] * 9
    assert plain.status == stereo.STEREO_OK
    for masks in ((ones0, ones1), (ones0, None), (None, ones1)):
        _same_bits(_device(s, masks=masks), plain)


def test_two_calls_give_the_same_bits(dev):
    s = sx.scene(52, 70, "small", sx.BOARD_S, "A", "B", sigma=0.3, rows=12)
    a, b = _device(s), _device(s)
    assert a.status == stereo.STEREO_OK and a.pairs_used == 70
    _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ the pool form

def _hand_built_pool(kps, pool, seed, gap=3):
    """Views id-sorted, in scrambled pool order with gaps between them -> packed int32 (counts | starts | rows | xy)."""
    packed, owned = pool_cases.lay_frames(kps, pool, np.random.default_rng(seed).permutation(len(kps)), gap=gap, first=2, filler=-9,
                                          id_sorted=True)
    assert owned.sum() == sum(len(k) for k in kps)                      # every view fits
    return packed


@pytest.mark.parametrize("refined", [True, False])
def test_pool_form_reads_two_hand_built_pools_in_place(dev, refined):
    s = sx.scene(61, 7, "toe90", sx.BOARD_S, "A", "B", sigma=0.3, rows=[(30, 11)] * 3 + [(8, 60)] * 4)
    kps0, kps1 = list(s.kps0), list(s.kps1)
    kps0[5] = kps0[5][:3]                                                # TOO_FEW
    kps1[1] = np.zeros((0, 3))                                           # seen by camera 0 only
    pool0, pool1 = 2 + sum(len(k) + 3 for k in kps0) + 17, 2 + sum(len(k) + 3 for k in kps1) + 5
    p0, p1 = _hand_built_pool(kps0, pool0, 1), _hand_built_pool(kps1, pool1, 2)
    d = stereo.stereo_calibrate_pool(torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev), 7, pool0, pool1, refined, *s.board,
                                     *sx.cam_args(s))
    if not refined:                      # the integer rows are the image points
        kps0, kps1 = [np.c_[np.rint(k[:, :2]), k[:, 2]] for k in kps0], [np.c_[np.rint(k[:, :2]), k[:, 2]] for k in kps1]
    lists = stereo.stereo_calibrate_device(kps0, kps1, *s.board, *sx.cam_args(s))
    assert d.view_status[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 0] and d.view_status[:, 1].tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert d.status == stereo.STEREO_OK and d.pairs_used == 5
    _same_bits(d, lists)                 # the same rows in the same order at other slots: the same numbers
    h = stereo.stereo_calibrate_host_full(kps0, kps1, *s.board, *sx.cam_args(s))
    _agree(d, h, f"hand-built pools refined={refined}")


def test_pool_form_reports_views_outside_the_pool(dev):
    """A view that starts before the pool and one cut by the pool's end are TRUNCATED and their slots are not read: everything
    else is stereo_calibrate_host_full's answer with those two views empty (which the host calls TOO_FEW)."""
    s = sx.scene(62, 2, "small", sx.BOARD_S, "A", "B", sigma=0.3, rows=12)
    pool = 2 + 2 * (12 + 3)
    p0, p1 = _hand_built_pool(s.kps0, pool, 1), _hand_built_pool(s.kps1, pool, 2)
    p0[2 + 1] = -1                       # starts[1] of camera 0: a negative start
    p1[2 + 1] = pool - 11                # starts[1] of camera 1: its 12 rows end one slot past the pool
    d = stereo.stereo_calibrate_pool(torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev), 2, pool, pool, True, *s.board,
                                     *sx.cam_args(s))
    none = np.zeros((0, 3))
    h = stereo.stereo_calibrate_host_full([s.kps0[0], none], [s.kps1[0], none], *s.board, *sx.cam_args(s))
    assert h.view_status.tolist() == [[pnp.PNP_OK] * 2, [pnp.PNP_TOO_FEW] * 2]
    assert d.view_status.tolist() == [[pnp.PNP_OK] * 2, [pnp.PNP_TRUNCATED] * 2]
    assert d.pairs_used == 1
    _agree(d._replace(view_status=h.view_status), h, "views outside the pool")


def test_calibrate_then_stereo_on_the_device(dev):
    """calibrate_charuco_pool on each camera's pool, then stereo_calibrate_pool with the two solved models, from the same two
    device pools.  The rig is recovered to the accuracy the host chain (calibrate_camera_host_full twice, then
    stereo_calibrate_host_full) reaches on the same views, and the two chains agree by the gates above."""
    s = sx.scene(71, 16, "toe90", sx.BOARD_S, "A", "B")
    sizes = ((320, 240), cx.CALIB_SIZE)
    packs, models, hmodels = [], [], []
    for c, kps in enumerate((s.kps0, s.kps1)):
        packed, b, pool = corner_pool.pack_keypoints(kps, dev)
        r = calib.calibrate_charuco_pool(packed, b, pool, True, *s.board, sizes[c])
        assert r.status == calib.CALIB_OK
        packs.append((packed, pool))
        models.append((r.camera_matrix, r.dist_coeffs))
        srt = [k[np.argsort(k[:, 2], kind="stable")] for k in kps]
        hr = calib.calibrate_camera_host_full([pnp.object_points(k[:, 2], *s.board) for k in srt],
                                              [k[:, :2].astype(np.float32) for k in srt], sizes[c])
        assert hr.status == calib.CALIB_OK
        hmodels.append((hr.camera_matrix, hr.dist_coeffs))
    d = stereo.stereo_calibrate_pool(packs[0][0], packs[1][0], 16, packs[0][1], packs[1][1], True, *s.board, *models[0], *models[1])
    h = stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *hmodels[0], *hmodels[1])
    assert d.status == h.status == stereo.STEREO_OK and d.pairs_used == 16
    (dR, dT), (hR, hT) = sx.rig_error(d, s), sx.rig_error(h, s)
    print(f"calibrate -> stereo: device rig error R {dR:.3e} T {dT:.3e}; host chain R {hR:.3e} T {hT:.3e}; rms {d.rms:.3e} / {h.rms:.3e}")
    # the host chain's own accuracy, with the 1e-6 that separates two exact chains whose intrinsics agree to 1e-8
    assert dR <= hR + 1e-6 and dT <= hT + 1e-6
    assert np.abs(d.R - h.R).max() <= 1e-6 and np.linalg.norm(d.T - h.T) <= 1e-6 * np.linalg.norm(h.T)


def test_device_argument_errors(dev):
    s = sx.scene(1, 3, "small", sx.BOARD_S, "A", "B", rows=9)
    bad = [k.copy() for k in s.kps1]
    bad[1][0, 2] = cx.n_ids(s.board)
    with pytest.raises(IndexError):
        stereo.stereo_calibrate_device(s.kps0, bad, *s.board, *sx.cam_args(s))
    skew = sx.K_A.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_device(s.kps0, s.kps1, *s.board, skew, None, sx.K_B, None)
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_device(s.kps0, s.kps1[:2], *s.board, *sx.cam_args(s))
    with pytest.raises(ValueError):
        stereo.stereo_calibrate_device([], [], *s.board, *sx.cam_args(s))
    assert stereo.workspace_bytes(3, 27, 27) > 0
    with pytest.raises(ValueError):
        stereo.workspace_bytes(0, 1, 1)
