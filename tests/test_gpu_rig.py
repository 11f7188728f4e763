"""The device rig calibration (csrc/dcx_rig.hip through deepcharuco_amd/rig.py) against its host definition
rig_calibrate_host_full, on the C-camera scenes of tests/rig_exact.py.

The gates are test_gpu_stereo's, unchanged: 1e-9 relative in every T_c and in the P_t translations, rotations as
max |R_dev - R_host| <= 1e-9; where the last LM steps are decided by rounding (two exact implementations may stop a step apart)
1e-6 with an equal cost, and every test prints how many scenes took that fallback.  The discrete outputs (statuses, the tree,
timestamps used, points used, row counts) must be equal; before comparing, the host definition's own margin to every discrete
decision is asserted (>= 1e-6).  The host definition is the module as shipped, run in full for every case."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import camera_exact as cx
import pool_cases
import rig_exact as rx
import stereo_exact as sx
from deepcharuco_amd import _lib, corner_pool, pnp, rig, stereo
from guarded import Arena, Guarded
from test_gpu_stereo import FALLBACK, FELL, MARGIN, OK, REL, _same_bits
from test_rig_host import CHAIN4, FAN3, FAN4, RANSAC, disconnected_scene, planted_scene

pytestmark = pytest.mark.gpu

CAMS8 = dict(angles=tuple(np.linspace(-35, 35, 8).tolist()), cams=("A", "B", "C", "A4") * 2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _host(s, **kw):
    return rig.rig_calibrate_host_full(s.kps, *s.board, *rx.cam_args(s), with_margin=True, **kw)


def _device(s, **kw):
    return rig.rig_calibrate_device(s.kps, *s.board, *rx.cam_args(s), **kw)


def _agree(d, h, name, noise_free=False):
    """Device against host -> OK or FELL (the stopping-rule fallback).  Discrete outputs first."""
    assert d.view_status.tolist() == h.view_status.tolist(), name
    assert (d.status, d.stamps_used, d.points_used) == (h.status, h.stamps_used, h.points_used), name
    assert d.parents.tolist() == h.parents.tolist(), name
    assert d.view_points.tolist() == h.view_points.tolist() and d.stamp_points.tolist() == h.stamp_points.tolist(), name
    assert h.status == rig.RIG_OK, name
    usable = h.view_status == pnp.PNP_OK
    used = np.flatnonzero(usable.sum(1) >= 2)
    part = usable & (usable.sum(1) >= 2)[:, None]
    out = np.setdiff1d(np.arange(len(h.view_status)), used)
    assert not d.rvecs[out].any() and not d.tvecs[out].any() and not d.stamp_rms[out].any() and not d.view_rms[~part].any(), name
    assert np.array_equal(d.R[0], np.eye(3)) and not d.T[0].any()
    g = {"R": float(np.abs(d.R - h.R).max()),
         "T": float(np.max(np.linalg.norm(d.T[1:] - h.T[1:], axis=1) / np.linalg.norm(h.T[1:], axis=1))),
         "P rot": max(cx.rot_gap(d.rvecs[t], h.rvecs[t]) for t in used),
         "P t": float(np.max(np.linalg.norm(d.tvecs[used] - h.tvecs[used], axis=1) / np.linalg.norm(h.tvecs[used], axis=1))),
         "rms": abs(d.rms - h.rms) / h.rms}
    worst = max(g["R"], g["T"], g["P rot"], g["P t"])
    print(f"{name}: device - host gaps {g}; steps / attempts device {d.iterations} / {d.attempts}, host {h.iterations} / "
          f"{h.attempts}")
    if worst <= REL:
        vr = np.abs(d.view_rms - h.view_rms)                 # (absolute, as test_gpu_stereo: a noise-free view's rms is ~5e-6 px)
        assert vr.max() <= REL * 400, (name, vr.max())
        return OK
    assert worst <= FALLBACK, (name, g)
    assert abs(d.rms - h.rms) <= max(1e-12 * h.rms, 1e-12 if noise_free else 0.0), (name, g, d.rms, h.rms)
    return FELL


def _compare(s, name, noise_free=False, **kw):
    h, margin = _host(s, **kw)
    assert margin >= MARGIN, (name, margin)
    return _agree(_device(s, **kw), h, name, noise_free), h


# ------------------------------------------------------------------------------------------------ device against host

CLASSES = {
    "fan3": lambda seed, sigma: rx.scene(seed, 6, sigma=sigma, **FAN3),
    "fan4 24x17": lambda seed, sigma: rx.scene(seed, 6, board=sx.BOARD_L, sigma=sigma, **FAN4),
    "chain4": lambda seed, sigma: rx.scene(seed, 6, visible=rx.chain_visibility(4, 2), sigma=sigma, **CHAIN4),
    "two": lambda seed, sigma: rx.scene(seed, 6, (0, 30), ("A", "B"), sigma=sigma),
    "eight": lambda seed, sigma: rx.scene(seed, 6, rows=8, sigma=sigma, **CAMS8),
}


@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_device_matches_host(dev, cls, sigma):
    """Six scenes per class (rig x cameras x board x noise); no class below 5 of 6 within 1e-9."""
    tally = [0, 0]
    for seed in range(6):
        s = CLASSES[cls](20 + seed, sigma)
        tally[_compare(s, f"{s.tag} #{seed}", noise_free=not sigma)[0]] += 1
    print(f"{cls} sigma {sigma}: within 1e-9 / stopping-rule fallback: {tally}")
    assert tally[OK] >= 5


@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_row_counts_at_the_evaluate_stride(dev, sigma):
    """24x17 board, rows per view spread over three cameras: 4, 5, one short of / exactly / one past the evaluate loop's 64-row
    stride, and two strides plus one."""
    rows = [(4, 129, 65), (5, 65, 129), (63, 64, 4), (64, 63, 5), (65, 5, 63), (129, 4, 64)]
    s = rx.scene(31, len(rows), board=sx.BOARD_L, sigma=sigma, rows=[list(r) for r in rows], **FAN3)
    assert [tuple(len(s.kps[c][t]) for c in range(3)) for t in range(len(rows))] == rows
    fell, h = _compare(s, f"row counts sigma {sigma}", noise_free=not sigma)
    print("row counts: stopping-rule fallback taken:", fell)
    assert h.stamps_used == len(rows) and h.view_points.tolist() == [list(r) for r in rows]


def _fan_ins():
    src = open(os.path.join(os.path.dirname(rig.__file__), "csrc", "dcx_rig.hip")).read()
    chunk = int(re.search(r"constexpr int kChunk = (\d+);", src).group(1))
    slices = int(re.search(r"constexpr int kSlices = (\d+);", src).group(1))
    return chunk, slices


def test_the_fan_ins_are_the_kernels():
    assert _fan_ins() == (rig.REDUCE_CHUNK, rig.REDUCE_SLICES) == (16, 16)


C, CS = rig.REDUCE_CHUNK, rig.REDUCE_CHUNK * rig.REDUCE_SLICES


@pytest.fixture(scope="module")
def many_stamps():
    """257 noisy timestamps of three cameras, 8 rows per view: one past kChunk * kSlices."""
    return rx.scene(41, CS + 1, sigma=0.3, rows=8, **FAN3)


@pytest.mark.parametrize("n", [1, 2, C - 1, C, C + 1, CS - 1, CS, CS + 1])
def test_timestamp_counts_at_the_reduction_fan_ins(dev, many_stamps, n):
    """1, 2, and one short of / exactly / one past kChunk (timestamps per first-level block) and kChunk * kSlices (where a
    second-level slice starts to sum two blocks): prefixes of one scene, each solved from scratch."""
    fell, h = _compare(rx.prefix(many_stamps, n), f"{n} timestamps")
    print(f"{n} timestamps: stopping-rule fallback taken:", fell)
    assert h.stamps_used == n


def test_sparse_timestamps(dev):
    """Timestamps where only cameras 1 and 2 are usable next to ones where all three are (and one where only 0 and 2 are): a camera
    missing from a timestamp must contribute exact zeros to that timestamp's Schur part and to the sums over the timestamps."""
    vis = np.array([[1, 1, 1], [0, 1, 1], [1, 1, 1], [0, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], bool)
    for sigma in (0.0, 0.3):
        s = rx.scene(45, 8, visible=vis, sigma=sigma, rows=12, **FAN3)
        fell, h = _compare(s, f"sparse timestamps sigma {sigma}", noise_free=not sigma)
        print("sparse timestamps: stopping-rule fallback taken:", fell)
        assert h.stamps_used == 8 and (h.view_status == pnp.PNP_OK).tolist() == vis.tolist()


def test_a_rejected_step_is_retried(dev):
    """The smallest rig the kernels take beyond a pair, 3 timestamps of 8 rows per view and three cameras, at which the host
    definition alone rejects steps: the device must report rejected steps too, so the retry launch (Schur, the two reductions,
    trial and decide without an evaluate, more damping) has run, and still meet this file's gates."""
    s = rx.scene(300, 3, sigma=0.3, rows=8, **FAN3)
    h, margin = _host(s)
    assert margin >= MARGIN and h.status == rig.RIG_OK and h.stamps_used == 3 and h.view_points.tolist() == [[8, 8, 8]] * 3
    assert h.attempts > h.iterations                                        # a condition on the input
    d = _device(s)
    assert d.attempts > d.iterations, (d.iterations, d.attempts)
    print("3 timestamps of 8 rows: stopping-rule fallback taken:", _agree(d, h, "3 timestamps of 8 rows"))


def _zero_outputs(d):
    for x in (d.R, d.T, d.rvec, d.rvecs, d.tvecs, d.stamp_rms, d.stamp_points, d.view_rms):
        assert not x.any()
    assert (d.rms, d.iterations, d.attempts) == (0.0, 0, 0)


def test_no_stamps_and_disconnected(dev):
    s = rx.scene(4, 3, rows=9, **FAN3)
    none = np.zeros((0, 3))
    kps = [[s.kps[0][0], none, none], [none, s.kps[1][1], none], [none, none, s.kps[2][2][:3]]]
    d = rig.rig_calibrate_device(kps, *s.board, *rx.cam_args(s))
    h = rig.rig_calibrate_host_full(kps, *s.board, *rx.cam_args(s))
    assert d.status == h.status == rig.RIG_NO_STAMPS and d.parents.tolist() == h.parents.tolist() == [-1, -1, -1]
    assert d.view_status.tolist() == h.view_status.tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 1]]
    assert d.view_points.tolist() == h.view_points.tolist() == [[9, 0, 0], [0, 9, 0], [0, 0, 3]]
    assert (d.stamps_used, d.points_used) == (h.stamps_used, h.points_used) == (0, 0)
    _zero_outputs(d)
    s = disconnected_scene()
    d, h = _device(s), _host(s)[0]
    assert d.status == h.status == rig.RIG_DISCONNECTED and d.parents.tolist() == h.parents.tolist() == [-1, 0, -1]
    assert d.view_status.tolist() == h.view_status.tolist() and d.view_points.tolist() == h.view_points.tolist()
    assert (d.stamps_used, d.points_used) == (h.stamps_used, h.points_used) == (3, 60)
    _zero_outputs(d)


# ------------------------------------------------------------------------------------------------ repeatability, masks

def test_null_and_all_ones_masks_give_the_same_bits(dev):
    s = rx.scene(51, 9, board=sx.BOARD_L, sigma=0.3, rows=[[70, 20, 33]] * 9, **FAN3)
    plain = _device(s)
    ones = [[np.ones(n, bool)] * 9 for n in (70, 20, 33)]
    assert plain.status == rig.RIG_OK
    for masks in (ones, [ones[0], None, None], [None, ones[1], ones[2]]):
        _same_bits(_device(s, masks=masks), plain)


def test_two_calls_give_the_same_bits(dev):
    s = rx.scene(52, 70, sigma=0.3, rows=12, **FAN4)
    a, b = _device(s), _device(s)
    assert a.status == rig.RIG_OK and a.stamps_used == 70
    _same_bits(a, b)


def test_masks_made_on_the_device_compose(dev):
    """The planted-exchange scene of test_rig_host: each pool's mask comes from solve_pnp_ransac_pool on the device and goes straight
    into rig_calibrate_pools; the host's come from solve_pnp_ransac_host_full."""
    s, good = planted_scene()
    cameras, dists = rx.cam_args(s)
    packs, dmasks, hmasks = [], [], [[], [], []]
    for c in range(3):
        packed, b, pool = corner_pool.pack_keypoints(s.kps[c], dev)
        st, _, info, inl = pnp.solve_pnp_ransac_pool(packed, b, pool, True, *s.board, cameras[c], dists[c], **RANSAC)
        assert (st.cpu().numpy() == pnp.PNP_OK).all()
        packs.append((packed, pool))
        dmasks.append(inl)
        for kp in s.kps[c]:
            hs, _, m, _, margin = pnp.solve_pnp_ransac_host_full(kp, *s.board, cameras[c], dists[c], with_margin=True, **RANSAC)
            assert hs == pnp.PNP_OK and margin >= MARGIN
            hmasks[c].append(m)
        assert all(np.array_equal(m, g) for m, g in zip(hmasks[c], good[c]))
    d = rig.rig_calibrate_pools([p[0] for p in packs], 6, [p[1] for p in packs], True, *s.board, cameras, dists, masks=dmasks)
    h, margin = _host(s, masks=hmasks)
    assert margin >= MARGIN
    _agree(d, h, "device masks")
    assert (d.view_points == 16).all() and d.points_used == 6 * 48
    # a mask that leaves 3 rows: the timestamp stays, on its two other views
    short = [m.copy() for m in hmasks[1]]
    short[2][:] = False
    short[2][np.argsort(s.kps[1][2][:, 2])[:3]] = True
    m3 = [hmasks[0], short, hmasks[2]]
    d3, (h3, _) = _device(s, masks=m3), _host(s, masks=m3)
    assert d3.view_status[2].tolist() == [pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_OK] and d3.view_points[2, 1] == 3 and d3.stamps_used == 6
    _agree(d3, h3, "3-row mask")


# ------------------------------------------------------------------------------------------------ the pool form

def _hand_built_pool(kps, pool, seed, gap=3):
    """Views id-sorted, in scrambled pool order with gaps between them -> packed int32 (counts | starts | rows | xy)."""
    packed, owned = pool_cases.lay_frames(kps, pool, np.random.default_rng(seed).permutation(len(kps)), gap=gap, first=2, filler=-9,
                                          id_sorted=True)
    assert owned.sum() == sum(len(k) for k in kps)                      # every view fits
    return packed


@pytest.mark.parametrize("refined", [True, False])
def test_pool_form_reads_hand_built_pools_in_place(dev, refined):
    s = rx.scene(61, 7, sigma=0.3, rows=[[30, 11, 17]] * 3 + [[8, 60, 9]] * 4, **FAN3)
    kps = [list(k) for k in s.kps]
    kps[0][5] = kps[0][5][:3]                                            # TOO_FEW
    kps[1][1] = np.zeros((0, 3))                                         # not seen by camera 1
    pools = [2 + sum(len(k) + 3 for k in kps[c]) + extra for c, extra in enumerate((17, 5, 0))]
    packed = [torch.from_numpy(_hand_built_pool(kps[c], pools[c], 1 + c)).to(dev) for c in range(3)]
    d = rig.rig_calibrate_pools(packed, 7, pools, refined, *s.board, *rx.cam_args(s))
    if not refined:                      # the integer rows are the image points
        kps = [[np.c_[np.rint(k[:, :2]), k[:, 2]] for k in kl] for kl in kps]
    lists = rig.rig_calibrate_device(kps, *s.board, *rx.cam_args(s))
    assert d.view_status[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 0] and d.view_status[:, 1].tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert d.status == rig.RIG_OK and d.stamps_used == 7
    _same_bits(d, lists)                 # the same rows in the same order at other slots: the same numbers
    h = rig.rig_calibrate_host_full(kps, *s.board, *rx.cam_args(s))
    _agree(d, h, f"hand-built pools refined={refined}")


def test_pool_form_reports_views_outside_the_pool(dev):
    """A view that starts before the pool and one cut by the pool's end are TRUNCATED and their slots are not read: everything
    else is rig_calibrate_host_full's answer with those two views empty (which the host calls TOO_FEW)."""
    s = rx.scene(62, 3, sigma=0.3, rows=12, **FAN3)
    pool = 2 + 3 * (12 + 3)
    packed = [_hand_built_pool(s.kps[c], pool, 1 + c) for c in range(3)]
    packed[0][3 + 1] = -1                # starts[1] of camera 0: a negative start
    packed[1][3 + 2] = pool - 11         # starts[2] of camera 1: its 12 rows end one slot past the pool
    d = rig.rig_calibrate_pools([torch.from_numpy(p).to(dev) for p in packed], 3, [pool] * 3, True, *s.board, *rx.cam_args(s))
    none = np.zeros((0, 3))
    kps = [[s.kps[0][0], none, s.kps[0][2]], [s.kps[1][0], s.kps[1][1], none], list(s.kps[2])]
    h = rig.rig_calibrate_host_full(kps, *s.board, *rx.cam_args(s))
    exp = np.zeros((3, 3), np.int32)
    exp[1, 0] = exp[2, 1] = pnp.PNP_TRUNCATED
    assert d.view_status.tolist() == exp.tolist() and d.stamps_used == 3
    assert h.view_status.tolist() == np.where(exp == 0, 0, pnp.PNP_TOO_FEW).tolist()
    _agree(d._replace(view_status=h.view_status), h, "views outside the pool")


def test_two_cameras_are_the_stereo_solver(dev):
    for sigma in (0.0, 0.3):
        s = rx.scene(63, 6, (0, 30), ("A", "B"), sigma=sigma)
        d = _device(s)
        st = stereo.stereo_calibrate_device(s.kps[0], s.kps[1], *s.board, *sx.cam("A"), *sx.cam("B"))
        g = {"R": float(np.abs(d.R[1] - st.R).max()), "T": float(np.linalg.norm(d.T[1] - st.T) / np.linalg.norm(st.T)),
             "P rot": max(cx.rot_gap(a, b) for a, b in zip(d.rvecs, st.rvecs)),
             "P t": float(np.max(np.linalg.norm(d.tvecs - st.tvecs, axis=1) / np.linalg.norm(st.tvecs, axis=1))),
             "rms": abs(d.rms - st.rms) / st.rms}
        print(f"C = 2 sigma {sigma}: rig - stereo on the device {g}; steps rig {d.iterations} / {d.attempts}, stereo "
              f"{st.iterations} / {st.attempts}")
        assert (d.status, d.stamps_used, d.points_used) == (st.status, st.pairs_used, st.points_used) == (0, 6, st.points_used)
        assert d.view_status.tolist() == st.view_status.tolist() and d.stamp_points.tolist() == st.pair_points.tolist()
        assert max(g["R"], g["T"], g["P rot"], g["P t"]) <= REL


# ------------------------------------------------------------------------------------------------ the C ABI, raw

def _table(packed, batch, pools, cameras, dists, masks=None):
    t = (rig._RigCamera * len(packed))()
    for c, p in enumerate(packed):
        cam9, d8, nd = pnp._camera_args(cameras[c], dists[c])
        t[c] = rig._RigCamera(*corner_pool.ptrs(p.data_ptr(), batch, pools[c])[:4], pools[c],
                              None if masks is None or masks[c] is None else masks[c].data_ptr(), cam9, d8, nd)
    return t


def test_memory_contract(dev):
    """dcx_rig_calibrate_pool, raw, on guarded buffers: the workspace is exactly dcx_rig_calibrate_workspace_bytes, between guards,
    8-byte and not 16-byte aligned, and holds in turn zeros, another call's leftovers, 0x7F bytes and 0xFF bytes; the three output
    buffers are guarded and prefilled.  Same output bits every time, every guard intact.  The scene leaves a view to each check
    (TOO_FEW, BAD_ID) and one timestamp without camera 0, so the reductions run over views that wrote nothing."""
    L = _lib.lib()
    vis = np.ones((8, 3), bool)
    vis[3, 0] = False
    s = rx.scene(64, 8, visible=vis, sigma=0.3, rows=10, **FAN3)
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[0][5] = kps[0][5][:3]
    kps[1][1][4, 2] = cx.n_ids(s.board)
    cameras, dists = rx.cam_args(s)
    B = 8
    pools = [2 + sum(len(k) + 3 for k in kps[c]) + 5 for c in range(3)]
    packed = [torch.from_numpy(_hand_built_pool(kps[c], pools[c], 1 + c)).to(dev) for c in range(3)]
    table = _table(packed, B, pools, cameras, dists)
    s2 = rx.scene(65, 20, sigma=0.3, rows=9, **FAN4)                     # the other call: four cameras, 20 timestamps
    cam2, dist2 = rx.cam_args(s2)
    packs2 = [corner_pool.pack_keypoints(k, dev) for k in s2.kps]
    pools2 = [p[2] for p in packs2]
    table2 = _table([p[0] for p in packs2], 20, pools2, cam2, dist2)
    need = L.dcx_rig_calibrate_workspace_bytes(3, B, (ctypes.c_int * 3)(*pools))
    need2 = L.dcx_rig_calibrate_workspace_bytes(4, 20, (ctypes.c_int * 4)(*pools2))
    assert 0 < need < need2 and need == rig.workspace_bytes(3, B, pools)
    stream = torch.cuda.current_stream().cuda_stream

    def run(ws_ptr):
        st, pose, info = Guarded(dev, (B, 3), torch.int32, -77), Guarded(dev, (B, 8), torch.float64, -7.5), \
            Guarded(dev, (B, 3, 2), torch.float64, -7.5)
        res, par = (ctypes.c_double * 20)(*([-7.5] * 20)), (ctypes.c_int32 * 3)(9, 9, 9)
        assert L.dcx_rig_calibrate_pool(3, table, B, *s.board, ws_ptr, need, st.ptr, pose.ptr, info.ptr, par, res, stream) == 0
        torch.cuda.synchronize()
        assert st.guard_ok() and pose.guard_ok() and info.guard_ok()
        return st.cpu().copy(), pose.cpu().copy(), info.cpu().copy(), np.array(res[:]), np.array(par[:])

    first = None
    for pattern in ("zeros", "leftovers", b"\x7f", b"\xff"):
        if pattern == "leftovers":
            big = Arena(need2, dev, align=16, offset=8)
            tmp = torch.zeros(20 * 4 * 4 + 20 * 8, dtype=torch.float64, device=dev)
            r2, p2 = (ctypes.c_double * 26)(), (ctypes.c_int32 * 4)()
            assert L.dcx_rig_calibrate_pool(4, table2, 20, *s2.board, big.ptr, need2, tmp.data_ptr(), tmp[80:].data_ptr(),
                                            tmp[240:].data_ptr(), p2, r2, stream) == 0
            torch.cuda.synchronize()
            assert int(r2[5]) == rig.RIG_OK and int(r2[3]) == 20 and big.guards_ok() is None
            ws = Arena(need, dev, align=16, offset=8)
            ws.body.copy_(big.body[:need])
        else:
            ws = Arena(need, dev, align=16, offset=8, body=b"\x00" if pattern == "zeros" else pattern)
        got = run(ws.ptr)
        assert ws.guards_ok() is None, (pattern, ws.guards_ok())
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), pattern
    st, pose, info, r, par = first
    exp = np.zeros((B, 3), np.int32)
    exp[3, 0], exp[5, 0], exp[1, 1] = pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID
    assert st.tolist() == exp.tolist() and par.tolist() == [-1, 0, 0]
    assert int(r[5]) == rig.RIG_OK and int(r[3]) == 8 and r[6] == 0 and r[7] == 0
    X = r[8:].reshape(2, 6)
    rvec, T = np.zeros((3, 3)), np.zeros((3, 3))
    rvec[1:], T[1:] = X[:, :3], X[:, 3:]
    d = rig.RigResult(int(r[5]), float(r[0]), np.stack([pnp._rodrigues(v) for v in rvec]), T, rvec, par.astype(np.int32), st,
                      info[:, :, 1].astype(np.int64), info[:, :, 0].copy(), pose[:, :3].copy(), pose[:, 3:6].copy(), pose[:, 6].copy(),
                      pose[:, 7].astype(np.int64), int(r[1]), int(r[2]), int(r[3]), int(r[4]))
    h = rig.rig_calibrate_host_full(kps, *s.board, cameras, dists)
    _agree(d, h, "dcx_rig_calibrate_pool on guarded buffers")


def test_device_argument_errors(dev):
    L = _lib.lib()
    s = rx.scene(1, 3, rows=9, **FAN3)
    cameras, dists = rx.cam_args(s)
    bad = [list(k) for k in s.kps]
    bad[1][1] = bad[1][1].copy()
    bad[1][1][0, 2] = cx.n_ids(s.board)
    with pytest.raises(IndexError):
        rig.rig_calibrate_device(bad, *s.board, cameras, dists)
    with pytest.raises(ValueError):
        rig.rig_calibrate_device(s.kps[:1], *s.board, cameras[:1], dists[:1])
    with pytest.raises(ValueError):
        rig.rig_calibrate_device([s.kps[0]] * 9, *s.board, [cameras[0]] * 9, None)
    with pytest.raises(ValueError):
        rig.rig_calibrate_device([s.kps[0], s.kps[1][:2], s.kps[2]], *s.board, cameras, dists)
    with pytest.raises(ValueError):
        rig.rig_calibrate_device([[], [], []], *s.board, cameras, dists)
    packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
    packed, pools = [p[0] for p in packs], [p[2] for p in packs]
    with pytest.raises(ValueError):                                      # pools on two devices
        rig.rig_calibrate_pools([packed[0], packed[1].cpu(), packed[2]], 3, pools, True, *s.board, cameras, dists)
    assert rig.workspace_bytes(3, 3, pools) > 0
    for n_cams, p in ((1, pools[:1]), (9, [pools[0]] * 9), (3, [27, -1, 27])):
        assert L.dcx_rig_calibrate_workspace_bytes(n_cams, 3, (ctypes.c_int * len(p))(*p)) == 0
        with pytest.raises(ValueError):
            rig.workspace_bytes(n_cams, 3, p)
    with pytest.raises(ValueError):
        rig.workspace_bytes(3, 0, pools)
    # the entry point itself
    need = rig.workspace_bytes(3, 3, pools)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=dev)
    st, pose, info = (torch.zeros(3 * 3, dtype=torch.int32, device=dev), torch.zeros(3 * 8, dtype=torch.float64, device=dev),
                      torch.zeros(3 * 3 * 2, dtype=torch.float64, device=dev))
    res, par = (ctypes.c_double * 62)(), (ctypes.c_int32 * 9)()
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_cams, table, nbytes):
        return L.dcx_rig_calibrate_pool(n_cams, table, 3, *s.board, ws.data_ptr(), nbytes, st.data_ptr(), pose.data_ptr(),
                                        info.data_ptr(), par, res, stream)
    table = _table(packed, 3, pools, cameras, dists)
    assert call(3, table, need) == 0 and int(res[5]) == rig.RIG_OK
    assert call(1, table, need) == -1                                    # DCX_E_ARG
    nine = _table([packed[0]] * 9, 3, [pools[0]] * 9, [cameras[0]] * 9, [None] * 9)
    assert call(9, nine, need) == -1
    assert call(3, table, need - 8) == -3                                # DCX_E_WS
    # a masked pool whose views share slots: found on the device
    overlap = packed[1].clone()
    overlap[3 + 1] = 4                                                   # starts[1] of camera 1 inside view 0's slots
    mask = torch.ones(pools[1], dtype=torch.uint8, device=dev)
    assert call(3, _table([packed[0], overlap, packed[2]], 3, pools, cameras, dists, [None, mask, None]), need) == -1
    with pytest.raises(_lib.DcxError):
        rig.rig_calibrate_pools([packed[0], overlap, packed[2]], 3, pools, True, *s.board, cameras, dists, masks=[None, mask, None])
