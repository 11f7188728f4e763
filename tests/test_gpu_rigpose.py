"""The device rig pose solve (csrc/dcx_rigpose.hip through deepcharuco_amd/rig.py) against its host definition rig_pose_host_full,
on the C-camera scenes of tests/rig_exact.py and tests/fisheye_rig_exact.py with the scene's true rig held fixed.

The gates are test_gpu_stereo's, as test_gpu_rig applies them: the discrete outputs (status, seed, rows, view status, view rows)
must be equal, after the host definition's own margin to every discrete decision is asserted (>= 1e-6); the poses within 1e-9
(rotations as max |R_dev - R_host|, translations relative); where the last LM step is decided by rounding (two exact
implementations may stop a step apart) 1e-6 with an equal cost, and every test prints how many scenes took that fallback."""
import ctypes

import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_rig_exact as frx
import pool_cases
import rig_exact as rx
import rigpose_exact as px
import stereo_exact as sx
from deepcharuco_amd import _lib, corner_pool, pnp, rig
from guarded import Arena, Guarded
from test_fisheye_rig_host import CLASSES as MIXED
from test_gpu_stereo import FALLBACK, FELL, MARGIN, OK, REL, _same_bits
from test_rig_host import CHAIN4, FAN3, FAN4, RANSAC, planted_scene

pytestmark = pytest.mark.gpu

CAMS8 = dict(angles=tuple(np.linspace(-35, 35, 8).tolist()), cams=("A", "B", "C", "A4") * 2)
E_ARG, E_WS = -1, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _host(s, **kw):
    a, m = rx.entry_args(s)
    return rig.rig_pose_host_full(s.kps, *s.board, *a, px.rig_rt(s.X), with_margin=True, **m, **kw)


def _device(s, **kw):
    a, m = rx.entry_args(s)
    return rig.rig_pose_device(s.kps, *s.board, *a, px.rig_rt(s.X), **m, **kw)


def _agree(d, h, name, noise_free=False):
    """Device against host -> OK or FELL (the stopping-rule fallback).  Discrete outputs first."""
    for f in ("status", "seed", "rows", "view_status", "view_points"):
        assert getattr(d, f).tolist() == getattr(h, f).tolist(), (name, f, getattr(d, f).tolist(), getattr(h, f).tolist())
    ok = np.flatnonzero(h.status == pnp.PNP_OK)
    out = np.setdiff1d(np.arange(len(h.status)), ok)
    for x in (d.rvec, d.tvec, d.rms, d.iterations, d.view_rms):
        assert not x[out].any(), name
    assert not d.view_rms[h.view_rms == 0].any(), name
    if not ok.size:
        return OK
    g = {"P rot": max(cx.rot_gap(d.rvec[t], h.rvec[t]) for t in ok),
         "P t": float(np.max(np.linalg.norm(d.tvec[ok] - h.tvec[ok], axis=1) / np.linalg.norm(h.tvec[ok], axis=1))),
         "rms": float(np.max(np.abs(d.rms[ok] - h.rms[ok]) / np.maximum(h.rms[ok], 1e-300)))}
    worst = max(g["P rot"], g["P t"])
    print(f"{name}: device - host gaps {g}; steps device {d.iterations.tolist()}, host {h.iterations.tolist()}")
    if worst <= REL:
        vr = np.abs(d.view_rms - h.view_rms)                 # (absolute, as test_gpu_stereo: a noise-free view's rms is ~5e-6 px)
        assert vr.max() <= REL * 400, (name, vr.max())
        return OK
    assert worst <= FALLBACK, (name, g)
    assert (np.abs(d.rms[ok] - h.rms[ok]) <= np.maximum(1e-12 * h.rms[ok], 1e-12 if noise_free else 0.0)).all(), (name, g)
    return FELL


def _compare(s, name, noise_free=False, **kw):
    h, margin = _host(s, **kw)
    assert margin >= MARGIN, (name, margin)
    return _agree(_device(s, **kw), h, name, noise_free), h


# ------------------------------------------------------------------------------------------------ device against host

# Every timestamp is a Levenberg-Marquardt solve of its own, and a scene takes the stopping-rule fallback if ANY of its timestamps
# does: under pnp's rules a last step of ~1e-9 |p| whose cost equals the previous one to rounding is taken by one implementation
# and damped away (lg up to 16) by the other.  test_gpu_rig's "5 of 6 scenes" counts one solve per scene, so the scenes here hold
# two timestamps (two blocks of the grid; the chain three, one per link), not six: with six, a first run on an MI355X had 5 of 36
# noisy scenes fall back, one or two timestamps each of 216, which put the eight-camera class at 4 of 6.  The row-count, status and
# mask tests below compare scenes of six to eight timestamps under the same gates.
CLASSES = {
    "fan3": lambda seed, sigma: rx.scene(seed, 2, sigma=sigma, **FAN3),
    "fan4 24x17": lambda seed, sigma: rx.scene(seed, 2, board=sx.BOARD_L, sigma=sigma, **FAN4),
    # every view of the chain holds the whole board, as test_rig_host.chain_scene's do and for its reason: a P_t there rests on the
    # two views of its own timestamp alone
    "chain4": lambda seed, sigma: rx.scene(seed, 3, visible=rx.chain_visibility(4, 1), sigma=sigma, rows=cx.n_ids(sx.BOARD_S), **CHAIN4),
    "two": lambda seed, sigma: rx.scene(seed, 2, (0, 30), ("A", "B"), sigma=sigma),
    "eight": lambda seed, sigma: rx.scene(seed, 2, rows=8, sigma=sigma, **CAMS8),
    "mixed fan3 F/P/F": lambda seed, sigma: frx.scene(seed, 2, sigma=sigma, **MIXED["fan3 F/P/F"]),
}


@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_device_matches_host(dev, cls, sigma):
    """Six scenes per class (rig x cameras x board x noise); no class below 5 of 6 within 1e-9."""
    tally = [0, 0]
    for seed in range(6):
        s = CLASSES[cls](20 + seed, sigma)
        fell, h = _compare(s, f"{s.tag} #{seed}", noise_free=not sigma)
        assert (h.status == pnp.PNP_OK).all()
        tally[fell] += 1
    print(f"{cls} sigma {sigma}: within 1e-9 / stopping-rule fallback: {tally}")
    assert tally[OK] >= 5


ROWS = [(1, 129, 65), (2, 65, 129), (3, 64, 63), (4, 129, 1), (5, 63, 2), (63, 3, 64), (64, 5, 129), (65, 4, 3)]


@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_row_counts_at_the_wave_stride(dev, sigma):
    """24x17 board, rows per view spread over three cameras: 1, 2, 3 (views that cannot stand alone), 4, 5, one short of / exactly /
    one past the joint evaluate's 64-lane stride, and two strides plus one."""
    s = rx.scene(31, len(ROWS), board=sx.BOARD_L, sigma=sigma, rows=[list(r) for r in ROWS], **FAN3)
    assert [tuple(len(s.kps[c][t]) for c in range(3)) for t in range(len(ROWS))] == ROWS
    fell, h = _compare(s, f"row counts sigma {sigma}", noise_free=not sigma)
    print("row counts: stopping-rule fallback taken:", fell)
    assert (h.status == pnp.PNP_OK).all() and h.rows.tolist() == [sum(r) for r in ROWS] and h.view_points.tolist() == [list(r) for r in ROWS]
    assert (h.view_status == np.where(np.array(ROWS) < 4, pnp.PNP_TOO_FEW, pnp.PNP_OK)).all() and (h.view_rms > 0).all()


def test_statuses_and_views_that_cannot_stand_alone(dev):
    """No seed, a bad id in a 2-row view, an empty camera, five collinear rows, all of it next to timestamps that are fine."""
    s = rx.scene(33, 6, sigma=0.3, rows=[[20, 2, 3], [3, 2, 1], [12, 2, 9], [12, 0, 9], [12, 5, 9], [12, 9, 10]], **FAN3)
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[1][2][1, 2] = cx.n_ids(s.board)                                  # the 2-row view of timestamp 2: an id outside the board
    kps[1][3] = np.zeros((0, 3))
    rm1 = s.board[1] - 1
    ids = np.arange(5) * rm1 + 2                                         # one board row: collinear
    kps[1][4] = np.c_[cx.f64(sx.project_rig(cx.board_points(ids, *s.board), s.P[4], s.X[0], *sx.cam("B"))).astype(np.float32), ids]
    s = s._replace(kps=kps)
    h, margin = _host(s)
    assert margin >= MARGIN
    few, deg = pnp.PNP_TOO_FEW, pnp.PNP_DEGENERATE
    assert h.status.tolist() == [0, few, 0, 0, 0, 0] and h.seed.tolist() == [0, -1] + h.seed[2:].tolist()
    assert h.view_status.tolist() == [[0, few, few], [few, few, few], [0, few, 0], [0, few, 0], [0, deg, 0], [0, 0, 0]]
    assert h.rows.tolist() == [25, 6, 21, 21, 26, 31] and h.view_rms[2, 1] == 0 and h.view_rms[4, 1] > 0 and h.view_rms[0, 2] > 0
    print("statuses: stopping-rule fallback taken:", _agree(_device(s), h, "statuses"))


# ------------------------------------------------------------------------------------------------ repeatability, masks

def test_null_and_all_ones_masks_give_the_same_bits(dev):
    s = rx.scene(51, 8, board=sx.BOARD_L, sigma=0.3, rows=[[70, 20, 3]] * 8, **FAN3)
    plain = _device(s)
    ones = [[np.ones(n, bool)] * 8 for n in (70, 20, 3)]
    assert (plain.status == pnp.PNP_OK).all()
    for masks in (ones, [ones[0], None, None], [None, ones[1], ones[2]]):
        _same_bits(_device(s, masks=masks), plain)


def test_a_mask_that_drops_rows_equals_the_host_with_the_same_mask(dev):
    s = rx.scene(53, 6, sigma=0.3, rows=[[20, 12, 9]] * 6, **FAN3)
    rng = np.random.default_rng(8)
    masks = [[rng.random(n) < 0.7 for _ in range(6)] for n in (20, 12, 9)]
    masks[1][2][:] = False
    masks[1][2][:2] = True                                               # two rows left: still a constraint
    masks[2][4][:] = False                                               # none left
    fell, h = _compare(s, "dropping masks", masks=masks)
    print("dropping masks: stopping-rule fallback taken:", fell)
    assert h.view_points.tolist() == [[int(masks[c][t].sum()) for c in range(3)] for t in range(6)]
    assert h.view_points[2, 1] == 2 and h.view_points[4, 2] == 0 and (h.status == pnp.PNP_OK).all()


def test_masks_made_on_the_device_compose(dev):
    """The planted-exchange scene of test_rig_host: each pool's mask comes from solve_pnp_ransac_pool on the device and goes straight
    into rig_pose_pools; the host's come from solve_pnp_ransac_host_full."""
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
    d = rig.unpack_rig_poses(*rig.rig_pose_pools([p[0] for p in packs], 6, [p[1] for p in packs], True, *s.board, cameras, dists,
                                                 px.rig_rt(s.X), masks=dmasks))
    h, margin = _host(s, masks=hmasks)
    assert margin >= MARGIN
    _agree(d, h, "device masks")
    assert (d.view_points == 16).all() and (d.rows == 48).all() and (d.status == pnp.PNP_OK).all()


def test_two_calls_give_the_same_bits(dev):
    s = rx.scene(52, 8, sigma=0.3, rows=12, **FAN4)
    a, b = _device(s), _device(s)
    assert (a.status == pnp.PNP_OK).all()
    _same_bits(a, b)


def test_graph_capture_and_replay_on_pools_rewritten_in_place(dev):
    """The call captured once with its workspace and outputs preallocated, replayed after the pools were overwritten in place with
    another scene's: bit for bit the eager call on that scene."""
    one, two = rx.scene(54, 6, sigma=0.3, rows=[[14, 9, 3]] * 6, **FAN3), rx.scene(55, 6, sigma=0.3, rows=[[14, 9, 3]] * 6, **FAN3)
    cameras, dists = rx.cam_args(one)
    R, T = px.rig_rt(one.X)
    p1 = [corner_pool.pack_keypoints(k, dev) for k in one.kps]
    p2 = [corner_pool.pack_keypoints(k, dev) for k in two.kps]
    pools = [p[2] for p in p1]
    assert pools == [p[2] for p in p2]
    call = lambda packed, **kw: rig.rig_pose_pools(packed, 6, pools, True, *one.board, cameras, dists, (R, T), **kw)   # noqa: E731
    eager1 = rig.unpack_rig_poses(*call([p[0] for p in p1]))
    eager2 = rig.unpack_rig_poses(*call([p[0] for p in p2]))
    live = [p[0].clone() for p in p1]
    ws = torch.empty(rig.rig_pose_workspace_bytes(3, 6, pools), dtype=torch.uint8, device=dev)
    out = rig.rig_pose_pools(live, 6, pools, True, *one.board, cameras, dists, (R, T), workspace=ws)      # warm-up, allocates `out`
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(live, workspace=ws, out=out)
    for x in out:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(rig.unpack_rig_poses(*out), eager1)
    for a, b in zip(live, p2):
        a.copy_(b[0])
    graph.replay()
    torch.cuda.synchronize()
    replayed = rig.unpack_rig_poses(*out)
    _same_bits(replayed, eager2)
    assert (replayed.status == pnp.PNP_OK).all() and not np.array_equal(eager1.tvec, eager2.tvec)


# ------------------------------------------------------------------------------------------------ the C ABI, raw

def _hand_built_pool(kps, pool, seed, gap=3):
    """Views id-sorted, in scrambled pool order with gaps between them -> packed int32 (counts | starts | rows | xy)."""
    packed, owned = pool_cases.lay_frames(kps, pool, np.random.default_rng(seed).permutation(len(kps)), gap=gap, first=2, filler=-9,
                                          id_sorted=True)
    assert owned.sum() == sum(len(k) for k in kps)                      # every view fits
    return packed


def _table(packed, batch, pools, cameras, dists, masks=None):
    t = (rig._RigCamera * len(packed))()
    for c, p in enumerate(packed):
        cam9, d8, nd = pnp._camera_args(cameras[c], dists[c])
        t[c] = rig._RigCamera(*corner_pool.ptrs(p.data_ptr(), batch, pools[c])[:4], pools[c],
                              None if masks is None or masks[c] is None else masks[c].data_ptr(), cam9, d8, nd)
    return t


def _x(s):
    return (ctypes.c_double * s.X.size)(*s.X.ravel().tolist())


def test_memory_contract(dev):
    """dcx_rig_pose_pool, raw, on guarded buffers: the workspace is exactly dcx_rig_pose_workspace_bytes, between guards, 8-byte and
    not 16-byte aligned, and holds in turn zeros, another call's leftovers, 0x7F bytes and 0xFF bytes; the six output buffers are
    guarded and prefilled.  Same output bits every time, every guard intact.  The scene leaves a view to each check (TOO_FEW with
    rows, BAD_ID, TRUNCATED) and a timestamp without camera 0; camera 1 has a mask of ones, so its index lists are written."""
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
    host_packed = [_hand_built_pool(kps[c], pools[c], 1 + c) for c in range(3)]
    host_packed[2][B + 6] = pools[2] - 4                                 # starts[6] of camera 2: its rows end past the pool
    packed = [torch.from_numpy(p).to(dev) for p in host_packed]
    ones = torch.ones(pools[1], dtype=torch.uint8, device=dev)
    table = _table(packed, B, pools, cameras, dists, [None, ones, None])
    s2 = rx.scene(65, 20, sigma=0.3, rows=9, **FAN4)                     # the other call: four cameras, 20 timestamps
    cam2, dist2 = rx.cam_args(s2)
    packs2 = [corner_pool.pack_keypoints(k, dev) for k in s2.kps]
    pools2 = [p[2] for p in packs2]
    table2 = _table([p[0] for p in packs2], 20, pools2, cam2, dist2)
    need = L.dcx_rig_pose_workspace_bytes(3, B, (ctypes.c_int * 3)(*pools))
    need2 = L.dcx_rig_pose_workspace_bytes(4, 20, (ctypes.c_int * 4)(*pools2))
    assert 0 < need < need2 and need == rig.rig_pose_workspace_bytes(3, B, pools)
    stream = torch.cuda.current_stream().cuda_stream

    def outputs(b, c):
        return (Guarded(dev, (2,), torch.int32, -77), Guarded(dev, (b,), torch.int32, -77), Guarded(dev, (b, 8), torch.float64, -7.5),
                Guarded(dev, (b, 2), torch.int32, -77), Guarded(dev, (b, c), torch.int32, -77), Guarded(dev, (b, c, 2), torch.float64, -7.5))

    def run(ws_ptr):
        o = outputs(B, 3)
        assert L.dcx_rig_pose_pool(3, table, None, _x(s), B, *s.board, ws_ptr, need, *(g.ptr for g in o), stream) == 0
        torch.cuda.synchronize()
        assert all(g.guard_ok() for g in o)
        return [g.cpu().copy() for g in o]

    first = None
    for pattern in ("zeros", "leftovers", b"\x7f", b"\xff"):
        if pattern == "leftovers":
            big = Arena(need2, dev, align=16, offset=8)
            o2 = outputs(20, 4)
            assert L.dcx_rig_pose_pool(4, table2, None, _x(s2), 20, *s2.board, big.ptr, need2, *(g.ptr for g in o2), stream) == 0
            torch.cuda.synchronize()
            assert (o2[1].cpu() == pnp.PNP_OK).all() and big.guards_ok() is None
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
    d = rig.unpack_rig_poses(*first)
    none = np.zeros((0, 3))
    hk = [list(k) for k in kps]
    hk[2][6] = none                                                      # the host has no pool to cut a view: it is empty there
    h, margin = rig.rig_pose_host_full(hk, *s.board, cameras, dists, px.rig_rt(s.X), with_margin=True)
    assert margin >= MARGIN and first[0].tolist() == [0, 0]
    exp = np.zeros((B, 3), np.int32)
    exp[3, 0], exp[5, 0], exp[1, 1], exp[6, 2] = pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_TRUNCATED
    assert d.view_status.tolist() == exp.tolist() and d.view_points[6, 2] == 0 and d.rows.tolist() == [30, 20, 30, 20, 30, 23, 20, 30]
    assert h.view_status[6, 2] == pnp.PNP_TOO_FEW
    _agree(d._replace(view_status=h.view_status), h, "dcx_rig_pose_pool on guarded buffers")


def test_refusals(dev):
    """DCX_E_ARG for what dcx_rig_calibrate_models_pool refuses and for a rig that is not finite; DCX_E_WS; overlapping slot ranges
    under a mask are found on the device and raise DcxError when the result is unpacked."""
    L = _lib.lib()
    s = rx.scene(1, 3, rows=9, **FAN3)
    cameras, dists = rx.cam_args(s)
    R, T = px.rig_rt(s.X)
    packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
    packed, pools = [p[0] for p in packs], [p[2] for p in packs]
    need = rig.rig_pose_workspace_bytes(3, 3, pools)
    for n_cams, p in ((1, pools[:1]), (9, [pools[0]] * 9), (3, [27, -1, 27])):
        assert L.dcx_rig_pose_workspace_bytes(n_cams, 3, (ctypes.c_int * len(p))(*p)) == 0
        with pytest.raises(ValueError):
            rig.rig_pose_workspace_bytes(n_cams, 3, p)
    with pytest.raises(ValueError):
        rig.rig_pose_workspace_bytes(3, 0, pools)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=dev)
    outs = rig._pose_outputs(None, 3, 9, dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_cams, table, nbytes, x=None, models=None, board=s.board, ws_ptr=None, outs=outs):
        x = _x(s) if x is None else (ctypes.c_double * len(x))(*x)
        m = None if models is None else (ctypes.c_int * len(models))(*models)
        return L.dcx_rig_pose_pool(n_cams, table, m, x, 3, *board, ws.data_ptr() if ws_ptr is None else ws_ptr, nbytes,
                                   *(None if o is None else o.data_ptr() for o in outs), stream)
    table = _table(packed, 3, pools, cameras, dists)
    assert call(3, table, need) == 0
    torch.cuda.synchronize()
    assert (outs[1][:3].cpu().numpy() == pnp.PNP_OK).all()
    assert call(1, table, need) == E_ARG and call(9, _table([packed[0]] * 9, 3, [pools[0]] * 9, [cameras[0]] * 9, [None] * 9), need) == E_ARG
    assert call(3, None, need) == E_ARG
    assert call(3, table, need - 8) == E_WS
    assert call(3, table, need, ws_ptr=ws.data_ptr() + 4) == E_ARG       # the workspace is not 8-byte aligned
    for i in range(6):
        assert call(3, table, need, outs=outs[:i] + (None,) + outs[i + 1:]) == E_ARG
    x = s.X.ravel().tolist()
    for bad in (float("nan"), float("inf")):
        assert call(3, table, need, x=x[:7] + [bad] + x[8:]) == E_ARG
    assert L.dcx_rig_pose_pool(3, table, None, None, 3, *s.board, ws.data_ptr(), need, *(o.data_ptr() for o in outs), stream) == E_ARG
    assert call(3, table, need, models=[0, 2, 0]) == E_ARG               # an unknown model
    assert call(3, table, need, models=[0, 1, 0]) == E_ARG               # a fisheye camera with five coefficients (camera B)
    assert call(3, table, need, models=[0, 0, 0]) == 0
    assert call(3, table, need, board=(1, s.board[1], s.board[2])) == E_ARG
    assert call(3, table, need, board=(s.board[0], s.board[1], float("nan"))) == E_ARG
    skewed = _table(packed, 3, pools, cameras, dists)
    skewed[2].camera9[1] = 0.5
    assert call(3, skewed, need) == E_ARG                                # a camera with skew
    # the Python layer
    with pytest.raises(ValueError):
        rig.rig_pose_device(s.kps, *s.board, cameras, dists, (R[:2], T[:2]))            # a rig of two for three cameras
    with pytest.raises(ValueError):
        rig.rig_pose_device(s.kps, *s.board, cameras, dists, (R * np.array([1, np.nan, 1])[:, None, None], T))
    with pytest.raises(ValueError):
        rig.rig_pose_device([s.kps[0], s.kps[1][:2], s.kps[2]], *s.board, cameras, dists, (R, T))
    with pytest.raises(ValueError):
        rig.rig_pose_pools([packed[0], packed[1].cpu(), packed[2]], 3, pools, True, *s.board, cameras, dists, (R, T))
    with pytest.raises(ValueError):
        rig.rig_pose_pools(packed, 3, pools, True, *s.board, cameras, dists, (R, T), workspace=ws[:4])
    failed = rig.rig_calibrate_host_full([[k[:3] for k in kl] for kl in s.kps], *s.board, cameras, dists)
    assert failed.status == rig.RIG_NO_STAMPS
    with pytest.raises(ValueError):
        rig.rig_pose_pools(packed, 3, pools, True, *s.board, cameras, dists, failed)
    # a masked pool whose views share slots: found on the device, reported in d_head and raised when unpacked
    overlap = packed[1].clone()
    overlap[3 + 1] = 4                                                   # starts[1] of camera 1 inside view 0's slots
    mask = torch.ones(pools[1], dtype=torch.uint8, device=dev)
    got = rig.rig_pose_pools([packed[0], overlap, packed[2]], 3, pools, True, *s.board, cameras, dists, (R, T), masks=[None, mask, None])
    head, status, pose, info, vst, vinfo = (g.cpu().numpy() for g in got)
    assert head.tolist() == [1, 0] and (status == pnp.PNP_TRUNCATED).all() and (vst == pnp.PNP_TRUNCATED).all()
    assert not pose.any() and not vinfo.any() and info.tolist() == [[-1, 0]] * 3
    with pytest.raises(_lib.DcxError):
        rig.unpack_rig_poses(*got)
    fine = rig.unpack_rig_poses(*rig.rig_pose_pools(packed, 3, pools, True, *s.board, cameras, dists, (R, T), masks=[None, mask, None]))
    assert (fine.status == pnp.PNP_OK).all()
