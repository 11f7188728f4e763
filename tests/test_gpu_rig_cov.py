"""dcx_rig_uncertainty_pool (csrc/dcx_rig_cov.hip) against its definition, rig.rig_uncertainty_host, on the MI355X.

The device is compared with the host definition EVALUATED AT THE DEVICE CALIBRATION'S OWN RESULT, so both sides stand at the same
(X, P) and only the order of the sums differs between them.  The gate is tests/test_rig_cov_host.py's: 1000 * cond(S) * 2^-52, with
cond(S) computed by the test from the host's cov_rig (sigma^2 S^-1 has S's condition).  Covariance entries are compared relative to
sqrt(c_ii c_jj), standard deviations relative to themselves, sigma^2 to 1e-12 relative; dof, points, stamps and the status must be
equal.  Every scene carries 0.3 px of noise (on noise-free float32 pixels the sum of squares carries 1e-8 of rounding, not 1e-12:
tests/test_gpu_calib_cov.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_rig_exact as frx
import rig_exact as rx
import stereo_exact as sx
from deepcharuco_amd import _lib, calib, corner_pool, pnp, rig, stereo
from test_calib_cov_host import _same_bits
from test_gpu_calib import STRIDE_BOARD
from test_gpu_rig import CAMS8, _hand_built_pool, _table
from test_rig_cov_host import SIGMA, _zero_but_counts, renoised, status_cases
from test_rig_host import CHAIN4, FAN3, FAN4, RANSAC, planted_scene

pytestmark = pytest.mark.gpu

REL_SIGMA2 = 1e-12
E_ARG, E_WS = -1, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _gate(h):
    return 1000.0 * float(np.linalg.cond(h.cov_rig)) * 2.0 ** -52


def _rel_cov(d, h):
    """max |d - h| / sqrt(h_ii h_jj) over the entries of [..., n, n] covariances (0 for none)."""
    s = np.sqrt(np.diagonal(h, axis1=-2, axis2=-1))
    scale = s[..., :, None] * s[..., None, :]
    return float(np.max(np.abs(d - h) / scale)) if h.size else 0.0


def _compare(d, h, name):
    """Device against host RigUncertainty at the gate of the module docstring -> the measured gaps."""
    assert (d.status, d.dof, d.points, d.stamps) == (h.status, h.dof, h.points, h.stamps), (name, d[6:], h[6:], d.status, h.status)
    assert d.status == calib.COV_OK, name
    used = np.flatnonzero(h.std_poses.any(1))
    unused = np.setdiff1d(np.arange(len(h.std_poses)), used)
    assert used.size == h.stamps and not d.cov_poses[unused].any() and not d.std_poses[unused].any(), name
    assert d.cov_rig.shape == h.cov_rig.shape and not d.std_rig[0].any() and d.baseline_std[0] == 0.0
    gate = _gate(h)
    gaps = {"sigma2": abs(d.sigma2 - h.sigma2) / h.sigma2,
            "cov_rig": _rel_cov(d.cov_rig, h.cov_rig),
            "cov_poses": _rel_cov(d.cov_poses[used], h.cov_poses[used]),
            "std_rig": float(np.max(np.abs(d.std_rig[1:] - h.std_rig[1:]) / h.std_rig[1:])),
            "std_poses": float(np.max(np.abs(d.std_poses[used] - h.std_poses[used]) / h.std_poses[used])),
            "baseline_std": float(np.max(np.abs(d.baseline_std[1:] - h.baseline_std[1:]) / h.baseline_std[1:]))}
    print(f"{name}: gate {gate:.3g}, device - host gaps {gaps}")
    assert gaps["sigma2"] <= REL_SIGMA2, (name, gaps)
    assert max(v for k, v in gaps.items() if k != "sigma2") <= gate, (name, gaps, gate)
    assert np.array_equal(d.cov_rig, d.cov_rig.T) and np.array_equal(d.cov_poses, d.cov_poses.transpose(0, 2, 1))
    return gaps


def _host(s, model, **kw):
    args, mk = rx.entry_args(s)
    return rig.rig_uncertainty_host(s.kps, *s.board, *args, model, **{**mk, **kw})


def _device(s, model, **kw):
    args, mk = rx.entry_args(s)
    return rig.rig_uncertainty_device(s.kps, *s.board, *args, model, **{**mk, **kw})


def _calibrated(s, **kw):
    """The device calibration of the scene: the point both sides are evaluated at."""
    args, mk = rx.entry_args(s)
    r = rig.rig_calibrate_device(s.kps, *s.board, *args, **{**mk, **kw})
    assert r.status == rig.RIG_OK, s.tag
    return r


def _at_device_result(s, name, **kw):
    r = _calibrated(s, **kw)
    return _compare(_device(s, r, **kw), _host(s, r, **kw), name), r


def _tuple(r, n=None, view_status=None):
    """A RigResult's first n timestamps as the explicit tuple."""
    k = slice(n)
    return r.rvec, r.T, r.rvecs[k], r.tvecs[k], (r.view_status if view_status is None else np.asarray(view_status, np.int32))[k]


# ------------------------------------------------------------------------------------------------ device against host

CLASSES = {
    "two": lambda: rx.scene(70, 6, (0, 30), ("A", "B"), sigma=SIGMA),
    "fan3": lambda: rx.scene(70, 6, sigma=SIGMA, **FAN3),
    "fan4 24x17": lambda: rx.scene(70, 6, board=sx.BOARD_L, sigma=SIGMA, **FAN4),
    "chain4": lambda: rx.scene(70, 6, visible=rx.chain_visibility(4, 2), sigma=SIGMA, **CHAIN4),
    "eight": lambda: rx.scene(70, 6, rows=8, sigma=SIGMA, **CAMS8),
    "mixed fan3 F/P/F": lambda: frx.scene(70, 6, (0, 25, -25), ("F", "P", "F0"), sigma=SIGMA),
}


@pytest.mark.parametrize("cls", list(CLASSES))
def test_device_matches_host(dev, cls):
    """C = 2, 3, 4 and 8 (n = 42, the LDS limit); the chain, whose timestamps each lack two cameras; a rig of two fisheye cameras
    and a pinhole through ``models``."""
    s = CLASSES[cls]()
    if cls.startswith("mixed"):
        assert rx.entry_args(s)[1]["models"] == ["fisheye", "pinhole", "fisheye"]
    _, r = _at_device_result(s, cls)
    assert r.stamps_used == 6


def test_row_counts_at_the_lds_chunk(dev):
    """The 130-id board, rows per view spread over three cameras: 4, one short of / exactly / one past the evaluate kernel's 64-row
    chunk, and one past two chunks."""
    rows = [(4, 129, 65), (65, 4, 129), (63, 64, 4), (64, 63, 130), (129, 65, 63), (130, 4, 64)]
    s = rx.scene(71, len(rows), board=STRIDE_BOARD, sigma=SIGMA, rows=[list(r) for r in rows], **FAN3)
    assert [tuple(len(s.kps[c][t]) for c in range(3)) for t in range(len(rows))] == rows
    _, r = _at_device_result(s, "4 / 63 / 64 / 65 / 129 / 130 rows")
    assert r.view_points.tolist() == [list(v) for v in rows]


def test_the_fan_ins_are_the_kernels():
    src = open(os.path.join(os.path.dirname(rig.__file__), "csrc", "dcx_rig_cov.hip")).read()
    chunk = int(re.search(r"constexpr int kChunk = (\d+);", src).group(1))
    slices = int(re.search(r"constexpr int kSlices = (\d+);", src).group(1))
    assert (chunk, slices) == (rig.REDUCE_COV_CHUNK, rig.REDUCE_COV_SLICES) == (16, 16)
    assert rig.RIGCOV_STRIDE == 6 * (rig.RIG_MAX_CAMERAS - 1) and rig.RIGCOV_STD == rig.RIGCOV_STRIDE ** 2
    assert rig.RIGCOV_SIGMA2 == rig.RIGCOV_STD + rig.RIGCOV_STRIDE and rig.RIGCOV_GLOBAL_WORDS == rig.RIGCOV_SIGMA2 + 6


CH, CS = rig.REDUCE_COV_CHUNK, rig.REDUCE_COV_CHUNK * rig.REDUCE_COV_SLICES
_MANY = {}


def many_stamps():
    """257 noisy timestamps of three cameras, 8 rows per view (one past kChunk * kSlices), calibrated once on the device."""
    if not _MANY:
        s = rx.scene(72, CS + 1, sigma=SIGMA, rows=8, **FAN3)
        _MANY["s"], _MANY["r"] = s, _calibrated(s)
    return _MANY["s"], _MANY["r"]


@pytest.mark.parametrize("n", [1, CH - 1, CH, CH + 1, CS - 1, CS, CS + 1])
def test_timestamp_counts_at_the_reduction_fan_ins(dev, n):
    """1, and one short of / exactly / one past kChunk (timestamps per first-level block) and kChunk * kSlices (where a slice starts
    to sum two blocks): prefixes of one scene at the 257-timestamp calibration's X and P.  (One timestamp alone leaves S with a
    large condition; the gate follows it.)"""
    s, r = many_stamps()
    sub = rx.prefix(s, n)
    h = _host(sub, _tuple(r, n))
    assert h.stamps == n and h.points == 24 * n
    _compare(_device(sub, _tuple(r, n)), h, f"{n} timestamps")


def test_1025_timestamps(dev):
    """41 timestamps laid 25 times, at the 41's calibration: the optimum of the 1,025 is the optimum of the 41."""
    s = rx.scene(73, 41, sigma=SIGMA, rows=8, **FAN3)
    r = _calibrated(s)
    big = s._replace(kps=[k * 25 for k in s.kps], P=np.tile(s.P, (25, 1)), visible=np.tile(s.visible, (25, 1)))
    model = (r.rvec, r.T, np.tile(r.rvecs, (25, 1)), np.tile(r.tvecs, (25, 1)), np.tile(r.view_status, (25, 1)))
    h = _host(big, model)
    assert h.stamps == 1025
    _compare(_device(big, model), h, "1,025 timestamps")


def test_every_view_status_between_used_timestamps(dev):
    """Eight timestamps of three cameras: a view of 3 rows and an empty view (TOO_FEW), a bad id, collinear rows (DEGENERATE), and a
    timestamp left with one usable view, between timestamps that are used."""
    s = rx.scene(74, 8, sigma=SIGMA, rows=12, **FAN3)
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[0][1] = kps[0][1][:3]                                          # TOO_FEW; the timestamp stays on cameras 1 and 2
    kps[1][2] = np.zeros((0, 3))                                       # not seen by camera 1
    kps[2][3][4, 2] = cx.n_ids(s.board)                                # BAD_ID
    line = np.arange(6) * (s.board[1] - 1)                             # one board line: collinear
    kps[1][4] = np.c_[np.linspace(40, 200, 6), np.linspace(30, 150, 6), line]
    kps[0][6], kps[1][6] = kps[0][6][:2], kps[1][6][:3]                # camera 2 alone: not used
    s = s._replace(kps=kps)
    packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]        # (the pool form: the list form raises for the bad id)
    r = rig.rig_calibrate_pools([p[0] for p in packs], 8, [p[2] for p in packs], True, *s.board, *rx.cam_args(s))
    exp = np.zeros((8, 3), np.int32)
    exp[1, 0] = exp[2, 1] = exp[6, 0] = exp[6, 1] = pnp.PNP_TOO_FEW
    exp[3, 2], exp[4, 1] = pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE
    assert r.status == rig.RIG_OK and r.view_status.tolist() == exp.tolist() and r.stamps_used == 7
    h = _host(s, r)
    assert h.stamps == 7 and h.points == r.points_used and not h.std_poses[6].any()
    _compare(_device(s, r), h, "every view status")


@pytest.mark.parametrize("refined", [True, False])
def test_pool_form_reads_hand_built_pools_in_place(dev, refined):
    """Views in scrambled pool order with gaps between them; refined xy and the integer rows."""
    s = rx.scene(75, 7, sigma=SIGMA, rows=[[30, 11, 17]] * 3 + [[8, 60, 9]] * 4, **FAN3)
    kps = [list(k) for k in s.kps]
    kps[0][5] = kps[0][5][:3]                                          # TOO_FEW
    kps[1][1] = np.zeros((0, 3))                                       # not seen by camera 1
    pools = [2 + sum(len(k) + 3 for k in kps[c]) + extra for c, extra in enumerate((17, 5, 0))]
    packed = [torch.from_numpy(_hand_built_pool(kps[c], pools[c], 1 + c)).to(dev) for c in range(3)]
    r = rig.rig_calibrate_pools(packed, 7, pools, refined, *s.board, *rx.cam_args(s))
    assert r.status == rig.RIG_OK and r.stamps_used == 7
    g, p = rig.rig_uncertainty_pools(packed, 7, pools, refined, *s.board, *rx.cam_args(s), r)
    d = rig.unpack_rig_uncertainty(g, p, r.T)
    if not refined:                                                     # the integer rows are the image points
        kps = [[np.c_[np.rint(k[:, :2]), k[:, 2]] for k in kl] for kl in kps]
    _compare(d, rig.rig_uncertainty_host(kps, *s.board, *rx.cam_args(s), r), f"hand-built pools refined={refined}")
    _same_bits(d, rig.rig_uncertainty_device(kps, *s.board, *rx.cam_args(s), r))   # the same rows at other slots


# ------------------------------------------------------------------------------------------------ masks

def _bits(dev_pair):
    return tuple(t.cpu().numpy().tobytes() for t in dev_pair)


def _pools_call(s, packs, model, **kw):
    return rig.rig_uncertainty_pools([p[0] for p in packs], packs[0][1], [p[2] for p in packs], True, *s.board, *rx.cam_args(s), model, **kw)


def test_masks_give_the_bits_of_the_compacted_pools(dev):
    s = rx.scene(76, 9, board=sx.BOARD_L, sigma=SIGMA, rows=[[70, 20, 33]] * 9, **FAN3)
    r = _calibrated(s)
    rng = np.random.default_rng(11)
    masks = [[rng.random(len(k)) < 0.8 for k in kl] for kl in s.kps]
    masks[1][3][:] = True
    assert all(m.sum() >= 6 for kl in masks for m in kl)
    order = [[np.argsort(k[:, 2], kind="stable") for k in kl] for kl in s.kps]
    packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
    cut = [corner_pool.pack_keypoints([k[m] for k, m in zip(s.kps[c], masks[c])], dev) for c in range(3)]
    by_slot = [torch.from_numpy(np.concatenate([m[o] for m, o in zip(masks[c], order[c])]).astype(np.uint8)).to(dev) for c in range(3)]
    model = _tuple(r)
    masked = _pools_call(s, packs, model, masks=by_slot)
    assert _bits(masked) == _bits(_pools_call(s, cut, model))
    u = rig.unpack_rig_uncertainty(*masked, r.T)
    assert u.status == calib.COV_OK and u.points == sum(int(m.sum()) for kl in masks for m in kl)
    _same_bits(u, _device(s, model, masks=masks))
    _compare(u, _host(s, model, masks=masks), "masked pools")
    plain = _pools_call(s, packs, model)
    ones = [torch.ones(p[2], dtype=torch.uint8, device=dev) for p in packs]
    for mk in (ones, [ones[0], None, None], [None, ones[1], ones[2]]):
        assert _bits(_pools_call(s, packs, model, masks=mk)) == _bits(plain)
    assert _bits(masked) != _bits(plain)


def test_masks_made_on_the_device_compose(dev):
    """The planted-exchange scene of test_rig_host: each pool's mask comes from solve_pnp_ransac_pool on the device and goes
    straight into the calibration and the uncertainty, which must give the bits of the call on pools without the rejected rows."""
    s, good = planted_scene()
    cameras, dists = rx.cam_args(s)
    packs, dmasks = [], []
    for c in range(3):
        packed, b, pool = corner_pool.pack_keypoints(s.kps[c], dev)
        st, _, _, inl = pnp.solve_pnp_ransac_pool(packed, b, pool, True, *s.board, cameras[c], dists[c], **RANSAC)
        assert (st.cpu().numpy() == pnp.PNP_OK).all()
        packs.append((packed, b, pool))
        dmasks.append(inl)
    r = rig.rig_calibrate_pools([p[0] for p in packs], 6, [p[2] for p in packs], True, *s.board, cameras, dists, masks=dmasks)
    assert r.status == rig.RIG_OK and (r.view_points == 16).all()
    masked = _pools_call(s, packs, r, masks=dmasks)
    cut = [corner_pool.pack_keypoints([k[m] for k, m in zip(s.kps[c], good[c])], dev) for c in range(3)]
    assert _bits(masked) == _bits(_pools_call(s, cut, r))
    d = rig.unpack_rig_uncertainty(*masked, r.T)
    assert d.points == r.points_used == 6 * 48
    _compare(d, _host(s, r, masks=good), "masks of the consensus pose solves")


# ------------------------------------------------------------------------------------------------ determinism and capture

def test_two_calls_and_a_captured_graph_give_the_same_bits(dev):
    """Captured with the process's default number of hardware queues."""
    s = rx.scene(77, 40, sigma=SIGMA, rows=12, **FAN4)
    r = _calibrated(s)
    packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
    B, pools = 40, [p[2] for p in packs]
    st = torch.from_numpy(r.view_status.astype(np.int32)).to(dev)
    pose = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    pose[:, :6] = torch.from_numpy(np.c_[r.rvecs, r.tvecs]).to(dev)
    masks = [torch.ones(p, dtype=torch.uint8, device=dev) for p in pools]
    masks[2][::7] = 0
    ws = torch.empty(rig.rig_uncertainty_workspace_bytes(4, B, pools), dtype=torch.uint8, device=dev)
    out = (torch.empty(rig.RIGCOV_GLOBAL_WORDS, dtype=torch.float64, device=dev),
           torch.empty((B, calib.COV_POSE_WORDS), dtype=torch.float64, device=dev))

    def call():
        return _pools_call(s, packs, (r.rvec, r.T, st, pose), masks=masks, workspace=ws, out=out)

    eager = _bits(call())
    assert rig.unpack_rig_uncertainty(*out, r.T).status == calib.COV_OK
    assert _bits(call()) == eager
    ws.fill_(0x7F)
    assert _bits(call()) == eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # a synchronising call would fail here
        call()
    for _ in range(2):
        out[0].fill_(-1.0)
        out[1].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(out) == eager


# ------------------------------------------------------------------------------------------------ what the numbers mean

@pytest.mark.parametrize("angles,cams", [((0, 25, -25), ("A", "B", "C")), ((0, 30), ("A", "B"))])
def test_standard_deviations_predict_the_spread_of_recalibrations(dev, angles, cams):
    """Monte-Carlo on the device: rig_exact.scene(2, 24, sigma=0.0, ...) re-noised 120 times at 0.3 px from default_rng(11), each
    draw calibrated by rig_calibrate_device; the empirical standard deviation of the 6 (C - 1) rig parameters over the draws
    against the standard deviations predicted from the first draw alone.  Every ratio in [0.80, 1.25]: a condition, not a tolerance
    (the 1-sigma sampling error of a standard deviation from 120 draws is 6.5 %, so +-3 sigma), and sigma^2 within
    +-3 sqrt(2 / dof) of 0.09.  The host definition gives 0.884 to 1.083 for the three cameras (dof 4,618) and 0.920 to 1.008 for
    the two."""
    draws, s = renoised(120, angles, cams)
    args = rx.cam_args(s)
    X, first = [], None
    for kps in draws:
        r = rig.rig_calibrate_device(kps, *s.board, *args)
        assert r.status == rig.RIG_OK and r.stamps_used == 24
        if first is None:
            first = rig.rig_uncertainty_device(kps, *s.board, *args, r)
        X.append(np.c_[r.rvec, r.T][1:].ravel())
    assert first.status == calib.COV_OK and first.dof == 2 * first.points - 6 * (len(cams) - 1) - 6 * 24
    if len(cams) == 3:
        assert first.dof == 4618
    ratios = np.std(X, axis=0, ddof=1) / first.std_rig[1:].ravel()
    half = 3.0 * np.sqrt(2.0 / first.dof)
    print(f"{len(cams)} cameras: empirical / predicted standard deviation of the rig parameters {np.round(ratios, 3).tolist()}; sigma2 "
          f"{first.sigma2:.5f} (0.09 +- {0.09 * half:.5f}), dof {first.dof}")
    assert ratios.shape == (6 * (len(cams) - 1),) and ratios.min() >= 0.80 and ratios.max() <= 1.25, ratios
    assert abs(first.sigma2 - SIGMA ** 2) <= half * SIGMA ** 2


# ------------------------------------------------------------------------------------------------ statuses and refusals

@pytest.mark.parametrize("name", list(status_cases()))
def test_statuses(dev, name):
    """tests/test_rig_cov_host.py's cases: NO_VIEWS, NO_DOF (before SINGULAR), and three ways to SINGULAR; zeros elsewhere."""
    s, model, expect = status_cases()[name]
    u = _device(s, model)
    print(f"{name}: status {u.status}, dof {u.dof}, points {u.points}, stamps {u.stamps}")
    assert (u.status, u.dof, u.points, u.stamps) == expect
    _zero_but_counts(u)
    h = _host(s, model)
    assert (h.status, h.dof, h.points, h.stamps) == expect


def test_a_failed_result_is_refused(dev):
    s = CLASSES["fan3"]()
    r = _calibrated(s)
    with pytest.raises(ValueError, match="failed"):
        _device(s, r._replace(status=rig.RIG_DISCONNECTED))


def test_a_used_view_whose_slots_leave_the_pool_is_not_read(dev):
    """A view that starts before its pool and one cut by the pool's end, both called usable: DCX_COV_SINGULAR, their rows not
    counted, zeros elsewhere."""
    s = rx.scene(78, 3, sigma=SIGMA, rows=12, **FAN3)
    pool = 2 + 3 * (12 + 3)
    packed = [_hand_built_pool(s.kps[c], pool, 1 + c) for c in range(3)]
    packed[0][3 + 1] = -1                                               # starts[1] of camera 0: a negative start
    packed[1][3 + 2] = pool - 11                                        # starts[2] of camera 1: its 12 rows end one slot past the pool
    model = (np.r_[np.zeros((1, 3)), s.X[:, :3]], np.r_[np.zeros((1, 3)), s.X[:, 3:]], s.P[:, :3], s.P[:, 3:], np.zeros((3, 3), np.int32))
    g, p = rig.rig_uncertainty_pools([torch.from_numpy(q).to(dev) for q in packed], 3, [pool] * 3, True, *s.board, *rx.cam_args(s), model)
    u = rig.unpack_rig_uncertainty(g, p, model[1])
    assert (u.status, u.stamps, u.points) == (calib.COV_SINGULAR, 3, 7 * 12)
    _zero_but_counts(u)


def test_abi_refusals(dev):
    L = _lib.lib()
    s = CLASSES["fan3"]()
    r = _calibrated(s)
    cameras, dists = rx.cam_args(s)
    packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
    packed, pools, B = [p[0] for p in packs], [p[2] for p in packs], 6
    table = _table(packed, B, pools, cameras, dists)
    hp = (ctypes.c_int * 3)(*pools)
    need = L.dcx_rig_uncertainty_workspace_bytes(3, B, hp)
    assert need == rig.rig_uncertainty_workspace_bytes(3, B, pools) > 0
    assert L.dcx_rig_uncertainty_workspace_bytes(1, B, hp) == 0 and L.dcx_rig_uncertainty_workspace_bytes(9, B, (ctypes.c_int * 9)(*([8] * 9))) == 0
    assert L.dcx_rig_uncertainty_workspace_bytes(3, 0, hp) == 0 and L.dcx_rig_uncertainty_workspace_bytes(3, B, None) == 0
    assert L.dcx_rig_uncertainty_workspace_bytes(3, B, (ctypes.c_int * 3)(8, -1, 8)) == 0
    assert need < L.dcx_rig_uncertainty_workspace_bytes(3, B + 1, hp)
    st = torch.from_numpy(r.view_status.astype(np.int32)).to(dev)
    pose = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    pose[:, :6] = torch.from_numpy(np.c_[r.rvecs, r.tvecs]).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    g = torch.full((rig.RIGCOV_GLOBAL_WORDS,), -7.0, dtype=torch.float64, device=dev)
    p = torch.full((B, calib.COV_POSE_WORDS), -7.0, dtype=torch.float64, device=dev)
    x = (ctypes.c_double * 12)(*np.c_[r.rvec, r.T][1:].ravel().tolist())
    stream = _lib.current_stream()

    def call(n_cams=3, table=table, models=None, x=x, batch=B, board=s.board, st=st.data_ptr(), pose=pose.data_ptr(), ws=ws.data_ptr(),
             nbytes=need, g=g.data_ptr(), p=p.data_ptr()):
        return L.dcx_rig_uncertainty_pool(n_cams, table, models, x, batch, *board, st, pose, ws, nbytes, g, p, stream)

    assert call(n_cams=1) == E_ARG and call(n_cams=9) == E_ARG and call(n_cams=0) == E_ARG
    assert call(batch=0) == E_ARG and call(batch=-1) == E_ARG and call(table=None) == E_ARG
    assert call(board=(1, 8, 0.02)) == E_ARG and call(models=(ctypes.c_int * 3)(0, 2, 0)) == E_ARG
    for kw in ("x", "st", "pose", "ws", "g", "p"):
        assert call(**{kw: None}) == E_ARG, kw
    assert call(nbytes=need - 1) == E_WS and call(nbytes=0) == E_WS
    torch.cuda.synchronize()
    assert bool((g == -7.0).all()) and bool((p == -7.0).all())          # a refused call writes nothing
    assert call() == 0 and call(models=(ctypes.c_int * 3)(0, 0, 0)) == 0
    torch.cuda.synchronize()
    _same_bits(rig.unpack_rig_uncertainty(g, p, r.T), _device(s, r))
    with pytest.raises(ValueError):
        _pools_call(s, packs, r, workspace=ws[:need - 8])
    with pytest.raises(ValueError):
        _pools_call(s, packs, r, masks=[torch.ones(pools[0], dtype=torch.int32, device=dev), None, None])
    with pytest.raises(ValueError):
        _pools_call(s, packs, (r.rvec, r.T, st[:3], pose))
    with pytest.raises(ValueError):
        rig.rig_uncertainty_workspace_bytes(1, B, pools[:1])


def test_the_stereo_wrappers_are_the_rig_call_with_two_cameras(dev):
    s = CLASSES["two"]()
    (k0, k1), (d0, d1) = rx.cam_args(s)
    sr = stereo.stereo_calibrate_device(s.kps[0], s.kps[1], *s.board, k0, d0, k1, d1)
    assert sr.status == stereo.STEREO_OK
    z = np.zeros((1, 3))
    model = (np.r_[z, sr.rvec[None]], np.r_[z, sr.T[None]], sr.rvecs, sr.tvecs, sr.view_status)
    d = stereo.stereo_uncertainty_device(s.kps[0], s.kps[1], *s.board, k0, d0, k1, d1, sr)
    _same_bits(d, _device(s, model))
    _compare(d, stereo.stereo_uncertainty_host(s.kps[0], s.kps[1], *s.board, k0, d0, k1, d1, sr), "stereo wrappers")
    (p0, b, n0), (p1, _, n1) = (corner_pool.pack_keypoints(k, dev) for k in s.kps)
    g, p = stereo.stereo_uncertainty_pool(p0, p1, b, n0, n1, True, *s.board, k0, d0, k1, d1, sr)
    _same_bits(rig.unpack_rig_uncertainty(g, p, model[1]), d)
    assert _bits((g, p)) == _bits(rig.rig_uncertainty_pools([p0, p1], b, [n0, n1], True, *s.board, (k0, k1), (d0, d1), model))
