"""The device rig calibration with fisheye cameras in the rig (csrc/dcx_rig.hip's mixed kernels through
dcx_rig_calibrate_models_pool and deepcharuco_amd/rig.py's ``models``) against its host definition rig_calibrate_host_full, on the
scenes of tests/fisheye_rig_exact.py and the classes of tests/test_fisheye_rig_host.py.

The gates are test_gpu_rig's (test_gpu_stereo's, imported): 1e-9, or where the last LM steps are decided by rounding 1e-6 with an
equal cost, and every test prints how often that fallback was taken; the discrete outputs must be equal, and before comparing the
host definition's own margin to every discrete decision is asserted (>= 1e-6).  The host definition is run in full for every case."""
import ctypes

import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_rig_exact as frx
import rig_exact as rx
import stereo_exact as sx
from deepcharuco_amd import _lib, corner_pool, fisheye, pnp, rig, stereo
from test_fisheye_rig_host import (CLASSES, ROWS_PX, SIZE, STEREO_PAIRS, class_scene, common_rows, on_axis_scene, outside_scene,
                                   pair_scene, stereo_args, wide_scene)
from test_gpu_rig import _agree
from test_gpu_stereo import _agree as _stereo_agree
from test_gpu_stereo import MARGIN, OK, _same_bits
from test_rig_host import FAN3 as PINHOLE_FAN3

pytestmark = pytest.mark.gpu

E_ARG = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _host(s, **kw):
    return rig.rig_calibrate_host_full(s.kps, *s.board, *frx.cam_args(s), models=frx.models(s), with_margin=True, **kw)


def _device(s, **kw):
    return rig.rig_calibrate_device(s.kps, *s.board, *frx.cam_args(s), models=frx.models(s), **kw)


def _compare(s, name, noise_free=False, **kw):
    h, margin = _host(s, **kw)
    assert margin >= MARGIN, (name, margin)
    return _agree(_device(s, **kw), h, name, noise_free), h


# ------------------------------------------------------------------------------------------------ device against host

@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_device_matches_host(dev, cls, sigma):
    """Six scenes per class; no class below 5 of 6 within 1e-9 (test_gpu_rig's cap on the stopping-rule fallback)."""
    tally = [0, 0]
    for seed in range(6):
        s = class_scene(cls, 20 + seed, sigma)
        tally[_compare(s, f"{s.tag} #{seed}", noise_free=not sigma)[0]] += 1
    print(f"{cls} sigma {sigma}: within 1e-9 / stopping-rule fallback: {tally}")
    assert tally[OK] >= 5


@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_row_counts_at_the_evaluate_stride(dev, sigma):
    """24x17 board, a fisheye, a pinhole and a fisheye camera, rows per view at 4, 5 and one short of / exactly / one past the
    evaluate loop's 64-row stride, and two strides plus one: every count meets either model."""
    rows = [(4, 129, 65), (5, 65, 129), (63, 64, 4), (64, 63, 5), (65, 5, 63), (129, 4, 64)]
    s = class_scene("fan3 F/P/F", 31, sigma, n_stamps=len(rows), board=sx.BOARD_L, rows=[list(r) for r in rows])
    assert [tuple(len(s.kps[c][t]) for c in range(3)) for t in range(len(rows))] == rows
    fell, h = _compare(s, f"row counts sigma {sigma}", noise_free=not sigma)
    print("row counts: stopping-rule fallback taken:", fell)
    assert h.stamps_used == len(rows) and h.view_points.tolist() == [list(r) for r in rows]


@pytest.fixture(scope="module")
def many_stamps():
    """257 noisy timestamps of the mixed fan, 8 rows per view: one past kChunk * kSlices."""
    return class_scene("fan3 F/P/F", 41, 0.3, n_stamps=rig.REDUCE_CHUNK * rig.REDUCE_SLICES + 1, rows=8)


@pytest.mark.parametrize("n", [1, rig.REDUCE_CHUNK + 1, rig.REDUCE_CHUNK * rig.REDUCE_SLICES + 1])
def test_timestamp_counts_past_the_reduction_fan_ins(dev, many_stamps, n):
    """1, and one past each fan-in of the reduction (the kernels that reduce never see a camera, so three counts are enough)."""
    fell, h = _compare(rx.prefix(many_stamps, n), f"{n} timestamps")
    print(f"{n} timestamps: stopping-rule fallback taken:", fell)
    assert h.stamps_used == n


# ------------------------------------------------------------------------------------------------ the model's edges

def test_a_corner_on_the_optical_axis_of_a_fisheye_camera(dev):
    for sigma in (0.0, 0.3):
        fell, h = _compare(on_axis_scene(sigma), f"on axis sigma {sigma}", noise_free=not sigma)
        print("on axis: stopping-rule fallback taken:", fell)
        assert h.stamps_used == 6


def test_a_board_out_to_80_degrees(dev):
    for sigma in (0.0, 0.3):
        fell, h = _compare(wide_scene(sigma), f"wide sigma {sigma}", noise_free=not sigma)
        print("wide: stopping-rule fallback taken:", fell)
        assert h.stamps_used == 6


def test_a_view_with_a_pixel_outside_the_model(dev):
    for sigma in (0.0, 0.3):
        s, expect = outside_scene(sigma)
        fell, h = _compare(s, f"outside pixels sigma {sigma}", noise_free=not sigma)
        print("outside pixels: stopping-rule fallback taken:", fell)
        assert h.view_status.tolist() == expect.tolist() and h.stamps_used == 3 and h.stamp_points.tolist() == [36, 24, 0, 36]


# ------------------------------------------------------------------------------------------------ bits

def _table(packed, batch, pools, cameras, dists, models, masks=None):
    t = (rig._RigCamera * len(packed))()
    for c, p in enumerate(packed):
        if models[c] == "fisheye":
            cam9, d4 = fisheye._camera_args(cameras[c], dists[c])
            d8, nd = (ctypes.c_double * 8)(*d4), 0 if dists[c] is None else 4
        else:
            cam9, d8, nd = pnp._camera_args(cameras[c], dists[c])
        t[c] = rig._RigCamera(*corner_pool.ptrs(p.data_ptr(), batch, pools[c])[:4], pools[c],
                              None if masks is None or masks[c] is None else masks[c].data_ptr(), cam9, d8, nd)
    return t


class _Raw:
    """One scene's pools and buffers for raw calls of the two entries."""

    def __init__(self, s, cameras, dists, models, dev):
        self.s, self.C, self.B = s, len(s.cams), len(s.kps[0])
        packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
        self.packed, self.pools = [p[0] for p in packs], [p[2] for p in packs]
        self.table = _table(self.packed, self.B, self.pools, cameras, dists, models)
        self.need = rig.workspace_bytes(self.C, self.B, self.pools)
        self.ws = torch.zeros(self.need // 8 + 1, dtype=torch.float64, device=dev)
        self.st = torch.zeros(self.B * self.C, dtype=torch.int32, device=dev)
        self.pose = torch.zeros(self.B * 8, dtype=torch.float64, device=dev)
        self.info = torch.zeros(self.B * self.C * 2, dtype=torch.float64, device=dev)

    def call(self, entry, *models, n_cams=None, table=None, need=None, st=True, par=True):
        """-> (return code, every output as host arrays)"""
        res, parents = (ctypes.c_double * (8 + 6 * 7))(), (ctypes.c_int32 * 8)()
        for t in (self.st, self.pose, self.info):
            t.fill_(-7)
        rc = entry(self.C if n_cams is None else n_cams, self.table if table is None else table, *models, self.B, *self.s.board,
                   self.ws.data_ptr(), self.need if need is None else need, self.st.data_ptr() if st else None, self.pose.data_ptr(),
                   self.info.data_ptr(), parents if par else None, res, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, (self.st.cpu().numpy(), self.pose.cpu().numpy(), self.info.cpu().numpy(), np.array(res[:]), np.array(parents[:]))


def test_all_pinhole_calls_of_the_new_entry_are_the_old_entry(dev):
    """dcx_rig_calibrate_models_pool with a NULL model table and with a table of zeros against dcx_rig_calibrate_pool on test_rig_host's
    pinhole fan: every output bit for bit; and the same through rig.py's keyword."""
    L = _lib.lib()
    s = rx.scene(53, 9, sigma=0.3, rows=12, **PINHOLE_FAN3)
    cameras, dists = rx.cam_args(s)
    raw = _Raw(s, cameras, dists, ["pinhole"] * 3, dev)
    rc, old = raw.call(L.dcx_rig_calibrate_pool)
    assert rc == 0 and int(old[3][5]) == rig.RIG_OK and int(old[3][3]) == 9
    for models in (None, (ctypes.c_int * 3)(0, 0, 0)):
        rc, new = raw.call(L.dcx_rig_calibrate_models_pool, models)
        assert rc == 0
        for a, b in zip(new, old):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    _same_bits(rig.rig_calibrate_device(s.kps, *s.board, cameras, dists, models=["pinhole"] * 3),
               rig.rig_calibrate_device(s.kps, *s.board, cameras, dists))


def test_two_calls_give_the_same_bits(dev):
    s = class_scene("four F", 52, 0.3, n_stamps=40, rows=12)
    a, b = _device(s), _device(s)
    assert a.status == rig.RIG_OK and a.stamps_used == 40
    _same_bits(a, b)


def test_null_and_all_ones_masks_give_the_same_bits(dev):
    s = class_scene("fan3 F/P/F", 51, 0.3, n_stamps=9, board=sx.BOARD_L, rows=[[70, 20, 33]] * 9)
    plain = _device(s)
    ones = [[np.ones(n, bool)] * 9 for n in (70, 20, 33)]
    assert plain.status == rig.RIG_OK
    for masks in (ones, [ones[0], None, None], [None, ones[1], ones[2]]):
        _same_bits(_device(s, masks=masks), plain)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals(dev):
    L = _lib.lib()
    s = class_scene("fan3 F/P/F", 1, n_stamps=3, rows=9)
    cameras, dists = frx.cam_args(s)
    raw = _Raw(s, cameras, dists, frx.models(s), dev)
    entry = L.dcx_rig_calibrate_models_pool
    tags = lambda *m: (ctypes.c_int * 3)(*m)
    rc, out = raw.call(entry, tags(1, 0, 1))
    assert rc == 0 and int(out[3][5]) == rig.RIG_OK and int(out[3][3]) == 3
    for bad in (tags(1, 2, 1), tags(-1, 0, 1), tags(1, 0, 256 + 1)):                  # a model that does not exist
        assert raw.call(entry, bad)[0] == E_ARG
    for nd in (5, 8):                                                                 # a fisheye camera has 0 or 4 coefficients
        table = _table(raw.packed, raw.B, raw.pools, cameras, dists, frx.models(s))
        table[0].n_dist = nd
        assert raw.call(entry, tags(1, 0, 1), table=table)[0] == E_ARG
    assert raw.call(entry, tags(1, 0, 1), table=0)[0] == E_ARG                                      # no camera table
    assert raw.call(entry, tags(1, 0, 1), st=False)[0] == E_ARG and raw.call(entry, tags(1, 0, 1), par=False)[0] == E_ARG
    assert raw.call(entry, tags(1, 0, 1), n_cams=1)[0] == E_ARG and raw.call(entry, tags(1, 0, 1), n_cams=9)[0] == E_ARG
    assert raw.call(entry, tags(1, 0, 1), need=raw.need - 1)[0] == -3                 # DCX_E_WS
    skew = np.array(cameras[0])
    skew[0, 1] = 0.5
    for kw in (dict(models=["fisheye", "pinhole"]), dict(models=["fisheye", "pinhole", "wide"])):
        with pytest.raises(ValueError):
            rig.rig_calibrate_device(s.kps, *s.board, cameras, dists, **kw)
    with pytest.raises(ValueError):
        rig.rig_calibrate_device(s.kps, *s.board, [skew] + cameras[1:], dists, models=frx.models(s))
    with pytest.raises(ValueError):                                                   # five coefficients for a fisheye camera
        rig.rig_calibrate_device(s.kps, *s.board, cameras, [np.zeros(5)] + dists[1:], models=frx.models(s))
    bad = [list(k) for k in s.kps]
    bad[2][1] = bad[2][1].copy()
    bad[2][1][0, 2] = cx.n_ids(s.board)
    with pytest.raises(IndexError):
        rig.rig_calibrate_device(bad, *s.board, cameras, dists, models=frx.models(s))


# ------------------------------------------------------------------------------------------------ the two-camera solver

@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("cams", STEREO_PAIRS, ids=["/".join(c) for c in STEREO_PAIRS])
def test_stereo_device_matches_host(dev, cams, sigma):
    """stereo_calibrate_device(models=...) against stereo_calibrate_host_full(models=...) with test_gpu_stereo's comparison, one
    view lost to TOO_FEW; F is None on both sides."""
    s = frx.scene(23, 6, (0, 30), cams, sigma=sigma)
    kps = [list(s.kps[0]), list(s.kps[1])]
    kps[1][4] = kps[1][4][:3]
    args, kw = stereo_args(s._replace(kps=kps))
    h, margin = stereo.stereo_calibrate_host_full(*args, with_margin=True, **kw)
    assert margin >= MARGIN and h.pairs_used == 5 and h.F is None
    d = stereo.stereo_calibrate_device(*args, **kw)
    assert d.F is None and np.array_equal(d.E, pnp._skew(d.T) @ d.R)
    fell = _stereo_agree(d._replace(F=np.zeros((3, 3))), h._replace(F=np.zeros((3, 3))), f"{s.tag}", noise_free=not sigma)
    print(f"{s.tag}: stopping-rule fallback taken:", fell)


def test_all_pinhole_calls_of_the_stereo_models_entry_are_the_old_entry(dev):
    """models=("pinhole", "pinhole") goes through dcx_stereo_calibrate_models_pool with two zero tags: dcx_stereo_calibrate_pool's
    bits, on test_stereo_host's first case with noise."""
    s = sx.scene(1, 9, "small", sx.BOARD_S, "A", "B", sigma=0.3)
    old = stereo.stereo_calibrate_device(s.kps0, s.kps1, *s.board, *sx.cam_args(s))
    new = stereo.stereo_calibrate_device(s.kps0, s.kps1, *s.board, *sx.cam_args(s), models=("pinhole", "pinhole"))
    assert old.status == stereo.STEREO_OK and old.pairs_used == 9
    _same_bits(new, old)
    again = stereo.stereo_calibrate_device(*stereo_args(pair_scene(2, 0.3))[0], models=("fisheye", "fisheye"))
    _same_bits(again._replace(F=0), stereo.stereo_calibrate_device(*stereo_args(pair_scene(2, 0.3))[0], models=("fisheye", "fisheye"))._replace(F=0))


# ------------------------------------------------------------------------------------------------ end to end

def test_a_fisheye_pair_from_corners_to_common_rows(dev):
    """Two fisheye cameras' corners -> stereo_calibrate_device(models=...) -> stereo_rectify_fisheye_host -> the two maps (what
    remap_device warps through) and rectify_points_fisheye_pool: both cameras' pixels of a corner land on one row, within the
    bound the host definition was measured against."""
    s = pair_scene(1)
    cameras, dists = frx.cam_args(s)
    args, kw = stereo_args(s)
    r = stereo.stereo_calibrate_device(*args, **kw)
    assert r.status == stereo.STEREO_OK and r.pairs_used == 6
    rect = fisheye.stereo_rectify_fisheye_host(cameras[0], dists[0], cameras[1], dists[1], SIZE, r.R, r.T)
    W, H = SIZE
    for c, (R, P) in enumerate(((rect.R1, rect.P1), (rect.R2, rect.P2))):
        m = fisheye.undistort_rectify_map_fisheye_device(cameras[c], dists[c], R, P, W, H).cpu().numpy()
        host = fisheye.undistort_rectify_map_fisheye_host(cameras[c], dists[c], R, P, W, H)
        assert m.shape == (H, W, 2) and np.abs(m.astype(np.int64) - host).max() <= 1
    worst, n = 0.0, 0
    for t in range(6):
        rows = []
        for c, pix in enumerate(common_rows(s, t)):
            packed, b, pool = corner_pool.pack_keypoints([np.c_[pix, np.arange(len(pix))]], dev)
            R, P = ((rect.R1, rect.P1), (rect.R2, rect.P2))[c]
            rows.append(fisheye.rectify_points_fisheye_pool(packed, b, pool, True, cameras[c], dists[c], R, P).cpu().numpy()[:len(pix)])
        worst, n = max(worst, float(np.abs(rows[0][:, 1] - rows[1][:, 1]).max())), n + len(rows[0])
    print(f"end to end: {n} corners seen by both, rows differ by at most {worst:.2e} px (gate {ROWS_PX:.1e})")
    assert rect.axis == 0 and n >= 40 and worst <= ROWS_PX
