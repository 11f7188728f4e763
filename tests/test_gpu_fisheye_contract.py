"""The memory contract of the fisheye entries (include/deepcharuco_amd.h), on tests/guarded.py arenas through the harness of
tests/test_gpu_workspace_contract.py (its ``drive``: exact-size workspace and outputs between guards; workspace bodies of zeros,
another call's leftovers, 0x7F and 0xFF; the same bits as the call on roomy buffers each time; guards intact), and DCX_E_WS for a
workspace one byte short.  The state words of the calibration (LmState<8>::code, lg, iters, attempts, in Ws<FisheyeCalib>::st of
dcx_calib_dev.h) are written by dcx_fisheye.hip's fcal_init_state_kernel before the first launch that tests them."""
import ctypes

import numpy as np
import pytest
import torch

import fisheye_exact as fx
import pool_cases
from deepcharuco_amd import _lib, corner_pool, fisheye as fe, pnp, rectify as rc
from staged_exact import SENTINEL
from test_gpu_calib import _check
from test_gpu_workspace_contract import F64, FSENT, I32, _gpu, _stream, drive

pytestmark = pytest.mark.gpu

K, KD = fx.camera(150.0, 152.0, off=(4.0, -3.0)), fx.K_LENS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _views(seed, n_ok):
    """n_ok views that stand, then three rows, an id outside the board, and a view cut by the pool's end."""
    _, imgs, ids_l, _ = fx.make_views(seed, n_ok + 1, K, KD)
    kps = fx.keypoints(imgs, ids_l)
    bad = kps[1].copy()
    bad[1, 2] = 28
    views = kps[:n_ok] + [kps[0][:3].copy(), bad, kps[n_ok].copy()]
    return views, [pnp.PNP_OK] * n_ok + [pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_TRUNCATED]


def _pool(views, seed, gap=3, cut=4):
    B = len(views)
    order = list(np.random.default_rng(seed).permutation(B - 1)) + [B - 1]
    pool = sum(len(v) + gap for v in views) - gap - cut
    return pool_cases.lay_frames(views, pool, order, gap=gap, filler=-9)[0], pool


def _nothing(bufs):
    pass


def test_fisheye_calibrate_pool(dev, L):
    views, expect = _views(7, 5)
    packed, pool = _pool(views, 7)
    big, _ = _views(8, 13)
    packed2, pool2 = _pool(big, 8)
    B, B2 = len(views), len(big)
    d, d2 = _gpu(dev, packed), _gpu(dev, packed2)
    need, need2 = L.dcx_fisheye_calibrate_workspace_bytes(B), L.dcx_fisheye_calibrate_workspace_bytes(B2)
    assert 0 < need < need2 and L.dcx_fisheye_calibrate_workspace_bytes(0) == 0
    cam, dist = fe._camera_args(K, KD)
    res = (ctypes.c_double * 16)()

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=8)
        st, pose = bufs.output("view_status", (B,), I32, SENTINEL), bufs.output("pose", (B, 8), F64, FSENT)

        def run():
            args = (*corner_pool.ptrs(d.data_ptr(), B, pool)[:4], B, pool, *fx.BOARD, *fx.SIZE, 0.0, ws.ptr)
            assert L.dcx_fisheye_calibrate_pool(*args, need - 1, st.ptr, pose.ptr, res, _stream()) == -3      # DCX_E_WS
            assert L.dcx_fisheye_calibrate_pool(*args, need, st.ptr, pose.ptr, res, _stream()) == 0
            return {"view_status": st.cpu().copy(), "pose": pose.cpu().copy(), "result": np.array(res[:], np.float64)}
        return run

    def left(bufs):
        tmp = torch.zeros(B2 * 9, dtype=F64, device=bufs.dev)
        r2 = (ctypes.c_double * 16)()
        assert L.dcx_fisheye_calibrate_pool(*corner_pool.ptrs(d2.data_ptr(), B2, pool2)[:4], B2, pool2, *fx.BOARD, *fx.SIZE, 0.0,
                                            bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[B2:].data_ptr(), r2, _stream()) == 0
        assert int(r2[12]) == 13

    def after(g, got):
        out = got["view_status"] != pnp.PNP_OK
        assert not got["pose"][out, :7].any() and got["pose"][:, 7].tolist() == [len(v) for v in views]
        assert got["result"][8] == 0.0 and got["result"][15] == 0.0
        return {"view_status": got["view_status"].tolist()}

    want, _ = drive("fisheye_calibrate_pool", dev, setup, left, after=after)
    assert want["view_status"].tolist() == expect
    dres = fe.CalibResult(*fe._calib_fields(want["result"], want["view_status"], want["pose"]))
    use = [b for b in range(B) if expect[b] in (pnp.PNP_OK, pnp.PNP_TOO_FEW)]
    h = fe.calibrate_fisheye_host_full([pnp.object_points(views[b][:, 2], *fx.BOARD) for b in use],
                                       [views[b][:, :2].astype(np.float32) for b in use], fx.SIZE)
    sel = np.array(use)
    _check(dres._replace(view_status=dres.view_status[sel], rvecs=dres.rvecs[sel], tvecs=dres.tvecs[sel], view_rms=dres.view_rms[sel],
                         view_points=dres.view_points[sel]), h, "fisheye_calibrate_pool on guarded buffers", rms_floor=1e-12)


def test_fisheye_pose_map_and_points(dev, L):
    """The three entries without a workspace: outputs of exactly their size between guards."""
    views, expect = _views(9, 3)
    packed, pool = _pool(views, 9)
    B = len(views)
    d = _gpu(dev, packed)
    cam, dist = fe._camera_args(K, KD)
    ptrs = corner_pool.ptrs(d.data_ptr(), B, pool)[:4]

    def pose_setup(bufs):
        st, pose = bufs.output("status", (B,), I32, SENTINEL), bufs.output("pose", (B, 8), F64, FSENT)

        def run():
            assert L.dcx_fisheye_solve_pnp_pool(*ptrs, B, pool, *fx.BOARD, cam, dist, st.ptr, pose.ptr, _stream()) == 0
            return {"status": st.cpu().copy(), "pose": pose.cpu().copy()}
        return run

    want, _ = drive("fisheye_solve_pnp_pool", dev, pose_setup, _nothing, patterns=(("once", b"\x00"),))
    assert want["status"].tolist() == expect and not want["pose"][np.array(expect) != pnp.PNP_OK].any()

    w, h = 67, 5

    def map_setup(bufs):
        m = bufs.output("map", (h, w, 2), I32, 7)

        def run():
            assert L.dcx_fisheye_undistort_rectify_map(cam, dist, None, None, w, h, m.ptr, _stream()) == 0
            return {"map": m.cpu().copy()}
        return run

    want, _ = drive("fisheye_undistort_rectify_map", dev, map_setup, _nothing, patterns=(("once", b"\x00"),))
    host = fe.undistort_rectify_map_fisheye_host(K, KD, None, None, w, h)
    assert np.abs(want["map"].astype(np.int64) - host).max() <= 1

    def points_setup(bufs):
        o = bufs.output("points", (pool, 2), F64, FSENT)

        def run():
            assert L.dcx_fisheye_rectify_points_pool(ptrs[2], ptrs[3], pool, cam, dist, None, None, o.ptr, _stream()) == 0
            return {"points": o.cpu().copy()}
        return run

    want, _ = drive("fisheye_rectify_points_pool", dev, points_setup, _nothing, patterns=(("once", b"\x00"),))
    xy = corner_pool.views(packed, B, pool)[3].astype(np.float64)
    host = fe.rectify_points_fisheye_host(xy, K, KD)
    ok = ~np.isnan(host[:, 0])
    assert np.array_equal(np.isnan(want["points"][:, 0]), ~ok) and np.abs(want["points"][ok] - host[ok]).max() <= 1e-9
    assert L.dcx_fisheye_solve_pnp_pool(*ptrs, B, pool, *fx.BOARD, None, dist, 1, 1, _stream()) == -1            # DCX_E_ARG
    assert L.dcx_fisheye_undistort_rectify_map(cam, dist, None, None, 0, 5, 8, _stream()) == -1
