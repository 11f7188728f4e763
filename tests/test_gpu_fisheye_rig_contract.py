"""The memory contract of the three entries that take fisheye cameras into the joint and the consensus solvers
(dcx_rig_calibrate_models_pool, dcx_stereo_calibrate_models_pool, dcx_fisheye_solve_pnp_ransac_pool; include/deepcharuco_amd.h), on
tests/guarded.py arenas through the harness of tests/test_gpu_workspace_contract.py (its ``drive``: the workspace of exactly
dcx_rig_calibrate_workspace_bytes and the three outputs between guards; workspace bodies of zeros, another call's leftovers, 0x7F
and 0xFF; the same bits as the call on roomy buffers each time; guards intact), and DCX_E_WS for a workspace one byte short.  The
workspace layout is dcx_rig_calibrate_pool's, and so are the words a kernel uses as an index or a count and the launches that
write them first (tests/test_gpu_rig.py, test_memory_contract): the mixed kernels read and write the same words."""
import ctypes

import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_rig_exact as frx
import fisheye_exact as fx
import pool_cases
import stereo_exact as sx
from deepcharuco_amd import _lib, corner_pool, fisheye, pnp, rig, stereo
from staged_exact import SENTINEL
from test_fisheye_rig_host import class_scene
from test_gpu_fisheye_rig import _table
from test_gpu_rig import _agree, _hand_built_pool
from test_gpu_workspace_contract import F64, FSENT, I32, U8, USENT, _gpu, _stream, drive

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def test_rig_calibrate_models_pool(dev):
    """A fisheye, a pinhole and a fisheye camera, eight noisy timestamps in hand-built pools: one view to each check (TOO_FEW,
    BAD_ID, and DEGENERATE for a pixel outside the first camera's model) and one timestamp without camera 0, so the reductions
    run over views that wrote nothing.  A four-camera call of 20 timestamps leaves its contents."""
    L = _lib.lib()
    vis = np.ones((8, 3), bool)
    vis[3, 0] = False
    s = frx.scene(64, 8, (0, 25, -25), ("FN", "P", "F0"), visible=vis, sigma=0.3, rows=10)
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[0][5] = kps[0][5][:3]
    kps[1][1][4, 2] = cx.n_ids(s.board)
    K = sx.cam_K("FN")
    kps[0][6][2, :2] = [K[0, 2] - 1.02 * frx.THETA_D_MAX_FN * K[0, 0], K[1, 2]]
    cameras, dists = frx.cam_args(s)
    models = frx.models(s)
    B = 8
    pools = [2 + sum(len(k) + 3 for k in kps[c]) + 5 for c in range(3)]
    packed = [torch.from_numpy(_hand_built_pool(kps[c], pools[c], 1 + c)).to(dev) for c in range(3)]
    table, tags = _table(packed, B, pools, cameras, dists, models), (ctypes.c_int * 3)(*(rig.MODELS.index(m) for m in models))
    s2 = class_scene("four F", 65, 0.3, n_stamps=20, rows=9)
    packs2 = [corner_pool.pack_keypoints(k, dev) for k in s2.kps]
    pools2 = [p[2] for p in packs2]
    table2, tags2 = _table([p[0] for p in packs2], 20, pools2, *frx.cam_args(s2), frx.models(s2)), (ctypes.c_int * 4)(1, 1, 1, 1)
    need = L.dcx_rig_calibrate_workspace_bytes(3, B, (ctypes.c_int * 3)(*pools))
    need2 = L.dcx_rig_calibrate_workspace_bytes(4, 20, (ctypes.c_int * 4)(*pools2))
    assert 0 < need < need2
    res, par = (ctypes.c_double * 20)(), (ctypes.c_int32 * 3)()

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=16, offset=8)
        o = {"view_status": bufs.output("view_status", (B, 3), I32, SENTINEL), "pose": bufs.output("pose", (B, 8), F64, FSENT),
             "view_info": bufs.output("view_info", (B, 3, 2), F64, FSENT)}

        def run():
            args = (3, table, tags, B, *s.board, ws.ptr)
            outs = (o["view_status"].ptr, o["pose"].ptr, o["view_info"].ptr, par, res, _stream())
            assert L.dcx_rig_calibrate_models_pool(*args, need - 1, *outs) == -3                      # DCX_E_WS
            assert L.dcx_rig_calibrate_models_pool(*args, need, *outs) == 0
            torch.cuda.synchronize()
            got = {k: g.cpu().copy() for k, g in o.items()}
            got["result"], got["parents"] = np.array(res[:], np.float64), np.array(par[:], np.int32)
            return got
        return run

    def left(bufs):
        tmp = torch.zeros(20 * 4 * 4 + 20 * 8, dtype=F64, device=bufs.dev)
        r2, p2 = (ctypes.c_double * 26)(), (ctypes.c_int32 * 4)()
        assert L.dcx_rig_calibrate_models_pool(4, table2, tags2, 20, *s2.board, bufs.ws["ws"].ptr, need2, tmp.data_ptr(),
                                               tmp[80:].data_ptr(), tmp[240:].data_ptr(), p2, r2, _stream()) == 0
        assert int(r2[5]) == rig.RIG_OK and int(r2[3]) == 20

    want, _ = drive("rig_calibrate_models_pool", dev, setup, left)
    exp = np.zeros((B, 3), np.int32)
    exp[3, 0], exp[5, 0], exp[1, 1], exp[6, 0] = pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE
    r, st, pose, info = want["result"], want["view_status"], want["pose"], want["view_info"]
    assert st.tolist() == exp.tolist() and want["parents"].tolist() == [-1, 0, 0]
    assert int(r[5]) == rig.RIG_OK and int(r[3]) == 8 and r[6] == 0 and r[7] == 0
    X = r[8:].reshape(2, 6)
    rvec, T = np.zeros((3, 3)), np.zeros((3, 3))
    rvec[1:], T[1:] = X[:, :3], X[:, 3:]
    d = rig.RigResult(int(r[5]), float(r[0]), np.stack([pnp._rodrigues(v) for v in rvec]), T, rvec, want["parents"], st,
                      info[:, :, 1].astype(np.int64), info[:, :, 0].copy(), pose[:, :3].copy(), pose[:, 3:6].copy(), pose[:, 6].copy(),
                      pose[:, 7].astype(np.int64), int(r[1]), int(r[2]), int(r[3]), int(r[4]))
    h = rig.rig_calibrate_host_full(kps, *s.board, cameras, dists, models=models)
    _agree(d, h, "dcx_rig_calibrate_models_pool on guarded buffers")


def test_stereo_calibrate_models_pool(dev):
    """A fisheye and a pinhole camera, eight noisy timestamps in hand-built pools, a view each to TOO_FEW, BAD_ID and DEGENERATE (a
    pixel outside the fisheye lens); a fisheye pair of 16 timestamps leaves its contents.  DCX_E_ARG for a model that does not
    exist and for a fisheye camera with five coefficients."""
    from test_gpu_stereo import _agree as stereo_agree
    L = _lib.lib()
    s = frx.scene(66, 8, (0, 30), ("FN", "P"), sigma=0.3, rows=10)
    kps = [[k.copy() for k in kl] for kl in s.kps]
    kps[0][5] = kps[0][5][:3]
    kps[1][1][4, 2] = cx.n_ids(s.board)
    K = sx.cam_K("FN")
    kps[0][6][2, :2] = [K[0, 2] - 1.02 * frx.THETA_D_MAX_FN * K[0, 0], K[1, 2]]
    (K0, K1), (d0, d1) = frx.cam_args(s)
    B = 8
    pools = [2 + sum(len(k) + 3 for k in kps[c]) + 5 for c in range(2)]
    packed = [torch.from_numpy(_hand_built_pool(kps[c], pools[c], 1 + c)).to(dev) for c in range(2)]
    cams = stereo._model_args(K0, d0, "fisheye") + stereo._model_args(K1, d1, "pinhole")
    s2 = frx.scene(67, 16, (0, 30), ("F", "F0"), sigma=0.3, rows=9)
    packs2 = [corner_pool.pack_keypoints(k, dev) for k in s2.kps]
    cams2 = stereo._model_args(*[a[0] for a in frx.cam_args(s2)], "fisheye") + stereo._model_args(*[a[1] for a in frx.cam_args(s2)], "fisheye")
    need = L.dcx_stereo_calibrate_workspace_bytes(B, *pools)
    need2 = L.dcx_stereo_calibrate_workspace_bytes(16, packs2[0][2], packs2[1][2])
    assert 0 < need < need2
    res = (ctypes.c_double * 16)()

    def call(pk, n, pls, cm, m0, m1, ws_ptr, nbytes, st, pose, info, r):
        return L.dcx_stereo_calibrate_models_pool(*corner_pool.ptrs(pk[0].data_ptr(), n, pls[0])[:4], None,
                                                  *corner_pool.ptrs(pk[1].data_ptr(), n, pls[1])[:4], None, n, *pls, *s.board, *cm, m0, m1,
                                                  ws_ptr, nbytes, st, pose, info, r, _stream())

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=16, offset=8)
        o = {"view_status": bufs.output("view_status", (B, 2), I32, SENTINEL), "pose": bufs.output("pose", (B, 8), F64, FSENT),
             "view_info": bufs.output("view_info", (B, 2, 2), F64, FSENT)}

        def run():
            outs = (o["view_status"].ptr, o["pose"].ptr, o["view_info"].ptr, res)
            assert call(packed, B, pools, cams, 1, 0, ws.ptr, need - 1, *outs) == -3                  # DCX_E_WS
            assert call(packed, B, pools, cams, 2, 0, ws.ptr, need, *outs) == -1                      # no such model
            five = cams[:2] + (5,) + cams[3:]
            assert call(packed, B, pools, five, 1, 0, ws.ptr, need, *outs) == -1                      # a fisheye camera with n_dist 5
            assert call(packed, B, pools, cams, 1, 0, ws.ptr, need, *outs) == 0
            torch.cuda.synchronize()
            got = {k: g.cpu().copy() for k, g in o.items()}
            got["result"] = np.array(res[:], np.float64)
            return got
        return run

    def left(bufs):
        tmp = torch.zeros(16 * 14, dtype=F64, device=bufs.dev)
        r2 = (ctypes.c_double * 16)()
        assert call([p[0] for p in packs2], 16, [p[2] for p in packs2], cams2, 1, 1, bufs.ws["ws"].ptr, need2, tmp.data_ptr(),
                    tmp[16:].data_ptr(), tmp[16 * 9:].data_ptr(), r2) == 0
        assert int(r2[11]) == stereo.STEREO_OK and int(r2[9]) == 16

    want, _ = drive("stereo_calibrate_models_pool", dev, setup, left)
    exp = np.zeros((B, 2), np.int32)
    exp[5, 0], exp[1, 1], exp[6, 0] = pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE
    r, pose, info = want["result"], want["pose"], want["view_info"]
    assert want["view_status"].tolist() == exp.tolist() and int(r[11]) == stereo.STEREO_OK and int(r[9]) == 5
    R = pnp._rodrigues(r[0:3])
    d = stereo.StereoResult(0, float(r[6]), R, r[3:6].copy(), r[0:3].copy(), pnp._skew(r[3:6]) @ R, np.zeros((3, 3)), want["view_status"],
                            pose[:, 0:3].copy(), pose[:, 3:6].copy(), pose[:, 6].copy(), pose[:, 7].astype(np.int64), info[:, :, 0].copy(),
                            info[:, :, 1].astype(np.int64), int(r[7]), int(r[8]), int(r[9]), int(r[10]))
    h = stereo.stereo_calibrate_host_full(kps[0], kps[1], *s.board, K0, d0, K1, d1, models=("fisheye", "pinhole"))
    stereo_agree(d, h._replace(F=np.zeros((3, 3))), "dcx_stereo_calibrate_models_pool on guarded buffers")


def test_fisheye_solve_pnp_ransac_pool(dev):
    """Six views in a hand-built pool with gaps (three ids exchanged in each), the workspace exactly
    dcx_solve_pnp_ransac_workspace_bytes, 8-byte and not 16-byte aligned; the mask guarded: slots of no frame keep its sentinel."""
    from test_fisheye_ransac_host import ARGS, K, KD, swapped_views
    L = _lib.lib()
    frames = [kp for kp, _, _ in swapped_views()]
    frames[4] = frames[4][:3]                                             # TOO_FEW
    B = len(frames)
    pool = sum(len(f) + 3 for f in frames) + 4
    packed, owned = pool_cases.lay_frames(frames, pool, [5, 0, 4, 1, 3, 2], gap=3, filler=-9, id_sorted=True)
    other, _ = pool_cases.lay_frames(frames[::-1], pool, [3, 1, 5, 0, 2, 4], gap=3, filler=-9, id_sorted=True)
    assert (~owned).sum() >= 15
    d, d2 = _gpu(dev, packed), _gpu(dev, other)
    cam, dist = fisheye._camera_args(K, KD)
    need = L.dcx_solve_pnp_ransac_workspace_bytes(B, pool, 100)

    def call(p, ws_ptr, nbytes, st, pose, info, inl, seed):
        return L.dcx_fisheye_solve_pnp_ransac_pool(*corner_pool.ptrs(p.data_ptr(), B, pool)[:4], B, pool, *fx.BOARD, cam, dist, 100,
                                                   ARGS["reproj_error"], 4, seed, ws_ptr, nbytes, st, pose, info, inl, _stream())

    def setup(bufs):
        ws = bufs.workspace("ws", need, align=16, offset=8)
        o = {"status": bufs.output("status", (B,), I32, SENTINEL), "pose": bufs.output("pose", (B, 8), F64, FSENT),
             "info": bufs.output("info", (B, 2), I32, SENTINEL), "inliers": bufs.output("inliers", (pool,), U8, USENT)}

        def run():
            outs = (o["status"].ptr, o["pose"].ptr, o["info"].ptr, o["inliers"].ptr)
            assert call(d, ws.ptr, need - 1, *outs, ARGS["seed"]) == -3   # DCX_E_WS
            assert call(d, ws.ptr, need, *outs, ARGS["seed"]) == 0
            torch.cuda.synchronize()
            got = {k: g.cpu().copy() for k, g in o.items()}
            got["inliers"] = got["inliers"][owned]
            return got
        return run

    def left(bufs):
        tmp = torch.zeros(B * 11 + pool, dtype=F64, device=bufs.dev)
        assert call(d2, bufs.ws["ws"].ptr, need, tmp.data_ptr(), tmp[B:].data_ptr(), tmp[9 * B:].data_ptr(), None, ARGS["seed"] + 1) == 0

    def after(g, got):
        assert g.out["inliers"].untouched(~owned), "a mask slot of no frame written"
        assert not got["pose"][got["status"] != pnp.PNP_OK].any()
        return {"status": got["status"].tolist()}

    want, _ = drive("fisheye_solve_pnp_ransac_pool", dev, setup, left, after=after)
    assert want["status"].tolist() == [0, 0, 0, 0, pnp.PNP_TOO_FEW, 0] and want["info"][:, 0].tolist() == [25, 25, 25, 25, 0, 25]
    mask = np.zeros(pool, np.uint8)
    mask[owned] = want["inliers"]
    for b in (0, 5):
        s0, n = int(packed[B + b]), int(packed[b])
        hs, hp, hm, hw = fisheye.solve_pnp_fisheye_ransac_host_full(frames[b], *fx.BOARD, K, KD, **ARGS)
        order = np.argsort(frames[b][:, 2], kind="stable")
        assert hs == pnp.PNP_OK and int(want["info"][b, 1]) == hw and np.array_equal(mask[s0:s0 + n].astype(bool), hm[order])
        assert np.abs(want["pose"][b, :6] - hp[:6]).max() <= 1e-9 * np.abs(hp[:6]).max()
