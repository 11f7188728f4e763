"""The memory contract of dcx_calibrate_flags_pool (include/deepcharuco_amd.h), raw, on tests/guarded.py arenas through the harness
of tests/test_gpu_workspace_contract.py (its ``drive``: a workspace of exactly dcx_calibrate_flags_workspace_bytes(batch, flags)
bytes and exact-size outputs between guards; workspace bodies of zeros, another call's leftovers, 0x7F and 0xFF; the same bits as
the call on roomy buffers each time; guards intact), for both model sizes, at an aligned workspace and at one that is 4 modulo 8,
and DCX_E_WS for a workspace one byte short.

The state words (LmState::code, lg, iters, attempts in Ws<M>::st of dcx_calib_dev.h) are written by calib_seed_kernel before the
first launch that tests them; without a guess the Zhang start's side state behind the model's workspace is written by dcx_calib.hip's
calib_init_reduce_kernel before the seed reads it."""
import ctypes

import numpy as np
import pytest
import torch

import camera_exact as cx
import pool_cases
from deepcharuco_amd import _lib, calib, corner_pool, pnp
from staged_exact import SENTINEL
from test_calib_flags_host import RAT_DIST, RAT_K, RAT_SIZE, TOGETHER, rational_views
from test_gpu_calib_flags import K_RATIO, _check, _check_by_position, wide_views
from test_gpu_workspace_contract import F64, FSENT, I32, _gpu, _stream, calib_pool, drive

pytestmark = pytest.mark.gpu

F = calib
G, R = F.CALIB_USE_INTRINSIC_GUESS, F.CALIB_RATIONAL_MODEL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _wide_scene(seed, n_ok):
    return _scene(wide_views(seed, n_ok + 1), n_ok)


def _rational_scene(seed, n_ok):
    return _scene(rational_views(n_ok + 1, 0.0, seed=seed), n_ok)


def _scene(made, n_ok):
    """n_ok views that stand, then three rows, an id outside the board, and a view cut by the pool's end."""
    _, imgs, ids_l, _ = made
    kps = [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]
    bad = kps[1].copy()
    bad[1, 2] = cx.n_ids(cx.CALIB_BOARD)
    views = kps[:n_ok] + [kps[0][:3].copy(), bad, kps[n_ok].copy()]
    return views, [pnp.PNP_OK] * n_ok + [pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_TRUNCATED]


def _camera9(K):
    return (ctypes.c_double * 9)(*np.asarray(K, np.float64).ravel().tolist())


CASES = {
    # a flagged 9-parameter call without a guess (the Zhang start, the aspect rule, the masked reduce_solve)
    "nine": dict(flags=TOGETHER | F.CALIB_FIX_ASPECT_RATIO, K=K_RATIO, dist=None, board=cx.CALIB_BOARD, size=RAT_SIZE, scene=_wide_scene,
                 seeds=(7, 8)),
    # the rational model from a guess (guess_views, the seed from the host's model, the NG = 12 kernels)
    "rational_guess": dict(flags=R | G, K=RAT_K * np.array([[1.02], [1.02], [1.0]]), dist=RAT_DIST, board=cx.CALIB_BOARD, size=RAT_SIZE,
                           scene=_rational_scene, seeds=(7, 9)),
    # the rational model without one
    "rational": dict(flags=R, K=None, dist=None, board=cx.CALIB_BOARD, size=RAT_SIZE, scene=_rational_scene, seeds=(7, 9)),
}


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned_by_4"])
@pytest.mark.parametrize("case", list(CASES))
def test_calibrate_flags_pool(dev, L, case, misaligned):
    """Eight views of which three fail three different checks, so every reduction runs over views that wrote nothing; the contents
    left behind are those of a 16-view call on another scene."""
    c = CASES[case]
    flags, board, size = c["flags"], c["board"], c["size"]
    views, expect = c["scene"](c["seeds"][0], 5)
    packed, _, pool = calib_pool(views, 7)
    big, _ = c["scene"](c["seeds"][1], 13)
    packed2, _, pool2 = calib_pool(big, 8)
    B, B2 = len(views), len(big)
    d, d2 = _gpu(dev, packed), _gpu(dev, packed2)
    need, need2 = L.dcx_calibrate_flags_workspace_bytes(B, flags), L.dcx_calibrate_flags_workspace_bytes(B2, flags)
    assert 0 < need < need2 and need == calib.flags_workspace_bytes(B, flags)
    cam = None if c["K"] is None else _camera9(c["K"])
    dist = None if c["dist"] is None else (ctypes.c_double * 8)(*c["dist"].tolist())
    n_dist = 0 if dist is None else 8
    res = (ctypes.c_double * 20)()

    def setup(bufs):
        ws = bufs.workspace("ws", need, need2, align=8, offset=4 if misaligned else 0)
        st, pose = bufs.output("view_status", (B,), I32, SENTINEL), bufs.output("pose", (B, 8), F64, FSENT)

        def run():
            args = (*corner_pool.ptrs(d.data_ptr(), B, pool)[:4], B, pool, *board, *size, flags, cam, dist, n_dist, ws.ptr)
            assert L.dcx_calibrate_flags_pool(*args, need - 1, st.ptr, pose.ptr, res, _stream()) == -3      # DCX_E_WS
            assert L.dcx_calibrate_flags_pool(*args, need, st.ptr, pose.ptr, res, _stream()) == 0
            return {"view_status": st.cpu().copy(), "pose": pose.cpu().copy(), "result": np.array(res[:], np.float64)}
        return run

    def left(bufs):
        tmp = torch.zeros(B2 * 9, dtype=F64, device=bufs.dev)
        r2 = (ctypes.c_double * 20)()
        assert L.dcx_calibrate_flags_pool(*corner_pool.ptrs(d2.data_ptr(), B2, pool2)[:4], B2, pool2, *board, *size, flags, cam, dist,
                                          n_dist, bufs.ws["ws"].ptr, need2, tmp.data_ptr(), tmp[B2:].data_ptr(), r2, _stream()) == 0
        assert int(r2[15]) == 13                      # thirteen views stood

    def after(g, got):
        out = got["view_status"] != pnp.PNP_OK
        assert not got["pose"][out, :7].any() and got["pose"][:, 7].tolist() == [len(v) for v in views]
        assert got["result"][17] == calib.CALIB_OK and not got["result"][18:].any()
        if not flags & R:
            assert not got["result"][9:12].any()
        return {"view_status": got["view_status"].tolist()}

    want, _ = drive(f"calibrate_flags_pool/{case}/{'misaligned_by_4' if misaligned else 'aligned'}", dev, setup, left, after=after)
    assert want["view_status"].tolist() == expect
    kw = dict(flags=flags, camera_matrix=c["K"], dist_coeffs=c["dist"])
    fm = calib._flag_model(flags, c["K"], c["dist"])
    dres = calib._flags_result(want["result"], want["view_status"], want["pose"], fm)
    use = [b for b in range(B) if expect[b] in (pnp.PNP_OK, pnp.PNP_TOO_FEW)]                 # what the host can take
    objs = [pnp.object_points(views[b][:, 2], *board) for b in use]
    imgs = [views[b][:, :2].astype(np.float32) for b in use]
    sel = np.array(use)
    sub = dres._replace(view_status=dres.view_status[sel], rvecs=dres.rvecs[sel], tvecs=dres.tvecs[sel], view_rms=dres.view_rms[sel],
                        view_points=dres.view_points[sel])
    if fm.rational:
        _check_by_position(sub, objs, imgs, size, f"calibrate_flags_pool/{case} on guarded buffers", **kw)
    else:
        _check(sub, calib.calibrate_camera_host_full(objs, imgs, size, **kw), f"calibrate_flags_pool/{case} on guarded buffers",
               rms_floor=1e-12)                                                                # (noise-free views)
