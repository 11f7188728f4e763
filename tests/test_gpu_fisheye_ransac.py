"""The device consensus pose on a fisheye camera (dcx_pnp_ransac.hip's two kernels on FisheyeCamera, through
dcx_fisheye_solve_pnp_ransac_pool and fisheye.solve_pnp_fisheye_ransac_*) against its host definition
solve_pnp_fisheye_ransac_host_full: the winner, the mask and the info words must be equal (the host's margin to every decision is
asserted first, >= 1e-6), the pose within test_gpu_pnp's gate, as tests/test_gpu_pnp_ransac.py holds the pinhole call."""
import ctypes

import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_exact as fx
import fisheye_rig_exact as frx
from deepcharuco_amd import _lib, corner_pool, fisheye, pnp
from test_fisheye_ransac_host import ARGS, K, KD, REPROJ, SEED, _outside_view, swapped_views
from test_gpu_pnp import _agree
from test_gpu_pnp_ransac import MARGIN, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _check(frames, board, cam, dist, tag, **ransac):
    """Every frame on the device in one call against the host definition -> the host statuses."""
    got = fisheye.solve_pnp_fisheye_ransac_batch_device(frames, *board, cam, dist, full=True, **ransac)
    tally, out = [0, 0, 0], []
    for i, (kp, (st, pose, mask, winner)) in enumerate(zip(frames, got)):
        hs, hp, hm, hw, margin = fisheye.solve_pnp_fisheye_ransac_host_full(kp, *board, cam, dist, with_margin=True, **ransac)
        print(f"{tag} #{i}: host status {hs} winner {hw} inliers {int(hm.sum())} margin {margin:.3g} | device {st} {winner} {int(mask.sum())}")
        assert margin >= MARGIN, (tag, i, margin)
        assert (st, winner) == (hs, hw) and mask.dtype == bool and np.array_equal(mask, hm), (tag, i, st, hs, winner, hw)
        if hs == pnp.PNP_OK:
            _agree(pose, hp, tally)
        else:
            assert not pose.any() and not mask.any()
        out.append(hs)
    print(f"{tag}: within 1e-9 / stopping-rule fallback / not converged: {tally}")
    return out


def _views(seed, n, sigma):
    _, imgs, ids_l, _ = fx.make_views(seed, n, K, KD, sigma=sigma)
    return fx.keypoints(imgs, ids_l)


def test_clean_and_exchanged_views_match_the_host_definition(dev):
    frames = _views(3, 4, 0.0) + _views(4, 4, 0.3) + [kp for kp, _, _ in swapped_views()] + [swapped_views(1)[0][0][:3]]
    st = _check(frames, fx.BOARD, K, KD, "views", **ARGS)
    assert st == [pnp.PNP_OK] * 14 + [pnp.PNP_TOO_FEW]
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    info = fisheye.solve_pnp_fisheye_ransac_pool(packed, b, pool, True, *fx.BOARD, K, KD, **ARGS)[2].cpu().numpy()
    assert info[8:14, 0].tolist() == [25] * 6 and info[:8, 0].tolist() == [28] * 8 and info[14].tolist() == [0, -1]


@pytest.mark.parametrize("iterations", [1, 64, 65])
def test_iterations_at_the_hypotheses_per_block_boundary(dev, iterations):
    frames = [kp for kp, _, _ in swapped_views()]
    _check(frames, fx.BOARD, K, KD, f"{iterations} iterations", **{**ARGS, "iterations": iterations})


def test_rows_4_and_129(dev):
    """The 24x17 board: 129 rows with eight ids exchanged in pairs, and four rows of it in general position."""
    board = cx.BOARDS[3]
    _, imgs, ids_l, _ = fx.make_views(21, 1, K, KD, board=board, rows=129, sigma=0.3, z_range=(0.05, 0.09))
    kp = fx.keypoints(imgs, ids_l)[0]
    g = cx.grid_xy(kp[:, 2], board[1]).astype(np.int64)
    four = kp[[int(np.argmin(g.sum(1))), int(np.argmax(g.sum(1))), int(np.argmin(g[:, 0] - g[:, 1])), int(np.argmax(g[:, 0] - g[:, 1]))]]
    big = kp.copy()
    big[[3, 40, 77, 100, 5, 60, 90, 120], 2] = big[[40, 3, 100, 77, 60, 5, 120, 90], 2]
    st = _check([big, four], board, K, KD, "rows 129 and 4", **ARGS)
    assert st == [pnp.PNP_OK, pnp.PNP_OK]


def test_a_sample_with_an_outside_pixel(dev):
    kp, Kn, kn = _outside_view()
    ids, rm1 = kp[:, 2].astype(np.int64), fx.BOARD[1] - 1
    hit = next(s for s in range(40) if (lambda q: q is not None and 0 in q)(pnp._ransac_sample(s, 12, 0, ids, rm1)))
    for kw in (dict(iterations=1, seed=hit), dict(iterations=100, seed=SEED)):
        st = _check([kp], fx.BOARD, Kn, kn, f"outside pixel {kw}", reproj_error=REPROJ, **kw)
        assert st == [pnp.PNP_DEGENERATE if kw["iterations"] == 1 else pnp.PNP_OK]


def test_graph_replay_equals_the_eager_call(dev):
    frames = [kp for kp, _, _ in swapped_views()]
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    args = (packed, b, pool, True, *fx.BOARD, K, KD)
    eager = fisheye.solve_pnp_fisheye_ransac_pool(*args, **ARGS)
    assert _same(eager, fisheye.solve_pnp_fisheye_ransac_pool(*args, **ARGS)) and (eager[0] == pnp.PNP_OK).all()
    ws = torch.empty((pnp.ransac_workspace_bytes(b, pool, 100) // 8,), dtype=torch.float64, device=dev)
    out = (torch.full_like(eager[0], -1), torch.full_like(eager[1], -1.0), torch.full_like(eager[2], -9), torch.zeros_like(eager[3]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                # warm-up launch outside the capture
        fisheye.solve_pnp_fisheye_ransac_pool(*args, out=out, workspace=ws, **ARGS)
    torch.cuda.current_stream().wait_stream(s)
    assert _same(eager, out)
    out[0].fill_(-1), out[1].fill_(-1.0), out[2].fill_(-9), out[3].zero_(), ws.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fisheye.solve_pnp_fisheye_ransac_pool(*args, out=out, workspace=ws, **ARGS)
    g.replay()
    torch.cuda.synchronize()
    assert _same(eager, out)


def test_refused_arguments(dev):
    L = _lib.lib()
    frames = [kp for kp, _, _ in swapped_views(2)]
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    ptrs = corner_pool.ptrs(packed.data_ptr(), b, pool)[:4]
    cam, dist = fisheye._camera_args(K, KD)
    need = pnp.ransac_workspace_bytes(b, pool, 100)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=dev)
    st, pose = torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(b * 8, dtype=torch.float64, device=dev)
    info, inl = torch.zeros(b * 2, dtype=torch.int32, device=dev), torch.zeros(pool, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(cam=cam, iterations=100, reproj=REPROJ, nbytes=need, status=st.data_ptr()):
        return L.dcx_fisheye_solve_pnp_ransac_pool(*ptrs, b, pool, *fx.BOARD, cam, dist, iterations, reproj, 4, SEED, ws.data_ptr(), nbytes,
                                                   status, pose.data_ptr(), info.data_ptr(), inl.data_ptr(), stream)
    assert call() == 0
    torch.cuda.synchronize()
    assert st.tolist() == [pnp.PNP_OK] * 2
    skew = (ctypes.c_double * 9)(*cam)
    skew[1] = 0.5
    for kw in (dict(cam=None), dict(cam=skew), dict(iterations=0), dict(iterations=pnp.RANSAC_MAX_ITERATIONS + 1), dict(reproj=0.0),
               dict(status=None)):
        assert call(**kw) == -1, kw
    assert call(nbytes=need - 1) == -3                                    # DCX_E_WS
    with pytest.raises(ValueError):
        fisheye.solve_pnp_fisheye_ransac_device(frames[0], *fx.BOARD, K, np.zeros(5))
    assert fisheye.solve_pnp_fisheye_ransac_device(frames[0][:3], *fx.BOARD, K, KD)[0] is False
    ret, rvec, tvec, inliers = fisheye.solve_pnp_fisheye_ransac_device(frames[0], *fx.BOARD, K, KD, **ARGS)
    assert ret is True and int(inliers.sum()) == 25 and rvec.shape == (3, 1)
