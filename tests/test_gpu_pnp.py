"""The device PnP solver (csrc/dcx_pnp.hip through deepcharuco_amd/pnp.py) against its host definition solve_pnp_host: seeded
frames, a hand-built corner pool with every status, the corner pool infer_batch_device leaves in HBM (no host sync in between),
hipGraph capture, and FrameStream's device PnP stage.

The two differ only in fp64 summation order, and the gate is 1e-9 relative in rvec and tvec.  One thing can move a frame further:
the stopping rule (OpenCV's: |dp| / |p| < FLT_EPSILON, at most 20 steps).  On an ill-conditioned noisy view Gauss-Newton converges
linearly (cond(JtJ) ~ 1e6 for a 3 cm board at 15 cm), the last steps change the cost by ~1e-14 relative, and whether such a step is
accepted is decided by rounding: two exact implementations can then stop one step (< FLT_EPSILON |p|) apart.  Such a frame passes
if both stopped by the rule, agree to 1e-6 and reach the same cost to 1e-12; a frame that ran into the 20-step cap is not
converged and only its status is compared.  The tests report how many frames needed the fallback, and most must not."""
import numpy as np
import pytest
import torch

import pool_cases
from conftest import GoldenCase
from deepcharuco_amd import corner_pool, pnp
from test_pnp_host import BOARD, DIST5, K, make_frame

pytestmark = pytest.mark.gpu

REL = 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _rel(a, b):
    return max(np.linalg.norm(a[:3] - b[:3]) / np.linalg.norm(b[:3]), np.linalg.norm(a[3:6] - b[3:6]) / np.linalg.norm(b[3:6]))


def _agree(dev8, host8, tally):
    """Device pose [8] vs host pose [8] (module docstring); tally[0] += 1 for a frame within REL, tally[1] for the fallback."""
    d = _rel(dev8, host8)
    if d <= REL:
        tally[0] += 1
        return
    assert max(dev8[7], host8[7]) < pnp.LM_MAX_ITER or dev8[7] == host8[7] == pnp.LM_MAX_ITER, (dev8, host8)
    if dev8[7] == host8[7] == pnp.LM_MAX_ITER:       # not converged: the path depends on rounding
        tally[2] += 1
        return
    assert d <= 1e-6 and abs(dev8[6] - host8[6]) <= 1e-12 * host8[6], (d, dev8, host8)
    tally[1] += 1


def _check_against_host(st, pose, frames, board, cam, dist):
    tally = [0, 0, 0]
    for b, kp in enumerate(frames):
        hs, hp = pnp.solve_pnp_host_full(kp, *board, cam, dist) if kp is not None else (pnp.PNP_TRUNCATED, None)
        assert st[b] == hs, (b, st[b], hs)
        if hs == pnp.PNP_OK:
            _agree(pose[b], hp, tally)
        else:
            assert not pose[b].any()
    return tally


def _models(case, dev):
    from deepcharuco_amd.models.net import dcModel, lModel
    from deepcharuco_amd.models.refinenet import RefineNet, lRefineNet
    return lModel(dcModel(case.n_ids, case.sd_dc, dev)), lRefineNet(RefineNet(case.sd_rn, dev))


def test_batch_device_matches_host_64_frames(dev):
    rng = np.random.default_rng(2024)
    frames = []
    for i in range(64):
        n = int(rng.integers(6, 17))
        ids = np.sort(rng.choice(16, n, replace=False))
        while np.linalg.matrix_rank(pnp.object_points(ids, *BOARD)[:, :2] - pnp.object_points(ids, *BOARD)[:, :2].mean(0),
                                    tol=1e-6) < 2:
            ids = np.sort(rng.choice(16, n, replace=False))
        frames.append(make_frame(rng, ids=ids, sigma=0.3 if i % 2 else 0.0)[0])
    got = pnp.solve_pnp_batch_device(frames, *BOARD, K, DIST5)
    assert len(got) == 64
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    st, pose = pnp.solve_pnp_pool(packed, b, pool, True, *BOARD, K, DIST5)
    st, pose = st.cpu().numpy(), pose.cpu().numpy()
    for b, (ret, rvec, tvec) in enumerate(got):         # the list form is the pool form, unpacked
        assert ret is True and st[b] == pnp.PNP_OK
        assert rvec.shape == (3, 1) and tvec.shape == (3, 1) and rvec.dtype == np.float64
        assert np.array_equal(np.r_[rvec.ravel(), tvec.ravel()], pose[b, :6])
    tally = _check_against_host(st, pose, frames, BOARD, K, DIST5)
    print("within 1e-9 / stopping-rule fallback / 20-step cap:", tally)
    assert tally[0] >= 48 and tally[0] + tally[1] + tally[2] == 64
    assert all(_rel(pose[i], pnp.solve_pnp_host_full(frames[i], *BOARD, K, DIST5)[1]) <= REL for i in range(0, 64, 2))  # noise-free
    # single-frame drop-in, shaped like cv2's
    ret, rvec, tvec = pnp.solve_pnp_device(frames[0], *BOARD, K, DIST5)
    assert ret is True and np.array_equal(np.r_[rvec.ravel(), tvec.ravel()], np.r_[got[0][1].ravel(), got[0][2].ravel()])
    assert pnp.solve_pnp_device(frames[0][:3], *BOARD, K, DIST5) == (False, None, None)
    bad = frames[0].copy()
    bad[0, 2] = 16
    with pytest.raises(IndexError):
        pnp.solve_pnp_device(bad, *BOARD, K, DIST5)
    with pytest.raises(ValueError):
        pnp.solve_pnp_device(frames[0], *BOARD, K, np.zeros(12))


def _board_frame(rng, ids, board, sigma):
    """A frame on a (col, row, square) board: the pose keeps the board's centre near the optical axis at 0.12-0.2 m."""
    col, row, sq = board
    r = rng.normal(size=3)
    r *= np.deg2rad(rng.uniform(5, 50)) / np.linalg.norm(r)
    R = pnp._rodrigues(r)
    centre = np.array([col * sq / 2, row * sq / 2, 0.0])
    t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.12, 0.2)]) - R @ centre
    obj = pnp.object_points(ids, *board).astype(np.float64)
    img, _, _ = pnp._project(obj, np.zeros((len(ids), 2)), np.r_[r, t], K, pnp._dist(DIST5), False)
    img = img + rng.normal(scale=sigma, size=img.shape)
    return np.c_[img.astype(np.float32).astype(np.float64), ids]


def test_pool_hand_built_every_status(dev):
    """Frames in scrambled pool order, 300 points in one frame (several per lane), 3 points, an empty frame, a truncated frame,
    a bad id and collinear points; once with the refined xy, once with the integer rows."""
    board = (20, 20, 0.002)
    rng = np.random.default_rng(77)
    frames = [
        _board_frame(rng, np.arange(16) * 7, board, 0.0),                              # 0: OK
        _board_frame(rng, np.sort(rng.choice(361, 300, replace=False)), board, 0.3),   # 1: OK, 300 points
        _board_frame(rng, np.array([3, 50, 200]), board, 0.0),                         # 2: TOO_FEW
        np.zeros((0, 3)),                                                              # 3: TOO_FEW (empty)
        _board_frame(rng, np.arange(10) * 13, board, 0.0),                             # 4: TRUNCATED
        _board_frame(rng, np.arange(12) * 5, board, 0.3),                              # 5: BAD_ID (one id = 361)
        _board_frame(rng, np.arange(19) * 19, board, 0.0),                             # 6: DEGENERATE (column of the board)
        _board_frame(rng, np.arange(40, 80), board, 0.3),                              # 7: OK
    ]
    frames[5][4, 2] = 361
    order = [7, 4, 1, 0, 6, 3, 5, 2]          # pool order; frame 4 goes last but one ... then is cut by the pool size
    order.remove(4)
    order.append(4)
    B = len(frames)
    pool = sum(len(f) for f in frames) - 3    # frame 4 (last in the pool) does not fit
    packed, _ = pool_cases.lay_frames(frames, pool, order, cell=-7)
    d = torch.from_numpy(packed).to(dev)
    expect = [pnp.PNP_OK, pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW, pnp.PNP_TRUNCATED, pnp.PNP_BAD_ID,
              pnp.PNP_DEGENERATE, pnp.PNP_OK]
    st, pose = pnp.solve_pnp_pool(d, B, pool, True, *board, K, DIST5)
    st, pose = st.cpu().numpy(), pose.cpu().numpy()
    assert st.tolist() == expect
    tally = [0, 0, 0]
    for b in (0, 1, 7):
        _, hp = pnp.solve_pnp_host_full(frames[b], *board, K, DIST5)
        _agree(pose[b], hp, tally)
    assert not pose[[2, 3, 4, 5, 6]].any()
    assert pose[1, 7] >= 1 and 0.1 < pose[1, 6] < 0.5             # rms ~ sigma = 0.3 px
    # integer rows as the image points (no RefineNet)
    st_i, pose_i = pnp.solve_pnp_pool(d, B, pool, False, *board, K, DIST5)
    st_i, pose_i = st_i.cpu().numpy(), pose_i.cpu().numpy()
    assert st_i.tolist() == expect
    for b in (0, 1, 7):
        kpi = np.c_[np.rint(frames[b][:, :2]).astype(np.int64), frames[b][:, 2].astype(np.int64)]
        _, hp = pnp.solve_pnp_host_full(kpi, *board, K, DIST5)
        _agree(pose_i[b], hp, tally)
    assert tally[0] >= 4, tally


def _pipeline_and_pnp(case, dev, frames):
    from deepcharuco_amd.inference import infer_batch_device
    dc, rn = _models(case, dev)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    pool = 64 * len(frames)
    packed = infer_batch_device(d_frames, case.n_ids, dc, rn, pool=pool)
    cam = np.array([[300.0, 0, frames.shape[2] / 2], [0, 300.0, frames.shape[1] / 2], [0, 0, 1]])
    st, pose = pnp.solve_pnp_pool(packed, len(frames), pool, True, 5, 5, 0.01, cam, DIST5)     # no sync in between
    return packed, pool, cam, st, pose


@pytest.mark.parametrize("name", ["board_240x320", "diverse_ids_240x320"])
def test_end_to_end_from_the_corner_pool(dev, name):
    from deepcharuco_amd.inference import unpack_results
    case = GoldenCase(name)
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1]])
    packed, pool, cam, st, pose = _pipeline_and_pnp(case, dev, frames)
    res, _ = unpack_results(packed.cpu().numpy(), len(frames), pool, True)
    tally = _check_against_host(st.cpu().numpy(), pose.cpu().numpy(), res, (5, 5, 0.01), cam, DIST5)
    print("within 1e-9 / stopping-rule fallback / 20-step cap:", tally)
    if name.startswith("diverse"):
        assert st.cpu().numpy()[0] == pnp.PNP_OK


def test_graph_capture_bit_identical(dev):
    case = GoldenCase("diverse_ids_240x320")
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1]])
    packed, pool, cam, st, pose = _pipeline_and_pnp(case, dev, frames)
    out = (torch.full_like(st, -1), torch.full_like(pose, -1.0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):            # warm-up launch outside the capture
        pnp.solve_pnp_pool(packed, len(frames), pool, True, 5, 5, 0.01, cam, DIST5, out=out)
    torch.cuda.current_stream().wait_stream(s)
    out[0].fill_(-1)
    out[1].fill_(-1.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pnp.solve_pnp_pool(packed, len(frames), pool, True, 5, 5, 0.01, cam, DIST5, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], st)
    assert np.array_equal(out[1].cpu().numpy().view(np.uint64), pose.cpu().numpy().view(np.uint64))


def test_frame_stream_device_pnp(dev):
    from deepcharuco_amd.stream import FrameStream
    case = GoldenCase("diverse_ids_240x320")
    dc, rn = _models(case, dev)
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1]] + [np.roll(f, 8 * k, axis=1) for k in range(1, 7)])
    cfg = dict(col_count=5, row_count=5, square_len=0.01, camera_matrix=np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]]),
               dist_coeffs=DIST5)
    batches = [frames[i:i + 4] for i in range(0, 10, 4)]
    plain = list(FrameStream(case.n_ids, dc, rn, batch=4, height=240, width=320, depth=2).run(batches))
    out = list(FrameStream(case.n_ids, dc, rn, batch=4, height=240, width=320, depth=2, pnp=cfg, pnp_device=True).run(batches))
    assert [o[0] for o in out] == [0, 1, 2] and all(len(o) == 3 for o in out)
    kps = [a for o in plain for a in o[1]]
    kps2 = [a for o in out for a in o[1]]
    poses = [p for o in out for p in o[2]]
    assert len(kps) == len(kps2) == len(poses) == 10
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(kps, kps2))
    # the stage is solve_pnp_pool on each batch's own corner pool: bit for bit
    from deepcharuco_amd.inference import infer_batch_device
    want = []
    for fr in batches:
        d = torch.zeros((4, 240, 320), dtype=torch.uint8, device=dev)
        d[:len(fr)] = torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
        packed = infer_batch_device(d, case.n_ids, dc, rn, pool=4 * 64)
        st, pose = pnp.solve_pnp_pool(packed, 4, 4 * 64, True, **cfg)
        st, pose = st.cpu().numpy()[:len(fr)], pose.cpu().numpy()[:len(fr)]
        want += [(int(a), b) for a, b in zip(st, pose)]
    n_ok = 0
    for (ret, rvec, tvec), (s_, p_) in zip(poses, want):
        assert ret == (s_ == pnp.PNP_OK)
        if ret:
            n_ok += 1
            assert np.array_equal(np.r_[rvec.ravel(), tvec.ravel()], p_[:6])
        else:
            assert rvec is None and tvec is None
    assert n_ok >= 1
    # and, on the id-sorted keypoints, what solve_pnp_batch_device / the host definition give
    ref = pnp.solve_pnp_batch_device(kps, **cfg)
    assert [r[0] for r in ref] == [r[0] for r in poses]
    tally = [0, 0, 0]
    for kp, (s_, p_) in zip(kps, want):
        if s_ == pnp.PNP_OK:
            _agree(p_, pnp.solve_pnp_host_full(kp, **cfg)[1], tally)
    print("within 1e-9 / stopping-rule fallback / 20-step cap:", tally)
