"""The device RANSAC pose solver (csrc/dcx_pnp_ransac.hip through deepcharuco_amd/pnp.py) against its host definition
solve_pnp_ransac_host_full: frames with planted wrong ids and clean ones, a hand-built corner pool with every status, batch
invariance, hipGraph capture, the corner pool infer_batch_device leaves in HBM, FrameStream's stage and the C ABI's argument checks.

The discrete outputs (status, winning hypothesis, inlier count, mask) must be EQUAL to the host's.  That is fair because every
frame compared here has a margin >= 1e-6 (asserted from the host run: no row of any hypothesis that scores within one of the
winner lies closer than that, relatively, to the inlier threshold), five orders above the ~1e-9 at which device and host poses
agree.  The refit pose is compared like the plain solver's (tests/test_gpu_pnp.py: 1e-9 relative, its stated fallback for frames
stopped by the rounding of the last LM step)."""
import ctypes

import numpy as np
import pytest
import torch

import pool_cases
from conftest import GoldenCase
from deepcharuco_amd import corner_pool, pnp
from test_gpu_pnp import _agree, _board_frame, _models
from test_pnp_host import BOARD, DIST5, K, make_frame
from test_pnp_ransac_host import REPROJ, SAMPLER_SEED, planted_frames

pytestmark = pytest.mark.gpu

RANSAC = dict(iterations=100, reproj_error=REPROJ, min_inliers=4, seed=SAMPLER_SEED)
MARGIN = 1e-6
E2E_SEED = 24      # the golden frames' corners lie on no board; under this seed the unflipped diverse-ids frame reaches a 4-row consensus at 8 px


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _check_frame(got, kp, board, cam, dist, ransac, tally, tag, pool_order=False):
    """got = (status, pose[8], mask in kp's row order, winner) from the device against the host definition on kp."""
    st, pose, mask, winner = got
    hs, hp, hm, hw, margin = pnp.solve_pnp_ransac_host_full(kp, *board, cam, dist, with_margin=True, pool_order=pool_order, **ransac)
    print(tag, "host status", hs, "winner", hw, "inliers", int(hm.sum()), "margin %.3g" % margin, "| device", st, winner, int(mask.sum()))
    assert margin >= MARGIN, (tag, margin)
    assert st == hs and winner == hw, (tag, st, hs, winner, hw)
    assert mask.dtype == bool and np.array_equal(mask, hm), (tag, mask, hm)
    if hs == pnp.PNP_OK:
        _agree(pose, hp, tally)
    else:
        assert not pose.any() and not mask.any()
    return hs


def test_planted_and_clean_frames_match_the_host_definition(dev):
    planted = planted_frames()
    rng = np.random.default_rng(4242)
    clean = []
    for i in range(32):
        n = int(rng.integers(6, 17))
        ids = np.sort(rng.choice(16, n, replace=False))
        while np.linalg.matrix_rank(pnp.object_points(ids, *BOARD)[:, :2] - pnp.object_points(ids, *BOARD)[:, :2].mean(0),
                                    tol=1e-6) < 2:
            ids = np.sort(rng.choice(16, n, replace=False))
        kp = make_frame(rng, ids=ids, sigma=0.3 if i % 2 else 0.0)[0]
        clean.append(kp[rng.permutation(n)])                       # the caller's row order is not the pool's
    frames = [p[0] for p in planted] + clean
    got = pnp.solve_pnp_ransac_batch_device(frames, *BOARD, K, DIST5, full=True, **RANSAC)
    cv = pnp.solve_pnp_ransac_batch_device(frames, *BOARD, K, DIST5, **RANSAC)
    assert len(got) == len(cv) == 64
    tally, n_ok = [0, 0, 0], 0
    for b, kp in enumerate(frames):
        hs = _check_frame(got[b], kp, BOARD, K, DIST5, RANSAC, tally, f"frame {b}")
        n_ok += hs == pnp.PNP_OK
        ret, rvec, tvec, inl = cv[b]                                # the cv2-shaped form is the full form, unpacked
        assert ret is (hs == pnp.PNP_OK) and np.array_equal(inl, got[b][2])
        if ret:
            assert rvec.shape == (3, 1) and tvec.shape == (3, 1) and rvec.dtype == np.float64
            assert np.array_equal(np.r_[rvec.ravel(), tvec.ravel()], got[b][1][:6])
    for b, (kp, good, _) in enumerate(planted):                     # and what the host test showed: the planted rows, exactly
        assert got[b][0] == pnp.PNP_OK and np.array_equal(got[b][2], good)
    print("within 1e-9 / stopping-rule fallback / 20-step cap:", tally, "of", n_ok)
    assert n_ok >= 60 and tally[0] >= 0.75 * n_ok and sum(tally) == n_ok
    # single-frame drop-in
    one = pnp.solve_pnp_ransac_device(frames[0], *BOARD, K, DIST5, **RANSAC)
    assert one[0] is True and np.array_equal(np.r_[one[1].ravel(), one[2].ravel()], got[0][1][:6]) and np.array_equal(one[3], got[0][2])
    short = pnp.solve_pnp_ransac_device(frames[0][:3], *BOARD, K, DIST5, **RANSAC)
    assert short[:3] == (False, None, None) and short[3].shape == (3,) and not short[3].any()
    bad = frames[0].copy()
    bad[0, 2] = 16
    with pytest.raises(IndexError):
        pnp.solve_pnp_ransac_device(bad, *BOARD, K, DIST5, **RANSAC)
    with pytest.raises(ValueError):
        pnp.solve_pnp_ransac_device(frames[0], *BOARD, K, np.zeros(12), **RANSAC)
    with pytest.raises(ValueError):
        pnp.solve_pnp_ransac_device(frames[0], *BOARD, K, DIST5, iterations=0)


def hand_built_pool():
    """Frames of the 20x20 board in scrambled pool order -> (frames, expected status, packed pool, B, pool size).  Frame 1 has 300
    rows of which 40 carry a wrong id at least five grid steps from the true one."""
    board = (20, 20, 0.002)
    rng = np.random.default_rng(77)
    big_ids = np.sort(rng.choice(361, 300, replace=False))
    big = _board_frame(rng, big_ids, board, 0.3)
    wrong = rng.choice(300, 40, replace=False)
    for j in wrong:
        gx, gy = int(big[j, 2]) % 19, int(big[j, 2]) // 19
        while True:
            nx, ny = int(rng.integers(0, 19)), int(rng.integers(0, 19))
            if max(abs(nx - gx), abs(ny - gy)) >= 5:
                break
        big[j, 2] = ny * 19 + nx
    big = big[np.argsort(big[:, 2], kind="stable")]                      # a pool holds a frame's rows id-sorted
    frames = [
        _board_frame(rng, np.arange(16) * 7, board, 0.0),                  # 0: OK, clean
        big,                                                               # 1: OK, 300 rows, 40 wrong ids
        _board_frame(rng, np.array([3, 50, 200]), board, 0.0),             # 2: TOO_FEW
        np.zeros((0, 3)),                                                  # 3: TOO_FEW (empty)
        _board_frame(rng, np.arange(10) * 13, board, 0.0),                 # 4: TRUNCATED
        _board_frame(rng, np.arange(12) * 5, board, 0.3),                  # 5: BAD_ID (one id = 361)
        _board_frame(rng, np.arange(19) * 19, board, 0.0),                 # 6: DEGENERATE (a column of the board: no sample)
        _board_frame(rng, np.arange(40, 80), board, 0.3),                  # 7: OK
        _board_frame(rng, np.arange(12) * 23, board, 0.0),                 # 8: NO_CONSENSUS (every corner moved by many px)
    ]
    frames[5][4, 2] = 361
    frames[8][:, :2] += rng.uniform(-40, 40, size=(12, 2)).astype(np.float32)
    expect = [pnp.PNP_OK, pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW, pnp.PNP_TRUNCATED, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE,
              pnp.PNP_OK, pnp.PNP_NO_CONSENSUS]
    order = [7, 8, 1, 0, 6, 3, 5, 2, 4]       # pool order; frame 4 goes last and is cut by the pool size
    B = len(frames)
    pool = sum(len(f) for f in frames) - 3
    packed, _ = pool_cases.lay_frames(frames, pool, order, cell=-7)
    return board, frames, expect, packed, B, pool


def test_pool_hand_built_every_status(dev):
    board, frames, expect, packed, B, pool = hand_built_pool()
    ransac = dict(RANSAC, min_inliers=6)
    d = torch.from_numpy(packed).to(dev)
    counts, starts = packed[:B], packed[B:2 * B]
    tally = [0, 0, 0]
    for refined in (True, False):
        st, pose, info, inl = (t.cpu().numpy() for t in pnp.solve_pnp_ransac_pool(d, B, pool, refined, *board, K, DIST5, **ransac))
        assert st.tolist() == expect, (refined, st.tolist())
        for b in range(B):
            n, s0 = int(counts[b]), int(starts[b])
            mask = inl[s0:min(s0 + n, pool)].astype(bool)
            assert info[b, 0] == mask.sum()                              # the count is the population of the written mask
            if expect[b] in (pnp.PNP_OK, pnp.PNP_NO_CONSENSUS):
                kp = frames[b] if refined else np.c_[np.rint(frames[b][:, :2]).astype(np.int64), frames[b][:, 2].astype(np.int64)]
                _check_frame((int(st[b]), pose[b], mask, int(info[b, 1])), kp, board, K, DIST5, ransac, tally,
                             f"refined={refined} frame {b}")
            else:
                assert not pose[b].any() and not mask.any() and info[b, 1] == -1 and info[b, 0] == 0
        if refined:
            assert info[1, 0] == 260 and 0.1 < pose[1, 6] < 0.5            # the 40 wrong ids are out, rms ~ sigma = 0.3 px
            assert info[0, 0] == 16 and info[7, 0] == 40
    assert tally[0] >= 4, tally


def test_batch_invariance(dev):
    planted = [p[0] for p in planted_frames()]
    kp = planted[0]
    alone = pnp.solve_pnp_ransac_batch_device([kp], *BOARD, K, DIST5, full=True, **RANSAC)[0]
    for at in (0, 7, 31):
        frames = list(planted)
        frames[at], frames[0] = kp, planted[at]
        got = pnp.solve_pnp_ransac_batch_device(frames, *BOARD, K, DIST5, full=True, **RANSAC)[at]
        assert got[0] == alone[0] == pnp.PNP_OK and got[3] == alone[3]
        assert np.array_equal(got[1].view(np.uint64), alone[1].view(np.uint64)) and np.array_equal(got[2], alone[2])


def _pipeline(case, dev, frames):
    from deepcharuco_amd.inference import infer_batch_device
    dc, rn = _models(case, dev)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    pool = 64 * len(frames)
    packed = infer_batch_device(d_frames, case.n_ids, dc, rn, pool=pool)
    cam = np.array([[300.0, 0, frames.shape[2] / 2], [0, 300.0, frames.shape[1] / 2], [0, 0, 1]])
    return packed, pool, cam


def _pool_frames(head, batch, pool):
    """The frames of a refined host pool as [x, y, id] rows in SLOT order (infer_batch_device: raster order), which is the
    order the hypotheses' slots count; unpack_results returns the same rows id-sorted."""
    counts, starts, rows, xy, _ = corner_pool.views(head, batch, pool)
    return [np.c_[xy[s:s + n].astype(np.float64), rows[s:s + n, 2]] for n, s in zip(counts, starts)]


@pytest.mark.parametrize("name", ["board_240x320", "diverse_ids_240x320"])
def test_end_to_end_from_the_corner_pool(dev, name):
    """Plumbing: pool layout, refined xy, slot order of the mask.  The golden weights are synthetic, so the corners lie on no
    board: most frames end in NO_CONSENSUS or with a small consensus, and every one of them is compared in full.  The host
    definition gets each frame's rows as the pool holds them (pool_order=True): slots are what the sampler draws."""
    from deepcharuco_amd.inference import unpack_results
    case = GoldenCase(name)
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1]])
    packed, pool, cam = _pipeline(case, dev, frames)
    outs = [pnp.solve_pnp_ransac_pool(packed, len(frames), pool, True, 5, 5, 0.01, cam, DIST5, seed=E2E_SEED,
                                      reproj_error=thr) for thr in (8.0, 3.0)]          # no sync in between
    head = packed.cpu().numpy()
    res, counts = unpack_results(head, len(frames), pool, True)
    slots = _pool_frames(head, len(frames), pool)
    starts = corner_pool.views(head, len(frames), pool)[1]
    tally = [0, 0, 0]
    for thr, out in zip((8.0, 3.0), outs):
        st, pose, info, inl = (t.cpu().numpy() for t in out)
        for b, kp in enumerate(slots):
            assert sorted(map(tuple, kp)) == sorted(map(tuple, res[b]))          # the unpacked result, before its id sort
            mask = inl[starts[b]:starts[b] + counts[b]].astype(bool)
            assert info[b, 0] == mask.sum()
            _check_frame((int(st[b]), pose[b], mask, int(info[b, 1])), kp, (5, 5, 0.01), cam, DIST5,
                         dict(iterations=100, reproj_error=thr, min_inliers=4, seed=E2E_SEED), tally,
                         f"{name} thr={thr} frame {b}", pool_order=True)
    print("within 1e-9 / stopping-rule fallback / 20-step cap:", tally)


def test_two_runs_and_graph_replay_bit_identical(dev):
    case = GoldenCase("diverse_ids_240x320")
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1]])
    packed, pool, cam = _pipeline(case, dev, frames)
    B = len(frames)
    # two pools in one: the golden frames' own, and the planted frames (poses come out, so the refit is replayed too)
    planted, pb, ppool = corner_pool.pack_keypoints([p[0] for p in planted_frames(8)], dev)
    for pk, b, pl, board, cm in ((packed, B, pool, (5, 5, 0.01), cam), (planted, pb, ppool, BOARD, K)):
        args = (pk, b, pl, True, *board, cm, DIST5)
        eager = pnp.solve_pnp_ransac_pool(*args, **RANSAC)
        again = pnp.solve_pnp_ransac_pool(*args, **RANSAC)
        assert _same(eager, again)
        ws = torch.empty((pnp.ransac_workspace_bytes(b, pl, 100) // 8,), dtype=torch.float64, device=dev)
        out = (torch.full_like(eager[0], -1), torch.full_like(eager[1], -1.0), torch.full_like(eager[2], -9), torch.zeros_like(eager[3]))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):            # warm-up launch outside the capture
            pnp.solve_pnp_ransac_pool(*args, out=out, workspace=ws, **RANSAC)
        torch.cuda.current_stream().wait_stream(s)
        assert _same(eager, out)
        out[0].fill_(-1)
        out[1].fill_(-1.0)
        out[2].fill_(-9)
        out[3].zero_()
        ws.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pnp.solve_pnp_ransac_pool(*args, out=out, workspace=ws, **RANSAC)
        g.replay()
        torch.cuda.synchronize()
        assert _same(eager, out)
    assert (eager[0] == pnp.PNP_OK).all()


def test_frame_stream_ransac_stage(dev):
    from deepcharuco_amd.inference import infer_batch_device
    from deepcharuco_amd.stream import FrameStream
    case = GoldenCase("diverse_ids_240x320")
    dc, rn = _models(case, dev)
    f = case.frame
    frames = np.stack([f, f[::-1], f[:, ::-1], f[::-1, ::-1]] + [np.roll(f, 8 * k, axis=1) for k in range(1, 7)])
    cfg = dict(col_count=5, row_count=5, square_len=0.01, camera_matrix=np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]]),
               dist_coeffs=DIST5)
    ransac = dict(iterations=100, reproj_error=8.0, seed=E2E_SEED)
    batches = [frames[i:i + 4] for i in range(0, 10, 4)]
    with pytest.raises(ValueError):
        FrameStream(case.n_ids, dc, rn, batch=4, height=240, width=320, depth=2, pnp=cfg, pnp_ransac=ransac)
    out = list(FrameStream(case.n_ids, dc, rn, batch=4, height=240, width=320, depth=2, pnp=cfg, pnp_device=True,
                           pnp_ransac=ransac).run(batches))
    assert [o[0] for o in out] == [0, 1, 2] and all(len(o) == 3 for o in out)
    kps = [a for o in out for a in o[1]]
    poses = [p for o in out for p in o[2]]
    assert len(kps) == len(poses) == 10
    # the stage is solve_pnp_ransac_pool on each batch's own corner pool: bit for bit
    want = []
    for fr in batches:
        d = torch.zeros((4, 240, 320), dtype=torch.uint8, device=dev)
        d[:len(fr)] = torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
        packed = infer_batch_device(d, case.n_ids, dc, rn, pool=4 * 64)
        st, pose, info, inl = (t.cpu().numpy() for t in pnp.solve_pnp_ransac_pool(packed, 4, 4 * 64, True, **cfg, **ransac))
        head = packed.cpu().numpy()
        counts, starts, rows, _, _ = corner_pool.views(head, 4, 256)
        want += pnp.unpack_ransac(st, pose, inl, counts, starts, rows[:, 2])[:len(fr)]     # masks in unpack_results' row order
        slot_order = pnp.unpack_ransac(st, pose, inl, counts, starts)
        for b, kp in enumerate(_pool_frames(head, 4, 256)[:len(fr)]):
            assert np.array_equal(slot_order[b][3][np.argsort(kp[:, 2], kind="stable")], want[b - len(fr)][3])
    n_ok = 0
    for kp, (ret, rvec, tvec, mask), (ret_w, rvec_w, tvec_w, mask_w) in zip(kps, poses, want):
        assert ret == ret_w and mask.shape == (len(kp),) and np.array_equal(mask, mask_w)
        if ret:
            n_ok += 1
            assert np.array_equal(rvec, rvec_w) and np.array_equal(tvec, tvec_w) and mask.sum() >= 4
            # the mask speaks of the handed-out (id-sorted) rows: the refit minimised exactly their error, from within 8 px each
            obj = pnp.object_points(kp[mask, 2], 5, 5, 0.01).astype(np.float64)
            e2 = pnp._row_errors2(obj, kp[mask, :2].astype(np.float32).astype(np.float64), np.r_[rvec.ravel(), tvec.ravel()],
                                  cfg["camera_matrix"], pnp._dist(DIST5))
            assert np.sqrt(e2.mean()) <= 8.0
        else:
            assert rvec is None and tvec is None and not mask.any()
    assert n_ok >= 1


def test_c_abi_refuses_bad_arguments(dev):
    from deepcharuco_amd import _lib
    L = _lib.lib()
    E_ARG = -1
    assert L.dcx_error_string(E_ARG)                                     # the code the header calls DCX_E_ARG
    B, pool = 2, 32
    packed = torch.zeros((corner_pool.packed_len(B, pool),), dtype=torch.int32, device=dev)
    st = torch.full((B,), -5, dtype=torch.int32, device=dev)
    pose = torch.full((B, 8), -5.0, dtype=torch.float64, device=dev)
    info = torch.full((B, 2), -5, dtype=torch.int32, device=dev)
    inl = torch.full((pool,), 9, dtype=torch.uint8, device=dev)
    need = L.dcx_solve_pnp_ransac_workspace_bytes(B, pool, 100)
    assert need == B * 100 * 52 + pool * 4 and need % 8 == 0
    assert L.dcx_solve_pnp_ransac_workspace_bytes(0, pool, 100) == 0 and L.dcx_solve_pnp_ransac_workspace_bytes(B, -1, 100) == 0
    assert L.dcx_solve_pnp_ransac_workspace_bytes(B, pool, 0) == 0 and L.dcx_solve_pnp_ransac_workspace_bytes(B, pool, 4097) == 0
    ws = torch.zeros((need // 8,), dtype=torch.float64, device=dev)
    cam = (ctypes.c_double * 9)(*K.ravel().tolist())
    dist = (ctypes.c_double * 8)(*DIST5.tolist(), 0, 0, 0)
    counts_p, starts_p, rows_p, xy_p, _ = corner_pool.ptrs(packed.data_ptr(), B, pool)
    good = dict(counts=counts_p, starts=starts_p, rows=rows_p, xy=xy_p, batch=B, pool=pool, col=5, row=5,
                sq=0.01, cam=cam, dist=dist, n_dist=5, iterations=100, thr=8.0, min_inliers=4, seed=0, ws=ws.data_ptr(), ws_bytes=need,
                st=st.data_ptr(), pose=pose.data_ptr(), info=info.data_ptr(), inl=inl.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return L.dcx_solve_pnp_ransac_pool(a["counts"], a["starts"], a["rows"], a["xy"], a["batch"], a["pool"], a["col"], a["row"],
                                           a["sq"], a["cam"], a["dist"], a["n_dist"], a["iterations"], a["thr"], a["min_inliers"],
                                           a["seed"], a["ws"], a["ws_bytes"], a["st"], a["pose"], a["info"], a["inl"],
                                           _lib.current_stream())

    skew = (ctypes.c_double * 9)(*K.ravel().tolist())
    skew[1] = 1.0
    for kw in (dict(counts=None), dict(starts=None), dict(rows=None), dict(cam=None), dict(st=None), dict(pose=None), dict(info=None),
               dict(ws=None), dict(batch=0), dict(pool=-1), dict(col=1), dict(row=1), dict(n_dist=12), dict(n_dist=5, dist=None),
               dict(cam=skew), dict(sq=float("inf")), dict(iterations=0), dict(iterations=4097), dict(thr=0.0), dict(thr=-1.0),
               dict(thr=float("nan")), dict(thr=float("inf")), dict(ws_bytes=need - 8), dict(ws=ws.data_ptr() + 4)):
        assert call(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert (st == -5).all() and (pose == -5.0).all() and (info == -5).all() and (inl == 9).all()      # nothing was launched
    # and the accepted call, on two empty frames (the mask may be NULL; the integer rows may stand in for xy)
    assert call(inl=None, xy=None) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [pnp.PNP_TOO_FEW] * 2 and not pose.any() and info.tolist() == [[0, -1], [0, -1]] and (inl == 9).all()
