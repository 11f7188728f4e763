"""The device side of the fisheye model (csrc/dcx_fisheye.hip through deepcharuco_amd/fisheye.py) against its host definitions:
pose (test_gpu_pnp.py's gates), calibration (test_gpu_calib.py's gates), the undistort + rectify map (test_gpu_rectify.py's tie
rule), the remap through a fisheye map (bit for bit) and the corner pool in rectified coordinates.  Scenes are
tests/fisheye_exact.py's.  Host and device differ in fp64 summation order and in libm's last bits (atan, tan); every test prints
the gaps it measured."""
import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_exact as fx
import pool_cases
from camera_exact import f64
from deepcharuco_amd import calib, corner_pool, fisheye as fe, pnp, rectify as rc
from test_gpu_calib import _check
from test_gpu_pnp import _agree, _rel

pytestmark = pytest.mark.gpu

K150 = fx.camera(150.0, 152.0, off=(4.0, -3.0))
K400 = fx.camera(400.0, 395.0, off=(4.0, -3.0))
BIG = (14, 11, 0.015)                      # 13 x 10 = 130 ids: frames of 129 rows
MID = (11, 8, 0.02)                        # 10 x 7 = 70 ids: views of 63, 64, 65 rows
SQ32 = float(np.float32(0.03))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ pose

def on_axis_frame(K, k):
    """A fronto-parallel view whose corner 0 stands on the optical axis: it projects to (cx, cy).  The board is turned by 0.3 rad
    about that axis, which keeps it fronto-parallel: at rvec = 0 the gate's |d rvec| / |rvec| would divide rounding by rounding."""
    obj = cx.board_points(np.arange(28), *fx.BOARD)
    r = np.array([0.0, 0.0, 0.3])
    p = np.r_[r, np.array([0.0, 0.0, 0.2]) - f64(cx.rotation(r)) @ np.array([SQ32, SQ32, 0.0])]
    img = f64(fx.project(obj, p, K, k)).astype(np.float32)
    assert img[0, 0] == K[0, 2] and img[0, 1] == K[1, 2]
    return np.c_[img.astype(np.float64), np.arange(28)], p


def wide_frame(K, k):
    """The camera 3 cm above corner 0, tilted by 2 degrees: the far corners stand at about 80 degrees from the axis."""
    obj = cx.board_points(np.arange(28), *fx.BOARD)
    r = np.array([np.deg2rad(2.0), 0.0, 0.0])
    p = np.r_[r, np.array([0.0, 0.0, 0.03]) - f64(cx.rotation(r)) @ np.array([SQ32, SQ32, 0.0])]
    img = f64(fx.project(obj, p, K, k)).astype(np.float32)
    return np.c_[img.astype(np.float64), np.arange(28)], p, np.degrees(fx.theta_max(obj, p))


def _pose_check(frames, board, K, k, dev, name):
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    st, pose = fe.solve_pnp_fisheye_pool(packed, b, pool, True, *board, K, k)
    st2, pose2 = fe.solve_pnp_fisheye_pool(packed, b, pool, True, *board, K, k)
    assert torch.equal(st, st2) and np.array_equal(pose.cpu().numpy().view(np.uint64), pose2.cpu().numpy().view(np.uint64))
    st, pose = st.cpu().numpy(), pose.cpu().numpy()
    tally, worst = [0, 0, 0], 0.0
    for i, kp in enumerate(frames):
        hs, hp = fe.solve_pnp_fisheye_host_full(kp, *board, K, k)
        assert st[i] == hs, (name, i, st[i], hs)
        if hs == pnp.PNP_OK:
            worst = max(worst, _rel(pose[i], hp))
            _agree(pose[i], hp, tally)
        else:
            assert not pose[i].any()
    print(f"{name}: worst relative pose gap {worst:.3e}; within 1e-9 / stopping-rule fallback / 20-step cap: {tally}")
    return st, pose, tally


@pytest.mark.parametrize("K,k", [(K150, fx.K_LENS), (K400, fx.K_ZERO)], ids=["f150_k", "f400_k0"])
def test_pose_row_counts_at_the_lane_stride(dev, K, k):
    rows = [4, 5, 63, 64, 65, 129]
    _, imgs, ids_l, _ = fx.make_views(21, len(rows), K, k, board=BIG, rows=rows)
    frames = fx.keypoints(imgs, ids_l)
    assert [len(f) for f in frames] == rows
    st, pose, tally = _pose_check(frames, BIG, K, k, dev, "rows 4 5 63 64 65 129")
    assert (st == pnp.PNP_OK).all() and tally[0] >= 5
    got = fe.solve_pnp_fisheye_batch_device(frames, *BIG, K, k)
    assert all(g[0] is True and np.array_equal(np.r_[g[1].ravel(), g[2].ravel()], pose[i, :6]) for i, g in enumerate(got))
    one = fe.solve_pnp_fisheye_device(frames[2], *BIG, K, k)
    assert one[0] is True and np.array_equal(one[1].ravel(), pose[2, :3])
    assert fe.solve_pnp_fisheye_device(frames[0][:3], *BIG, K, k) == (False, None, None)
    with pytest.raises(ValueError):
        fe.solve_pnp_fisheye_device(frames[0], *BIG, K, np.zeros(5))


def test_pose_on_the_axis_and_at_80_degrees(dev):
    for K, k in ((K150, fx.K_LENS), (K150, fx.K_ZERO)):
        axis, p_axis = on_axis_frame(K, k)
        wide, p_wide, deg = wide_frame(K, k)
        assert 78.0 < deg < 83.0
        st, pose, tally = _pose_check([axis, wide], fx.BOARD, K, k, dev, f"on-axis corner and {deg:.1f} degrees, k1 {k[0]}")
        assert (st == pnp.PNP_OK).all() and tally[0] == 2
        for got, want in ((pose[0], p_axis), (pose[1], p_wide)):          # and the truth, to the float32 pixels
            assert np.linalg.norm(got[3:6] - want[3:]) <= 1e-4 * np.linalg.norm(want[3:]) and got[6] <= 2e-5


def test_pose_pool_with_every_status_and_graph_replay(dev):
    K, k = K150, fx.K_LENS
    _, imgs, ids_l, _ = fx.make_views(22, 4, K, k)
    fr = fx.keypoints(imgs, ids_l)
    outside = fr[1].copy()
    outside[5, :2] = (639.0, 240.0)                      # theta_d = 2.1: no theta below pi / 2 gives it
    bad = fr[2].copy()
    bad[3, 2] = 28
    line = np.c_[np.linspace(100, 300, 4), np.linspace(100, 250, 4), np.arange(4)]       # ids 0..3: one board line
    frames = [fr[0], fr[0][:3], np.zeros((0, 3)), fr[3], bad, line, outside, fr[1]]
    expect = [pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_TOO_FEW, pnp.PNP_TRUNCATED, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE,
              pnp.PNP_DEGENERATE, pnp.PNP_OK]
    order = [7, 1, 0, 6, 2, 5, 4, 3]
    pool = sum(len(f) for f in frames) - 3               # frame 3 goes last and is cut
    packed, _ = pool_cases.lay_frames(frames, pool, order, cell=-7)
    d = torch.from_numpy(packed).to(dev)
    B = len(frames)
    for refined in (True, False):
        st, pose = fe.solve_pnp_fisheye_pool(d, B, pool, refined, *fx.BOARD, K, k)
        st_h, pose_h = st.cpu().numpy(), pose.cpu().numpy()
        assert st_h.tolist() == expect, refined
        assert not pose_h[[1, 2, 3, 4, 5, 6]].any()
        tally = [0, 0, 0]
        for b in (0, 7):
            kp = frames[b] if refined else np.c_[np.rint(frames[b][:, :2]), frames[b][:, 2]]
            _agree(pose_h[b], fe.solve_pnp_fisheye_host_full(kp, *fx.BOARD, K, k)[1], tally)
        assert tally[0] + tally[1] == 2
    # one call under graph replay equals the eager call
    out = (torch.full_like(st, -1), torch.full_like(pose, -1.0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fe.solve_pnp_fisheye_pool(d, B, pool, False, *fx.BOARD, K, k, out=out)
    torch.cuda.current_stream().wait_stream(s)
    out[0].fill_(-1)
    out[1].fill_(-1.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fe.solve_pnp_fisheye_pool(d, B, pool, False, *fx.BOARD, K, k, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], st)
    assert np.array_equal(out[1].cpu().numpy().view(np.uint64), pose.cpu().numpy().view(np.uint64))


# ------------------------------------------------------------------------------------------------ calibration

def _truth(d, K, k, poses, name):
    """Against the exact scene: the bound the host definition meets (test_fisheye_host.py: float32 pixels)."""
    gk, gd = np.abs(d.camera_matrix - K).max(), np.abs(d.dist_coeffs.ravel() - k).max()
    print(f"{name}: against the truth |K - K*| {gk:.3e} px, |k - k*| {gd:.3e}, rms {d.rms:.3e} px")
    assert gk <= 1e-3 and gd <= 1e-4 and d.rms <= 2e-5
    assert np.all(np.linalg.norm(d.tvecs - poses[:, 3:], axis=1) <= 1e-5 * np.linalg.norm(poses[:, 3:], axis=1))


@pytest.mark.parametrize("seed,n_views,sigma,K,k,focal0", [(101, 8, 0.0, K150, fx.K_LENS, None), (102, 64, 0.3, K150, fx.K_LENS, None),
                                                          (103, 8, 0.0, K400, fx.K_ZERO, 300.0), (104, 9, 0.0, K150, fx.K_LENS, None)])
def test_calibration_matches_host(dev, seed, n_views, sigma, K, k, focal0):
    """Nine views put two views into reduce_solve's slice 0 (8 slices), so the serial adds inside a slice run; 8, 64 and 7 views
    never do that at NG = 8.  The noisy 64-view set is taken through the 150 px lens, whose corners reach 56 degrees.  Through the 400 px lens (38 degrees
    at the most) it is not a case: the column of k4 goes with theta^9, 0.027 at 0.67 rad against 0.83 at 0.98 rad, and runs nearly
    parallel to k3's, so k3 and k4 are weakly observed, host and device walk that flat valley a different number of steps (host
    11 steps / 30 attempts, device 15 / 36) and end 2.5e-7 apart in k while agreeing to 5.3e-10 in K, 8.5e-9 in rvec and 5.6e-16 in
    the rms (0.395 px): test_gpu_calib.py's finding about conditioning at a narrow field, not about a kernel."""
    objs, imgs, ids_l, poses = fx.make_views(seed, n_views, K, k, sigma=sigma)
    h = fe.calibrate_fisheye_host_full(objs, imgs, fx.SIZE, focal0)
    d = fe.calibrate_fisheye_device(fx.keypoints(imgs, ids_l), *fx.BOARD, fx.SIZE, focal0)
    assert d.dist_coeffs.shape == (1, 4)
    _check(d, h, f"{n_views} views sigma {sigma} focal0 {focal0}", rms_floor=1e-12 if sigma == 0.0 else 0.0)
    if sigma == 0.0:
        _truth(d, K, k, poses, f"{n_views} views")


def test_smallest_scene_and_a_rejected_step(dev):
    """4 views of 8 rows, at a seed where the host definition alone rejects steps: the device must report rejected steps too,
    so the retry launch (Schur, reduce, trial and decide without an evaluate) has run."""
    objs, imgs, ids_l, _ = fx.make_views(334, 4, K150, fx.K_LENS, rows=8)
    h = fe.calibrate_fisheye_host_full(objs, imgs, fx.SIZE)
    assert h.status == calib.CALIB_OK and h.attempts > h.iterations        # a condition on the input
    d = fe.calibrate_fisheye_device(fx.keypoints(imgs, ids_l), *fx.BOARD, fx.SIZE)
    assert d.attempts > d.iterations, (d.iterations, d.attempts)
    _check(d, h, "4 views of 8 rows", rms_floor=1e-12)


def test_calibration_row_counts_at_the_staging_stride(dev):
    rows = [63, 64, 65, 70, 63, 64, 65, 70]
    objs, imgs, ids_l, poses = fx.make_views(31, 8, K150, fx.K_LENS, board=MID, rows=rows)
    h = fe.calibrate_fisheye_host_full(objs, imgs, fx.SIZE)
    d = fe.calibrate_fisheye_device(fx.keypoints(imgs, ids_l), *MID, fx.SIZE)
    _check(d, h, "rows 63 64 65 70", rms_floor=1e-12)
    assert d.view_points.tolist() == rows
    _truth(d, K150, fx.K_LENS, poses, "rows 63 64 65 70")


def test_calibration_every_view_status_same_bits_and_argument_errors(dev):
    K, k = K150, fx.K_LENS
    objs, imgs, ids_l, _ = fx.make_views(41, 7, K, k, sigma=0.2)
    kps = fx.keypoints(imgs, ids_l)
    bad = kps[5].copy()
    bad[1, 2] = 28
    outside = kps[6].copy()
    outside[2, :2] = (1200.0, 240.0)                     # theta_d = 2.75 at the start camera (f = 320): beyond pi / 2
    line = np.c_[np.linspace(100, 300, 4), np.linspace(100, 250, 4), np.arange(4)]
    views = kps[:5] + [kps[0][:3], bad, line, outside, kps[4].copy()]
    expect = [pnp.PNP_OK] * 5 + [pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID, pnp.PNP_DEGENERATE, pnp.PNP_DEGENERATE, pnp.PNP_TRUNCATED]
    B = len(views)
    order = list(np.random.default_rng(5).permutation(B - 1)) + [B - 1]
    pool = sum(len(v) + 3 for v in views) - 3 - 4
    packed, _ = pool_cases.lay_frames(views, pool, order, gap=3, filler=-9)
    dp = torch.from_numpy(packed).to(dev)
    d = fe.calibrate_fisheye_pool(dp, B, pool, True, *fx.BOARD, fx.SIZE)
    d2 = fe.calibrate_fisheye_pool(dp, B, pool, True, *fx.BOARD, fx.SIZE)
    assert d.view_status.tolist() == expect and d.view_points.tolist() == [len(v) for v in views]
    for x, y in zip(d, d2):                                                   # two calls: the same bits
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    use = [b for b in range(B) if expect[b] in (pnp.PNP_OK, pnp.PNP_TOO_FEW, pnp.PNP_DEGENERATE)]      # what the host can take
    h = fe.calibrate_fisheye_host_full([pnp.object_points(views[b][:, 2], *fx.BOARD) for b in use],
                                       [views[b][:, :2].astype(np.float32) for b in use], fx.SIZE)
    assert h.view_status.tolist() == [expect[b] for b in use]
    sel = np.array(use)
    _check(d._replace(view_status=d.view_status[sel], rvecs=d.rvecs[sel], tvecs=d.tvecs[sel], view_rms=d.view_rms[sel],
                      view_points=d.view_points[sel]), h, "every view status")
    assert not d.rvecs[5:].any()
    with pytest.raises(IndexError):
        fe.calibrate_fisheye_device([v for v in views[:7]], *fx.BOARD, fx.SIZE)
    with pytest.raises(ValueError):
        fe.calibrate_fisheye_device(kps, *fx.BOARD, (0, 480))
    with pytest.raises(ValueError):
        fe.calibrate_fisheye_device([], *fx.BOARD, fx.SIZE)
    with pytest.raises(ValueError):
        fe.calibrate_fisheye_device(kps, *fx.BOARD, fx.SIZE, focal0=np.inf)
    r = fe.calibrate_fisheye_device([v[:3] for v in kps], *fx.BOARD, fx.SIZE)
    assert r.status == calib.CALIB_NO_VIEWS and (r.view_status == pnp.PNP_TOO_FEW).all() and r.rms == 0.0


# ------------------------------------------------------------------------------------------------ map, remap, points

R100 = f64(cx.rotation([0.0, np.deg2rad(100.0), 0.0]))
R_SMALL = f64(cx.rotation([0.02, -0.03, 0.01]))
P_WIDE = np.array([[20.0, 0, 32.0], [0, 20.0, 24.0], [0, 0, 1]])
P_NEW = np.array([[120.0, 0, 160.0, 0], [0, 120.0, 120.0, 0], [0, 0, 1, 0]])
MAPS = [("1x1", K150, fx.K_LENS, None, None, 1, 1), ("R and P omitted, 67 wide", K150, fx.K_LENS, None, None, 67, 5),
        ("R and P given", K150, fx.K_LENS, R_SMALL, P_NEW, 320, 240), ("sentinel regions", K150, fx.K_LENS, R100, P_WIDE, 64, 48),
        ("k = 0", K400, fx.K_ZERO, R_SMALL, None, 130, 33)]


def _map_agrees(dev, K, k, R, P, w, h, name):
    """test_gpu_rectify.py's rule: entries may differ by 1, and only where the host's unquantised 32 m lies within 1e-6 of a
    half-integer; the count differing is at most the count near a tie, which is at most 1 % of the entries (checked on the host
    alone)."""
    host = fe.undistort_rectify_map_fisheye_host(K, k, R, P, w, h)
    m32 = 32.0 * fe.undistort_rectify_map_fisheye_host(K, k, R, P, w, h, quantised=False)
    with np.errstate(invalid="ignore"):
        near = np.abs(m32 - np.floor(m32) - 0.5) < 1e-6
    assert near.sum() <= max(0.01 * host.size, 0), (name, int(near.sum()))
    got = fe.undistort_rectify_map_fisheye_device(K, k, R, P, w, h, device=dev)
    assert got.dtype == torch.int32 and tuple(got.shape) == (h, w, 2)
    got_h = got.cpu().numpy()
    differ = host != got_h
    assert np.array_equal(host == rc.MAP_SENTINEL, got_h == rc.MAP_SENTINEL), name
    assert not (differ & ~near).any(), (name, int((differ & ~near).sum()))
    assert np.abs(host.astype(np.int64) - got_h)[differ].max(initial=0) <= 1, name
    print(f"{name}: {int(differ.sum())} of {host.size} entries differ, {int(near.sum())} near a tie, "
          f"{int((host[..., 0] == rc.MAP_SENTINEL).sum())} sentinels")
    assert differ.sum() <= near.sum()
    return host, got


@pytest.mark.parametrize("name,K,k,R,P,w,h", MAPS, ids=[m[0] for m in MAPS])
def test_map_device_matches_host(dev, name, K, k, R, P, w, h):
    host, got = _map_agrees(dev, K, k, R, P, w, h, name)
    if name == "sentinel regions":
        out = host == rc.MAP_SENTINEL
        assert out.any() and not out.all()
    pre = torch.full((h, w, 2), 7, dtype=torch.int32, device=dev)
    assert fe.undistort_rectify_map_fisheye_device(K, k, R, P, w, h, out=pre) is pre and torch.equal(pre, got)


def test_remap_through_a_fisheye_map_bit_for_bit(dev):
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (3, 480, 640), dtype=np.uint8)
    for R, P, w, h in ((R_SMALL, P_NEW, 320, 240), (R100, P_WIDE, 64, 48)):
        m = fe.undistort_rectify_map_fisheye_device(K150, fx.K_LENS, R, P, w, h, device=dev)
        got = rc.remap_device(torch.from_numpy(src).to(dev), m, 7)
        assert np.array_equal(got.cpu().numpy(), rc.remap_host(src, m.cpu().numpy(), 7))


@pytest.mark.parametrize("refined", [True, False])
def test_rectified_points_match_host(dev, refined):
    K, k = K150, fx.K_LENS
    _, imgs, ids_l, _ = fx.make_views(51, 5, K, k)
    frames = fx.keypoints(imgs, ids_l)
    frames[1][4, :2] = (639.0, 240.0)                    # outside the model: NaN
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    _, starts, rows, xy = corner_pool.views(packed.cpu().numpy(), b, pool)[:4]
    pix = xy.astype(np.float64) if refined else rows[:, :2].astype(np.float64)
    for R, P in ((None, None), (R_SMALL, P_NEW), (R100, P_WIDE)):
        want = fe.rectify_points_fisheye_host(pix, K, k, R, P)
        got = fe.rectify_points_fisheye_pool(packed, b, pool, refined, K, k, R, P).cpu().numpy()
        assert got.shape == (pool, 2) and np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want[:, 0])
        gap = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
        print(f"refined {refined} R {'given' if R is not None else 'omitted'}: {int((~ok).sum())} NaN rows, gap {gap:.3e} px")
        assert np.isnan(want).any() and gap <= 1e-9                          # test_gpu_rectify.py's gate
