"""dcx_calibrate_uncertainty_pool (csrc/dcx_calib_cov.hip) against its definition, calib.calibration_uncertainty_host and
fisheye.calibration_uncertainty_fisheye_host, on the MI355X.

Host and device are given the SAME solution (the host calibration's), so only the order of the sums differs between them.  The
gate is tests/test_calib_cov_host.py's: 1000 * cond(S) * 2^-52, the forward error of inverting a matrix of that condition in
float64 with three digits of room; cond(S) is computed by the test from the host's cov_intrinsics (sigma^2 S^-1 has S's condition).
Covariance entries are compared relative to sqrt(c_ii c_jj), standard deviations relative to themselves, sigma^2 to 1e-12 relative;
dof, points, views and the status must be equal.  Every scene carries 0.3 px of noise: on noise-free float32 pixels the residuals
are differences of ~300 px values that round to 1e-5 px, and their sum of squares carries 1e-8 of rounding, not 1e-12
(tests/test_gpu_calib.py says the same of the rms)."""
import ctypes

import numpy as np
import pytest
import torch

import camera_exact as cx
import fisheye_exact as fx
from deepcharuco_amd import _lib, calib, corner_pool, fisheye as fe, pnp
from test_calib_cov_host import FE_DIST, FE_K, SIGMA, _same_bits, renoised, solved
from test_calib_host import BOARD, DIST_TRUE, K_TRUE, SIZE, make_views
from test_gpu_calib import STRIDE_BOARD, _hand_built_pool, _kps

pytestmark = pytest.mark.gpu

REL_SIGMA2 = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _gate(h):
    return 1000.0 * float(np.linalg.cond(h.cov_intrinsics)) * 2.0 ** -52


def _rel_cov(d, h):
    """max |d - h| / sqrt(h_ii h_jj) over the entries of [..., n, n] covariances (0 for none)."""
    s = np.sqrt(np.diagonal(h, axis1=-2, axis2=-1))
    scale = s[..., :, None] * s[..., None, :]
    return float(np.max(np.abs(d - h) / scale)) if h.size else 0.0


def _compare(d, h, name, used=None):
    """Device against host CalibUncertainty at the gate of the module docstring -> the measured gaps."""
    assert (d.status, d.dof, d.points, d.views) == (h.status, h.dof, h.points, h.views), (name, d[:5], h[:5])
    assert d.status == calib.COV_OK, name
    used = np.arange(len(h.std_extrinsics)) if used is None else np.asarray(used)
    unused = np.setdiff1d(np.arange(len(h.std_extrinsics)), used)
    assert not d.cov_extrinsics[unused].any() and not d.std_extrinsics[unused].any(), name
    gate = _gate(h)
    gaps = {"sigma2": abs(d.sigma2 - h.sigma2) / h.sigma2,
            "cov_intrinsics": _rel_cov(d.cov_intrinsics, h.cov_intrinsics),
            "cov_extrinsics": _rel_cov(d.cov_extrinsics[used], h.cov_extrinsics[used]),
            "std_intrinsics": float(np.max(np.abs(d.std_intrinsics - h.std_intrinsics) / h.std_intrinsics)),
            "std_extrinsics": float(np.max(np.abs(d.std_extrinsics[used] - h.std_extrinsics[used]) / h.std_extrinsics[used]))}
    print(f"{name}: gate {gate:.3g}, device - host gaps {gaps}")
    assert gaps["sigma2"] <= REL_SIGMA2, (name, gaps)
    assert max(v for k, v in gaps.items() if k != "sigma2") <= gate, (name, gaps, gate)
    assert np.array_equal(d.cov_intrinsics, d.cov_intrinsics.T) and np.array_equal(d.cov_extrinsics, d.cov_extrinsics.transpose(0, 2, 1))
    return gaps


def _model(K, dist, view_status, poses6):
    """-> the explicit ``result_or_model`` tuple: view_status [B], pose [B, 8] with (rvec, tvec) in its first six words."""
    pose = np.zeros((len(poses6), 8))
    pose[:, :6] = poses6
    return K, dist, np.asarray(view_status, np.int32), pose


def _small_noisy_views(seed=336):
    """Four views of eight rows each at 0.3 px: make_views' full views cut to eight of their ids (not on one line)."""
    objs, imgs, ids_l, _ = make_views(seed, 4, sigma=SIGMA, partial=False)
    rng = np.random.default_rng([seed, 8])
    for i in range(4):
        while True:
            sel = np.sort(rng.choice(len(ids_l[i]), 8, replace=False))
            g = objs[i][sel, :2].astype(np.float64)
            if np.linalg.matrix_rank(g - g.mean(0), tol=1e-6) == 2:
                break
        objs[i], imgs[i], ids_l[i] = objs[i][sel], imgs[i][sel], ids_l[i][sel]
    return objs, imgs, ids_l


def test_four_views_of_eight_rows(dev):
    objs, imgs, ids_l = _small_noisy_views()
    h = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert h.status == calib.CALIB_OK and h.points_used == 32
    hu = calib.calibration_uncertainty_host(objs, imgs, h)
    assert hu.dof == 31
    _compare(calib.calibration_uncertainty_device(_kps(imgs, ids_l), *BOARD, h), hu, "4 views of 8 rows")


def _chunk_views(seed, rows=(63, 64, 65, 129)):
    """Six views of the 130-id board at 0.3 px: two full ones and four redrawn at their true poses to ``rows`` ids (in general
    position): one short of, exactly at and one past the evaluate kernel's 64-row LDS chunk, and one past two chunks."""
    objs, imgs, ids_l, poses = cx.calib_views(seed, 6, SIGMA, board=STRIDE_BOARD)
    rng = np.random.default_rng([seed, 1])
    N = cx.n_ids(STRIDE_BOARD)
    for i, n in zip((1, 2, 3, 5), rows):
        while True:
            ids = np.sort(rng.choice(N, n, replace=False))
            g = cx.grid_xy(ids, STRIDE_BOARD[1]).astype(np.float64)
            if np.linalg.matrix_rank(g - g.mean(0)) == 2:
                break
        obj = cx.board_points(ids, *STRIDE_BOARD)
        img = cx.f64(cx.project(obj, poses[i], cx.CALIB_K, cx.CALIB_DIST)) + rng.normal(scale=SIGMA, size=(n, 2))
        objs[i], imgs[i], ids_l[i] = obj, img.astype(np.float32), ids
    return objs, imgs, ids_l


def test_row_counts_at_the_lds_chunk(dev):
    objs, imgs, ids_l = _chunk_views(32)
    assert [len(i) for i in ids_l] == [130, 63, 64, 65, 130, 129]
    h = calib.calibrate_camera_host_full(objs, imgs, cx.CALIB_SIZE)
    assert h.status == calib.CALIB_OK and h.views_used == 6
    _compare(calib.calibration_uncertainty_device(_kps(imgs, ids_l), *STRIDE_BOARD, h),
             calib.calibration_uncertainty_host(objs, imgs, h), "63 / 64 / 65 / 129 / 130 rows")


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
@pytest.mark.parametrize("batch", [1, 7, 8, 9])
def test_batches_around_the_reduction_slices(dev, model, batch):
    """The first ``batch`` views of a solved 24-view calibration, at its solution: 1, 7, 8 and 9 views against reduce_invert's 8
    slices.  (One view alone leaves S with a condition of 1e9 to 1e12; the gate follows it.)"""
    objs, imgs, r = solved(model, 24)
    board, host, device = ((BOARD, calib.calibration_uncertainty_host, calib.calibration_uncertainty_device) if model == "pinhole"
                           else (fx.BOARD, fe.calibration_uncertainty_fisheye_host, fe.calibration_uncertainty_fisheye_device))
    ids_l = [_ids_of(o, board) for o in objs[:batch]]
    m = _model(r.camera_matrix, r.dist_coeffs, r.view_status[:batch], np.c_[r.rvecs, r.tvecs][:batch])
    hu = host(objs[:batch], imgs[:batch], r.camera_matrix, r.dist_coeffs, r.rvecs[:batch], r.tvecs[:batch])
    _compare(device(_kps(imgs[:batch], ids_l), *board, m), hu, f"{model}, {batch} views")


def _ids_of(obj, board):
    """Board points -> their ids (the inverse of pnp.object_points)."""
    col, row, sq = board
    g = np.rint(np.asarray(obj, np.float64)[:, :2] / sq).astype(np.int64) - 1
    ids = g[:, 1] * (row - 1) + g[:, 0]
    assert np.array_equal(pnp.object_points(ids, *board), obj)
    return ids


def test_1025_views(dev):
    """41 distinct views laid 25 times: the optimum of the 1,025 is the optimum of the 41, so the host calibrates 41."""
    objs, imgs, ids_l, _ = make_views(530, 41, sigma=SIGMA)
    h = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert h.status == calib.CALIB_OK and h.views_used == 41
    objs, imgs, ids_l = objs * 25, imgs * 25, ids_l * 25
    poses = np.tile(np.c_[h.rvecs, h.tvecs], (25, 1))
    m = _model(h.camera_matrix, h.dist_coeffs, np.zeros(1025, np.int32), poses)
    hu = calib.calibration_uncertainty_host(objs, imgs, h.camera_matrix, h.dist_coeffs, poses[:, :3], poses[:, 3:])
    assert hu.views == 1025
    _compare(calib.calibration_uncertainty_device(_kps(imgs, ids_l), *BOARD, m), hu, "1,025 views")


@pytest.mark.parametrize("refined", [True, False])
def test_pool_with_every_view_status(dev, refined):
    """test_gpu_calib's hand-built pool: views in scrambled order with gaps, used ones between three rows, an empty view, a bad id,
    collinear points and a view cut by the pool's end.  Refined xy and the integer rows."""
    kps, packed, B, pool, expect = _hand_built_pool(7)
    use = [b for b in range(B) if expect[b] in (pnp.PNP_OK, pnp.PNP_DEGENERATE, pnp.PNP_TOO_FEW)]   # what the host can take
    objs = [pnp.object_points(kps[b][:, 2], *BOARD) for b in use]
    imgs = [kps[b][:, :2].astype(np.float32) if refined else np.rint(kps[b][:, :2]).astype(np.float32) for b in use]
    h = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    assert h.status == calib.CALIB_OK and h.view_status.tolist() == [expect[b] for b in use]
    hu = calib.calibration_uncertainty_host(objs, imgs, h)
    poses = np.zeros((B, 6))
    poses[use] = np.c_[h.rvecs, h.tvecs]
    g, p = calib.calibration_uncertainty_pool(torch.from_numpy(packed).to(dev), B, pool, refined, *BOARD,
                                              _model(h.camera_matrix, h.dist_coeffs, expect, poses))
    d = calib.unpack_uncertainty(g, p)
    ok = [b for b in range(B) if expect[b] == pnp.PNP_OK]
    sub = d._replace(std_extrinsics=d.std_extrinsics[use], cov_extrinsics=d.cov_extrinsics[use])
    assert not d.cov_extrinsics[[b for b in range(B) if b not in ok]].any()
    _compare(sub, hu, f"hand-built pool refined={refined}", used=[use.index(b) for b in ok])


def test_fisheye_with_unused_views(dev):
    objs, imgs, r = solved("fisheye", 8)
    st = r.view_status.copy()
    st[[0, 6]] = pnp.PNP_DEGENERATE
    ids_l = [_ids_of(o, fx.BOARD) for o in objs]
    hu = fe.calibration_uncertainty_fisheye_host(objs, imgs, r.camera_matrix, r.dist_coeffs, r.rvecs, r.tvecs, view_status=st)
    d = fe.calibration_uncertainty_fisheye_device(_kps(imgs, ids_l), *fx.BOARD,
                                                  _model(r.camera_matrix, r.dist_coeffs, st, np.c_[r.rvecs, r.tvecs]))
    assert d.std_intrinsics.shape == (8,) and d.cov_intrinsics.shape == (8, 8)
    _compare(d, hu, "fisheye, 6 of 8 views", used=[1, 2, 3, 4, 5, 7])
    _compare(fe.calibration_uncertainty_fisheye_device(_kps(imgs, ids_l), *fx.BOARD, r),
             fe.calibration_uncertainty_fisheye_host(objs, imgs, r), "fisheye, a CalibResult in")


# ------------------------------------------------------------------------------------------------ masks

def _bits(dev_pair):
    return tuple(t.cpu().numpy().tobytes() for t in dev_pair)


@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_masks_give_the_bits_of_the_compacted_pool(dev, model):
    objs, imgs, r = solved(model, 8)
    board, pool_fn = (BOARD, calib.calibration_uncertainty_pool) if model == "pinhole" else (fx.BOARD, fe.calibration_uncertainty_fisheye_pool)
    kps = _kps(imgs, [_ids_of(o, board) for o in objs])
    rng = np.random.default_rng(11)
    masks = [rng.random(len(k)) < 0.8 for k in kps]
    masks[3][:] = True
    assert all(m.sum() >= 6 for m in masks) and not all(m.all() for m in masks)
    m = _model(r.camera_matrix, r.dist_coeffs, r.view_status, np.c_[r.rvecs, r.tvecs])
    packed, b, pool = corner_pool.pack_keypoints(kps, dev)
    cut, b2, pool2 = corner_pool.pack_keypoints([k[s] for k, s in zip(kps, masks)], dev)
    masked = pool_fn(packed, b, pool, True, *board, m, inliers=masks)             # (ids are sorted: slot order is the row order)
    removed = pool_fn(cut, b2, pool2, True, *board, m)
    assert _bits(masked) == _bits(removed)
    u = calib.unpack_uncertainty(*masked, 9 if model == "pinhole" else 8)
    assert u.status == calib.COV_OK and u.points == sum(int(s.sum()) for s in masks)
    ones = torch.ones(pool, dtype=torch.uint8, device=dev)
    assert _bits(pool_fn(packed, b, pool, True, *board, m, inliers=ones)) == _bits(pool_fn(packed, b, pool, True, *board, m))
    assert _bits(masked) != _bits(pool_fn(packed, b, pool, True, *board, m))


def test_mask_from_the_robust_calibration(dev):
    """Planted mislabels: the d_inliers of calibrate_charuco_ransac_pool go straight into the uncertainty, which must give the bits
    of the same call on a pool without the rejected rows, and meet the host at the gate."""
    objs, imgs, ids_l, _ = make_views(91, 8, sigma=SIGMA)
    kps = _kps(imgs, ids_l)
    for b in (1, 4):                                                  # two rows of two views carry another corner's pixels
        kps[b][[2, 3], :2] = kps[b][[3, 2], :2]
    packed, B, pool = corner_pool.pack_keypoints(kps, dev)
    inl = torch.zeros(pool, dtype=torch.uint8, device=dev)
    rr = calib.calibrate_charuco_ransac_pool(packed, B, pool, True, *BOARD, SIZE, out_inliers=inl)
    assert rr.status == calib.CALIB_OK and rr.views_used == 8 and 0 < int(rr.view_inliers.sum()) < pool
    by_tensor = calib.calibration_uncertainty_pool(packed, B, pool, True, *BOARD, rr, inliers=inl)
    assert _bits(by_tensor) == _bits(calib.calibration_uncertainty_pool(packed, B, pool, True, *BOARD, rr))   # its own masks
    cut, b2, pool2 = corner_pool.pack_keypoints([k[m] for k, m in zip(kps, rr.inliers)], dev)
    plain = calib.CalibResult(*rr[:13])
    assert _bits(by_tensor) == _bits(calib.calibration_uncertainty_pool(cut, b2, pool2, True, *BOARD, plain))
    d = calib.unpack_uncertainty(*by_tensor)
    assert d.points == rr.points_used == int(rr.view_inliers.sum())
    hu = calib.calibration_uncertainty_host([pnp.object_points(k[:, 2], *BOARD) for k in kps], [k[:, :2].astype(np.float32) for k in kps], rr)
    _compare(d, hu, "masks of the robust calibration")
    _same_bits(calib.calibration_uncertainty_device(kps, *BOARD, rr), d)


# ------------------------------------------------------------------------------------------------ determinism and capture

def test_two_calls_and_a_captured_graph_give_the_same_bits(dev):
    objs, imgs, r = solved("pinhole", 24)
    kps = _kps(imgs, [_ids_of(o, BOARD) for o in objs])
    packed, B, pool = corner_pool.pack_keypoints(kps, dev)
    st = torch.from_numpy(r.view_status.astype(np.int32)).to(dev)
    pose = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    pose[:, :6] = torch.from_numpy(np.c_[r.rvecs, r.tvecs]).to(dev)
    mask = torch.ones(pool, dtype=torch.uint8, device=dev)
    mask[::7] = 0
    m = (r.camera_matrix, r.dist_coeffs, st, pose)
    ws = torch.empty(calib.uncertainty_workspace_bytes(B), dtype=torch.uint8, device=dev)
    out = (torch.empty(calib.COV_GLOBAL_WORDS, dtype=torch.float64, device=dev),
           torch.empty((B, calib.COV_POSE_WORDS), dtype=torch.float64, device=dev))

    def call():
        return calib.calibration_uncertainty_pool(packed, B, pool, True, *BOARD, m, inliers=mask, workspace=ws, out=out)

    eager = _bits(call())
    assert calib.unpack_uncertainty(*out).status == calib.COV_OK
    assert _bits(call()) == eager
    ws.fill_(0x7F)
    assert _bits(call()) == eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # a synchronising call would fail here
        call()
    for _ in range(2):
        out[0].fill_(-1.0)
        out[1].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(out) == eager


# ------------------------------------------------------------------------------------------------ what the numbers mean

def test_standard_deviations_predict_the_spread_of_recalibrations(dev):
    """Monte-Carlo on the device: the 24 clean views of make_views(524, ...) re-noised 120 times at 0.3 px, each calibrated by
    calibrate_charuco_device; the empirical standard deviation of the nine intrinsics and of view 0's pose over the draws against
    the standard deviations predicted from the first draw alone.  All 15 ratios in [0.80, 1.25]: a condition, not a tolerance (the
    1-sigma sampling error of a standard deviation from 120 draws is 6.5 %, so +-3 sigma).  The host definition gives 0.918 to 1.051
    on this scene."""
    objs, ids_l, draws = renoised(120)
    thetas, pose0, first = [], [], None
    for imgs in draws:
        kps = _kps(imgs, ids_l)
        r = calib.calibrate_charuco_device(kps, *BOARD, SIZE)
        assert r.status == calib.CALIB_OK and r.views_used == 24
        if first is None:
            first = calib.calibration_uncertainty_device(kps, *BOARD, r)
        K = r.camera_matrix
        thetas.append(np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], r.dist_coeffs.ravel()])
        pose0.append(np.r_[r.rvecs[0], r.tvecs[0]])
    assert first.status == calib.COV_OK and first.dof == 1483
    ratios = np.r_[np.std(thetas, axis=0, ddof=1) / first.std_intrinsics, np.std(pose0, axis=0, ddof=1) / first.std_extrinsics[0]]
    print("empirical / predicted standard deviation: intrinsics", np.round(ratios[:9], 3).tolist(), "view 0's pose",
          np.round(ratios[9:], 3).tolist())
    assert ratios.shape == (15,) and ratios.min() >= 0.80 and ratios.max() <= 1.25, ratios


# ------------------------------------------------------------------------------------------------ statuses and refusals

def _zero_but_counts(u):
    assert u.sigma2 == 0.0 and not u.std_intrinsics.any() and not u.cov_intrinsics.any()
    assert not u.std_extrinsics.any() and not u.cov_extrinsics.any()


def test_statuses(dev):
    objs, imgs, ids_l, poses = make_views(77, 2, sigma=0.0, f32=False, partial=False)
    five = [0, 6, 24, 42, 48]
    k5 = [np.c_[m[five], i[five]] for m, i in zip(imgs, ids_l)]
    ok = np.zeros(2, np.int32)
    u = calib.calibration_uncertainty_device(k5, *BOARD, _model(K_TRUE, DIST_TRUE, ok, poses))
    assert (u.status, u.dof, u.points, u.views) == (calib.COV_NO_DOF, -1, 10, 2)
    _zero_but_counts(u)
    kps = _kps(imgs, ids_l)
    u = calib.calibration_uncertainty_device(kps, *BOARD, _model(K_TRUE, DIST_TRUE, [pnp.PNP_TOO_FEW, pnp.PNP_DEGENERATE], poses))
    assert (u.status, u.points, u.views) == (calib.COV_NO_VIEWS, 0, 0)
    _zero_but_counts(u)
    back = poses.copy()
    back[1, 5] = -back[1, 5]                                          # the board behind the camera
    u = calib.calibration_uncertainty_device(kps, *BOARD, _model(K_TRUE, DIST_TRUE, ok, back))
    assert (u.status, u.points, u.views) == (calib.COV_SINGULAR, 98, 2) and u.dof == 2 * 98 - 9 - 12
    _zero_but_counts(u)
    nan = poses.copy()
    nan[0, 1] = np.nan
    u = calib.calibration_uncertainty_device(kps, *BOARD, _model(K_TRUE, DIST_TRUE, ok, nan))
    assert u.status == calib.COV_SINGULAR
    _zero_but_counts(u)
    u = calib.calibration_uncertainty_device(kps, *BOARD, _model(K_TRUE, DIST_TRUE, ok, poses))
    assert u.status == calib.COV_OK and (u.std_intrinsics > 0).all() and (u.std_extrinsics > 0).all()
    for n in (4, 8):
        with pytest.raises(ValueError, match="held fixed"):
            calib.calibration_uncertainty_device(kps, *BOARD, _model(K_TRUE, np.zeros(n), ok, poses))
    with pytest.raises(ValueError, match="held fixed"):
        fe.calibration_uncertainty_fisheye_device(kps, *BOARD, _model(K_TRUE, DIST_TRUE, ok, poses))


def test_a_used_view_whose_slots_leave_the_pool_is_not_read(dev):
    """The hand-built pool's last view is cut by the pool's end; called used, it makes the call DCX_COV_SINGULAR."""
    kps, packed, B, pool, expect = _hand_built_pool(7)
    st = np.array(expect, np.int32)
    st[B - 1] = pnp.PNP_OK
    g, p = calib.calibration_uncertainty_pool(torch.from_numpy(packed).to(dev), B, pool, True, *BOARD,
                                              _model(K_TRUE, DIST_TRUE, st, np.tile(np.r_[0.1, 0.2, 0.0, 0.0, 0.0, 0.3], (B, 1))))
    u = calib.unpack_uncertainty(g, p)
    assert u.status == calib.COV_SINGULAR and u.views == expect.count(pnp.PNP_OK) + 1
    assert u.points == sum(len(kps[b]) for b in range(B) if expect[b] == pnp.PNP_OK)
    _zero_but_counts(u)


def test_abi_refusals(dev):
    L = _lib.lib()
    objs, imgs, r = solved("pinhole", 8)
    kps = _kps(imgs, [_ids_of(o, BOARD) for o in objs])
    packed, B, pool = corner_pool.pack_keypoints(kps, dev)
    ptrs = corner_pool.ptrs(packed.data_ptr(), B, pool)[:4]
    need = L.dcx_calibrate_uncertainty_workspace_bytes(B)
    assert need > 0 and L.dcx_calibrate_uncertainty_workspace_bytes(0) == 0 and need < L.dcx_calibrate_uncertainty_workspace_bytes(B + 1)
    assert need == calib.uncertainty_workspace_bytes(B)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    pose = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    pose[:, :6] = torch.from_numpy(np.c_[r.rvecs, r.tvecs]).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    g = torch.full((calib.COV_GLOBAL_WORDS,), -7.0, dtype=torch.float64, device=dev)
    p = torch.full((B, calib.COV_POSE_WORDS), -7.0, dtype=torch.float64, device=dev)
    K = r.camera_matrix
    th = (ctypes.c_double * 9)(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *r.dist_coeffs.ravel().tolist())
    s = _lib.current_stream()

    def call(ptrs=ptrs, batch=B, pool=pool, board=BOARD, model=0, th=th, st=st.data_ptr(), pose=pose.data_ptr(), mask=None,
             ws=ws.data_ptr(), nbytes=need, g=g.data_ptr(), p=p.data_ptr()):
        return L.dcx_calibrate_uncertainty_pool(*ptrs, batch, pool, *board, model, th, st, pose, mask, ws, nbytes, g, p, s)

    E_ARG, E_WS = -1, -3
    assert call(model=2) == E_ARG and call(model=-1) == E_ARG
    for kw in ("th", "st", "pose", "ws", "g", "p"):
        assert call(**{kw: None}) == E_ARG, kw
    assert call(ptrs=(None,) + ptrs[1:]) == E_ARG and call(batch=0) == E_ARG and call(board=(1, 8, 0.02)) == E_ARG
    assert call(nbytes=need - 1) == E_WS and call(nbytes=0) == E_WS
    torch.cuda.synchronize()
    assert bool((g == -7.0).all()) and bool((p == -7.0).all())        # a refused call writes nothing
    assert call() == 0 and call(ptrs=ptrs[:3] + (None,)) == 0          # (d_xy NULL: the integer rows)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_pool(packed, B, pool, True, *BOARD, r, workspace=ws[:need - 8])
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_pool(packed, B, pool, True, *BOARD, r, inliers=torch.ones(pool, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_pool(packed, B, pool, True, *BOARD, (r.camera_matrix, r.dist_coeffs, st[:3], pose))
