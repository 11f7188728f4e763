"""The device calibration with cv2's flags and the rational model (csrc/dcx_calib_flags.hip through deepcharuco_amd/calib.py)
against its host definition, calibrate_camera_host_full with ``flags``.

Flagged 9-parameter calls run dcx_calibrate_pool's per-view kernels and are held to tests/test_gpu_calib.py's gates, restated here:
intrinsics 1e-8 relative (to fx), distortion 1e-8 absolute, poses 1e-8 relative, rms 1e-12 relative with the absolute 1e-12 px floor
on noise-free sets (there the rms is the float32 rounding of the image points and a residual's own fp64 rounding is 7e-14 px).
Their scene is the wide lens of the rational tests with five coefficients, camera_exact.calib_views without its fronto-parallel
views (``wide_views``), because those gates need a scene at which the definition reproduces itself: run on the views in reverse
order, the host differs from itself by up to 2.5e-7 in the distortion on test_calib_host.make_views' narrow field (k3 sits in a
flat valley there, and FIX_K4, which changes nothing, measures 1.1e-8 on the 64-view set), by up to 1.2e-6 relative in the rvec of
calib_views' fronto-parallel views (|rvec| ~ 0), and by at most 7.4e-10 in any gated quantity on the scenes used here (all eleven
flag sets, both sizes, measured on the host alone; the aspect ratio given is 0.975 for a truth of 230 / 236, since a ratio 0.5 %
off leaves a biased fit that the host reproduces only to 9.5e-9).

Rational models are compared by where they project, never coefficient by coefficient.  The quantity: the largest distance in px
between the positions two solutions give every used row, plus the difference of their rms.  The gate is set in the test against
the reference's own spread: the host definition run on the views in the given order and in reverse order (two accumulation orders
of the same sums; no code under test).  The device may differ from the host by max(10 x that spread, 1e-9 px): 10 x because two
orders sample the rounding spread once and the device is a third order; 1e-9 px is 1e4 times the fp64 rounding of a 300 px residual
and 1e3 times tighter than what the 1e-8 parameter gates allow in the image.  Every test prints both numbers."""
import numpy as np
import pytest
import torch

import camera_exact as cx
import pool_cases
from deepcharuco_amd import calib, pnp
from test_calib_flags_host import ALONE, RAT_DIST, RAT_K, RAT_SIZE, RAT_TZ, TOGETHER, bits, positions, rational_views, theta12
from test_calib_host import BOARD, SIZE, make_views

pytestmark = pytest.mark.gpu

F = calib
REL_K, ABS_DIST, REL_POSE, REL_RMS = 1e-8, 1e-8, 1e-8, 1e-12
G = F.CALIB_USE_INTRINSIC_GUESS
R = F.CALIB_RATIONAL_MODEL
WIDE_BOARD = cx.CALIB_BOARD
WIDE_DIST = np.array([0.12, -0.05, 8e-4, -5e-4, 0.01])             # the wide lens with a denominator of 1
K_RATIO = np.array([[0.975, 0, 0], [0, 1.0, 0], [0, 0, 1]])        # only fx / fy is read without a guess; the truth is 230 / 236


def wide_views(seed, n_views, sigma=0.0):
    """``n_views`` tilted views of the wide lens: camera_exact.calib_views without every fourth, fronto-parallel one."""
    total = n_views + (n_views + 2) // 3
    objs, imgs, ids_l, poses = cx.calib_views(seed, total, sigma, K=RAT_K, dist=WIDE_DIST, tz=RAT_TZ)
    keep = [i for i in range(total) if i % 4][:n_views]
    assert len(keep) == n_views
    return [objs[i] for i in keep], [imgs[i] for i in keep], [ids_l[i] for i in keep], poses[keep]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _kps(imgs, ids_l):
    return [np.c_[m.astype(np.float64), i] for m, i in zip(imgs, ids_l)]


def _gaps(d, h):
    """Device vs host CalibResult -> the measured gaps (used views only); test_gpu_calib.py's."""
    used = np.flatnonzero(h.view_status == pnp.PNP_OK)

    def rel(a, b):
        return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1))) if len(b) else 0.0
    return {"K": float(np.abs(d.camera_matrix - h.camera_matrix).max() / h.camera_matrix[0, 0]),
            "dist": float(np.abs(d.dist_coeffs - h.dist_coeffs).max()),
            "rvec": rel(d.rvecs[used], h.rvecs[used]), "tvec": rel(d.tvecs[used], h.tvecs[used]),
            "rms": abs(d.rms - h.rms) / h.rms if h.rms else abs(d.rms),
            "view_rms": float(np.max(np.abs(d.view_rms[used] - h.view_rms[used]) / np.maximum(h.view_rms[used], 1e-300)))}


def _same_views(d, h, name):
    assert d.view_status.tolist() == h.view_status.tolist(), name
    assert d.status == h.status == calib.CALIB_OK, (name, d.status, h.status)
    assert (d.views_used, d.points_used) == (h.views_used, h.points_used)
    assert d.view_points.tolist() == h.view_points.tolist()
    assert d.flags == h.flags and d.dist_coeffs.shape == h.dist_coeffs.shape
    unused = np.flatnonzero(d.view_status != pnp.PNP_OK)
    assert not d.rvecs[unused].any() and not d.tvecs[unused].any() and not d.view_rms[unused].any()


def _check(d, h, name, rms_floor=0.0):
    """test_gpu_calib.py's check of a 9-parameter solution, with its gates."""
    _same_views(d, h, name)
    g = _gaps(d, h)
    print(f"{name}: device - host gaps {g}; steps / attempts device {d.iterations} / {d.attempts}, host {h.iterations} / "
          f"{h.attempts}")
    assert g["K"] <= REL_K and g["dist"] <= ABS_DIST, (name, g)
    assert g["rvec"] <= REL_POSE and g["tvec"] <= REL_POSE, (name, g)
    floor = g["rms"] > REL_RMS
    assert not floor or abs(d.rms - h.rms) <= rms_floor, (name, g, d.rms, h.rms)
    if floor:
        print(f"{name}: rms gate absolute {rms_floor} px (float32 floor)")


def _distance(a, b, objs, imgs):
    """The comparison quantity of two solutions (module docstring), px."""
    pa, pb = positions(a, objs, imgs), positions(b, objs, imgs)
    return float(np.linalg.norm(pa - pb, axis=1).max()) + abs(a.rms - b.rms)


def _reversed(r):
    return r._replace(view_status=r.view_status[::-1], rvecs=r.rvecs[::-1], tvecs=r.tvecs[::-1], view_rms=r.view_rms[::-1],
                      view_points=r.view_points[::-1])


def _check_by_position(d, objs, imgs, size, name, **kw):
    """The device's solution against the host's by position, the gate from the host's own spread -> the host's result."""
    h = calib.calibrate_camera_host_full(objs, imgs, size, **kw)
    hr = _reversed(calib.calibrate_camera_host_full(objs[::-1], imgs[::-1], size, **kw))
    assert hr.view_status.tolist() == h.view_status.tolist() and hr.status == h.status
    _same_views(d, h, name)
    spread, gap = _distance(hr, h, objs, imgs), _distance(d, h, objs, imgs)
    gate = max(10 * spread, 1e-9)
    print(f"{name}: host forward - host reversed {spread:.3g} px, device - host {gap:.3g} px (gate {gate:.3g}); rms device {d.rms!r} "
          f"host {h.rms!r}; steps / attempts device {d.iterations} / {d.attempts}, host {h.iterations} / {h.attempts}, "
          f"reversed {hr.iterations} / {hr.attempts}")
    assert gap <= gate, (name, gap, spread)
    return h


def _bit_equal(a, b):
    assert len(a) == len(b) and a.flags == b.flags
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


# ---------------------------------------------------------------------------------------------------- flags = 0, 9-parameter flags

def test_flags_zero_is_todays_call(dev):
    objs, imgs, ids_l, _ = make_views(201, 12, sigma=0.3)
    a = calib.calibrate_charuco_device(_kps(imgs, ids_l), *BOARD, SIZE)
    b = calib.calibrate_charuco_device(_kps(imgs, ids_l), *BOARD, SIZE, flags=0)
    assert a.status == calib.CALIB_OK and a.flags == 0
    _bit_equal(a, b)


@pytest.fixture(scope="module")
def sets():
    return {(8, 0.0): wide_views(101, 8, 0.0), (64, 0.3): wide_views(102, 64, 0.3)}


@pytest.mark.parametrize("n_views,sigma", [(8, 0.0), (64, 0.3)])
@pytest.mark.parametrize("flags", ALONE + [TOGETHER], ids=hex)
def test_flagged_nine_parameter_calls_match_the_host(dev, sets, flags, n_views, sigma):
    objs, imgs, ids_l, _ = sets[n_views, sigma]
    kw = dict(flags=flags, camera_matrix=K_RATIO)
    h = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, **kw)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE, **kw)
    _check(d, h, f"flags {flags:#x}, {n_views} views sigma {sigma}", rms_floor=1e-12 if sigma == 0.0 else 0.0)
    fm = calib._flag_model(flags, K_RATIO, None)
    _, start, _ = calib._initialise_flags(calib._views(objs, imgs), RAT_SIZE, fm)
    fixed = ~fm.free
    if fm.aspect is not None:
        fixed[0] = False
        assert d.camera_matrix[0, 0] == (K_RATIO[0, 0] / K_RATIO[1, 1]) * d.camera_matrix[1, 1]
    if flags & F.CALIB_FIX_FOCAL_LENGTH:
        # the start is the device's own least squares over the views, equal to the host's to rounding and not to the bit; the
        # bits of a fixed focal length are pinned with a guess (test_guess_with_every_intrinsic_fixed)
        fixed[:2] = False
        assert np.abs(theta12(d)[:2] - start[:2]).max() <= REL_K * start[0]
    assert np.array_equal(bits(theta12(d)[fixed]), bits(start[fixed])), (theta12(d), start)
    assert np.array_equal(bits(theta12(d)[fixed]), bits(theta12(h)[fixed]))


def test_two_calls_give_the_same_bits(dev):
    objs, imgs, ids_l, _ = wide_views(104, 48, 0.5)
    kw = dict(flags=TOGETHER | F.CALIB_FIX_ASPECT_RATIO, camera_matrix=K_RATIO)
    a = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE, **kw)
    b = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE, **kw)
    assert a.status == calib.CALIB_OK
    _bit_equal(a, b)
    objs, imgs, ids_l, _ = rational_views(16, 0.3)
    a = calib.calibrate_charuco_device(_kps(imgs, ids_l), *cx.CALIB_BOARD, RAT_SIZE, flags=R)
    b = calib.calibrate_charuco_device(_kps(imgs, ids_l), *cx.CALIB_BOARD, RAT_SIZE, flags=R)
    assert a.status == calib.CALIB_OK and a.dist_coeffs.shape == (1, 8)
    _bit_equal(a, b)


# ---------------------------------------------------------------------------------------------------- the rational model

@pytest.mark.parametrize("n_views,sigma", [(8, 0.0), (16, 0.0), (16, 0.3)])
def test_rational_model_matches_the_host_by_position(dev, n_views, sigma):
    """The three rational sets of DESIGN 3.9c; at sigma = 0.3 both sides reach the 30-step cap."""
    objs, imgs, ids_l, _ = rational_views(n_views, sigma)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *cx.CALIB_BOARD, RAT_SIZE, flags=R)
    h = _check_by_position(d, objs, imgs, RAT_SIZE, f"rational, {n_views} views sigma {sigma}", flags=R)
    if sigma:
        assert h.iterations == d.iterations == calib.CALIB_MAX_ITER
    else:
        assert d.rms <= 2e-5


def test_rational_rejected_steps_are_retried(dev):
    """The 16 noise-free views reject steps on the host (20 accepted in 36 attempts): the device must report rejected steps too,
    so the retry launch of the NG = 12 kernels (schur, reduce_solve, trial, decide without an evaluate) has run."""
    objs, imgs, ids_l, _ = rational_views(16, 0.0)
    h = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, flags=R)
    assert h.status == calib.CALIB_OK and h.attempts > h.iterations        # a condition on the input
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *cx.CALIB_BOARD, RAT_SIZE, flags=R)
    assert d.status == calib.CALIB_OK and d.attempts > d.iterations, (d.iterations, d.attempts)


def _cut(objs, imgs, ids_l, which, n, board, seed):
    """The views ``which`` cut to ``n`` of their rows each, ids in general position (not on one line)."""
    rng = np.random.default_rng([seed, n])
    for i in which:
        while True:
            sel = np.sort(rng.choice(len(ids_l[i]), n, replace=False))
            g = cx.grid_xy(ids_l[i][sel], board[1]).astype(np.float64)
            if np.linalg.matrix_rank(g - g.mean(0)) == 2:
                break
        objs[i], imgs[i], ids_l[i] = objs[i][sel], imgs[i][sel], ids_l[i][sel]
    return objs, imgs, ids_l


def test_rational_views_of_four_rows(dev):
    """Four of the sixteen views carry four rows: one lane in sixteen of the evaluate has a row, and a view's 6x6 block rests on
    eight residuals.  Four rows leave the pose of a planar target two-fold ambiguous, and a draw whose start falls into the other
    pose ends at 0.3 px on these noise-free views, on the host as anywhere: the draw used is one at which the host reaches the
    float32 floor, which is asserted as a condition on the input."""
    objs, imgs, ids_l, _ = rational_views(16, 0.0)
    objs, imgs, ids_l = _cut(objs, imgs, ids_l, (2, 5, 10, 15), 4, cx.CALIB_BOARD, 41)
    assert sorted(len(i) for i in ids_l)[:4] == [4] * 4
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *cx.CALIB_BOARD, RAT_SIZE, flags=R)
    h = _check_by_position(d, objs, imgs, RAT_SIZE, "rational, four views of four rows", flags=R)
    assert h.rms <= 2e-5                                                    # a condition on the input


STRIDE_BOARD = (11, 14, 0.012)                  # 10 x 13 = 130 ids (test_gpu_calib.py's)
STRIDE_ROWS = (63, 64, 65, 127, 128, 129, 130)


def test_rational_row_counts_at_the_evaluate_stride(dev):
    """test_gpu_calib.test_row_counts_at_the_evaluate_stride for the NG = 12 evaluate (LDS stride 21): 16 noise-free views of the
    130-id board under the rational truth, the twelve tilted ones with 63 .. 130 rows in turn, the four full ones with 130."""
    objs, imgs, ids_l, poses = cx.calib_views(31, 16, 0.0, board=STRIDE_BOARD, K=RAT_K, dist=RAT_DIST, tz=RAT_TZ)
    rng = np.random.default_rng([31, 1])
    N, tilted = cx.n_ids(STRIDE_BOARD), 0
    for i in range(16):
        if i % 4 == 0:
            continue
        n = STRIDE_ROWS[tilted % len(STRIDE_ROWS)]
        tilted += 1
        while True:
            ids = np.sort(rng.choice(N, n, replace=False))
            g = cx.grid_xy(ids, STRIDE_BOARD[1]).astype(np.float64)
            if np.linalg.matrix_rank(g - g.mean(0)) == 2:
                break
        obj = cx.board_points(ids, *STRIDE_BOARD)
        objs[i], imgs[i], ids_l[i] = obj, cx.f64(cx.project(obj, poses[i], RAT_K, RAT_DIST)).astype(np.float32), ids
    rows = [130 if i % 4 == 0 else STRIDE_ROWS[(i - i // 4 - 1) % len(STRIDE_ROWS)] for i in range(16)]
    assert [len(i) for i in ids_l] == rows
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *STRIDE_BOARD, RAT_SIZE, flags=R)
    h = _check_by_position(d, objs, imgs, RAT_SIZE, "rational, row counts", flags=R)
    assert h.views_used == 16 and h.view_points.tolist() == rows


@pytest.mark.parametrize("n_ok", [5, 8, 9])
def test_rational_batches_with_unusable_views_in_between(dev, n_ok):
    """5, 8 and 9 usable views with a three-row view and a view with an id outside the board between them: every slice of
    reduce_solve's view sum (4 slices at NG = 12) meets a skipped view and an uneven tail."""
    objs, imgs, ids_l, _ = rational_views(n_ok, 0.0)
    kps = _kps(imgs, ids_l)
    bad = kps[2].copy()
    bad[1, 2] = cx.n_ids(cx.CALIB_BOARD)
    kps.insert(1, kps[0][:3].copy())                                                   # TOO_FEW
    kps.insert(4, bad)                                                                 # BAD_ID
    B = len(kps)
    pool = sum(len(k) + 2 for k in kps)
    packed, _ = pool_cases.lay_frames(kps, pool, gap=2, filler=-9)
    d = calib.calibrate_charuco_pool(torch.from_numpy(packed).to(dev), B, pool, True, *cx.CALIB_BOARD, RAT_SIZE, flags=R)
    expect = [pnp.PNP_OK] * B
    expect[1], expect[4] = pnp.PNP_TOO_FEW, pnp.PNP_BAD_ID
    assert d.view_status.tolist() == expect and d.view_points.tolist() == [len(k) for k in kps]
    use = [b for b in range(B) if b != 4]                                              # what the host can take
    sel = np.array(use)
    sub = d._replace(view_status=d.view_status[sel], rvecs=d.rvecs[sel], tvecs=d.tvecs[sel], view_rms=d.view_rms[sel],
                     view_points=d.view_points[sel])
    ho = [pnp.object_points(kps[b][:, 2], *cx.CALIB_BOARD) for b in use]
    hi = [kps[b][:, :2].astype(np.float32) for b in use]
    _check_by_position(sub, ho, hi, RAT_SIZE, f"rational, {n_ok} usable views of {B}", flags=R)
    assert not d.rvecs[[1, 4]].any() and not d.view_rms[[1, 4]].any()


# ---------------------------------------------------------------------------------------------------- the guess start

def test_guess_from_the_truth(dev):
    objs, imgs, ids_l, _ = wide_views(63, 12)
    kw = dict(flags=G, camera_matrix=RAT_K, dist_coeffs=WIDE_DIST)
    h = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, **kw)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE, **kw)
    _check(d, h, "guess from the truth", rms_floor=1e-12)
    assert d.rms <= 2e-5 and d.iterations <= 10


def test_guess_from_a_wrong_camera(dev):
    objs, imgs, ids_l, _ = wide_views(64, 64, 0.3)
    K = RAT_K.copy()
    K[:2] *= 1.05
    kw = dict(flags=G, camera_matrix=K, dist_coeffs=WIDE_DIST)
    h = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, **kw)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE, **kw)
    _check(d, h, "guess 5 % off")
    plain = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE)
    g = _gaps(d, plain)
    print("guess 5 % off against the device call without a guess:", g)
    assert g["K"] <= REL_K and g["dist"] <= ABS_DIST


def test_guess_with_eight_coefficients_holds_k4_k5_k6_live(dev):
    """An 8-coefficient guess without RATIONAL_MODEL: the 12-parameter kernels run with k4 k5 k6 fixed at the bits given, and they
    are live in the projection: the noise-free views of the rational truth are met at the float32 floor, which nothing with a
    denominator of 1 reaches on these pixels (0.013 px at best)."""
    objs, imgs, ids_l, _ = rational_views(8, 0.0)
    d8 = RAT_DIST.copy()
    d8[:5] *= 1.1                                                       # the numerator is off, the denominator is the truth's
    K = RAT_K.copy()
    K[:2] *= 1.02
    kw = dict(flags=G, camera_matrix=K, dist_coeffs=d8)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *cx.CALIB_BOARD, RAT_SIZE, **kw)
    _check_by_position(d, objs, imgs, RAT_SIZE, "8-coefficient guess, k4 k5 k6 held", **kw)
    assert d.dist_coeffs.shape == (1, 8) and np.array_equal(bits(d.dist_coeffs.ravel()[5:]), bits(d8[5:]))
    assert d.rms <= 2e-5


def test_guess_with_every_intrinsic_fixed(dev):
    objs, imgs, ids_l, _ = wide_views(65, 6, 0.3)
    flags = (G | F.CALIB_FIX_FOCAL_LENGTH | F.CALIB_FIX_PRINCIPAL_POINT | F.CALIB_FIX_K1 | F.CALIB_FIX_K2 | F.CALIB_FIX_K3
             | F.CALIB_ZERO_TANGENT_DIST)
    K = RAT_K.copy()
    K[0, 0] *= 1.01
    kw = dict(flags=flags, camera_matrix=K, dist_coeffs=WIDE_DIST)
    h = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, **kw)
    d = calib.calibrate_charuco_device(_kps(imgs, ids_l), *WIDE_BOARD, RAT_SIZE, **kw)
    _check(d, h, "every intrinsic fixed")
    want = np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], WIDE_DIST[:2], 0.0, 0.0, WIDE_DIST[4]]
    assert np.array_equal(bits(theta12(d)[:9]), bits(want)) and np.array_equal(bits(theta12(h)[:9]), bits(want))
    assert d.rvecs.any() and d.iterations >= 1


def test_device_argument_errors(dev):
    objs, imgs, ids_l, _ = make_views(106, 4)
    kps = _kps(imgs, ids_l)
    with pytest.raises(ValueError):
        calib.calibrate_charuco_device(kps, *BOARD, SIZE, flags=0x100)
    with pytest.raises(ValueError):
        calib.calibrate_charuco_device(kps, *BOARD, SIZE, flags=G)
    bad = [k.copy() for k in kps]
    bad[2][0, 2] = 49
    with pytest.raises(IndexError):
        calib.calibrate_charuco_device(bad, *BOARD, SIZE, flags=F.CALIB_FIX_K3)
    for flags in (F.CALIB_FIX_K3, R, G):
        r = calib.calibrate_charuco_device([k[:3] for k in kps], *BOARD, SIZE, flags=flags, camera_matrix=RAT_K)
        assert r.status == calib.CALIB_NO_VIEWS and (r.view_status == pnp.PNP_TOO_FEW).all() and r.rms == 0.0 and r.flags == flags
        assert not r.camera_matrix.any() and not r.dist_coeffs.any()
