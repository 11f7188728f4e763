"""The calibration flags and the rational model on the host (deepcharuco_amd/calib.py: calibrate_camera_host_full with ``flags``,
``camera_matrix``, ``dist_coeffs``), the definition dcx_calibrate_flags_pool is pinned against: flags = 0 is the old call, the
12-column Jacobian against central differences, the masked and aspect-folded block elimination against a dense solve, every flag
alone and three together (fixed entries keep their bits, fx = a fy exactly, the free gradient vanishes), the guess start, the
rational scene, and what is refused (Python and the C entry, without a GPU).

Rational models are compared by where they project, never coefficient by coefficient: numerator and denominator trade against each
other, and on noisy views the coefficients wander while the projection does not."""
import ctypes

import numpy as np
import pytest

import camera_exact as cx
from deepcharuco_amd import calib, pnp
from test_calib_host import BOARD, DIST_TRUE, K_TRUE, SIZE, make_views

F = calib
# the wide-lens scene: a 100 degree pinhole lens with all eight coefficients, image points over 150-500 x 97-400 px
RAT_K = np.array([[230.0, 0, 319.3], [0, 236.0, 238.1], [0, 0, 1]])
RAT_DIST = np.array([0.35, -0.08, 8e-4, -5e-4, 0.01, 0.7, 0.05, -0.01])
RAT_SIZE = (640, 480)
RAT_TZ = (0.10, 0.16)

ALONE = [F.CALIB_FIX_ASPECT_RATIO, F.CALIB_FIX_PRINCIPAL_POINT, F.CALIB_ZERO_TANGENT_DIST, F.CALIB_FIX_FOCAL_LENGTH, F.CALIB_FIX_K1,
         F.CALIB_FIX_K2, F.CALIB_FIX_K3, F.CALIB_FIX_K4, F.CALIB_FIX_K5, F.CALIB_FIX_K6]
TOGETHER = F.CALIB_FIX_K3 | F.CALIB_ZERO_TANGENT_DIST | F.CALIB_FIX_PRINCIPAL_POINT
K_RATIO = np.array([[0.98, 0, 0], [0, 1.0, 0], [0, 0, 1]])      # only fx / fy is read without a guess; the truth is 400 / 410


def rational_views(n_views, sigma, seed=7):
    return cx.calib_views(seed, n_views, sigma, K=RAT_K, dist=RAT_DIST, tz=RAT_TZ)


def theta12(r):
    """A CalibResult -> theta12."""
    d = np.zeros(8)
    d[:r.dist_coeffs.size] = r.dist_coeffs.ravel()
    return np.r_[r.camera_matrix[0, 0], r.camera_matrix[1, 1], r.camera_matrix[0, 2], r.camera_matrix[1, 2], d]


def positions(r, objs, imgs):
    """Where a solution projects every row of its used views (px), the views in order."""
    th = theta12(r)
    out = []
    for i in np.flatnonzero(r.view_status == pnp.PNP_OK):
        o, m = objs[i].astype(np.float64), imgs[i].astype(np.float64)
        out.append(calib._project_full12(o, m, th, np.r_[r.rvecs[i], r.tvecs[i]], False)[0] + m)
    return np.concatenate(out, 0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_flags_zero_is_todays_call():
    objs, imgs, _, _ = make_views(61, 8, sigma=0.3)
    a = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    b = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=0)
    assert a._fields == b._fields and a.flags == b.flags == 0
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
        else:
            assert x == y
    assert calib.calibrate_camera_host(objs, imgs, SIZE, flags=0)[0] == a.rms


def test_rational_jacobian_matches_finite_differences():
    """All 12 intrinsic columns at a model whose k4 k5 k6 are not zero; the gate of test_calib_host's 9-column check."""
    objs, imgs, _, poses = rational_views(3, 0.3)
    theta = np.r_[RAT_K[0, 0], RAT_K[1, 1], RAT_K[0, 2], RAT_K[1, 2], RAT_DIST]
    assert theta[9:].all()
    o, m = objs[1].astype(np.float64), imgs[1].astype(np.float64)
    _, _, J = calib._project_full12(o, m, theta, poses[1], True)
    assert J.shape == (2 * len(o), 18)
    for j in range(12):
        h = 1e-6 * max(1.0, abs(theta[j]))
        d = np.zeros(12)
        d[j] = h
        fd = (calib._project_full12(o, m, theta + d, poses[1], False)[0]
              - calib._project_full12(o, m, theta - d, poses[1], False)[0]).ravel() / (2 * h)
        assert np.abs(fd - J[:, j]).max() <= 1e-6 * max(np.abs(J[:, j]).max(), 1.0), j
    # with the denominator at 1 the first nine columns are the 9-parameter model's
    t9 = np.r_[theta[:9], 0, 0, 0]
    J9 = calib._project_full(o, m, t9[:9], poses[1], True)[2]
    J12 = calib._project_full12(o, m, t9, poses[1], True)[2]
    assert np.array_equal(J12[:, :9], J9[:, :9]) and np.array_equal(J12[:, 12:], J9[:, 9:])


def _map(free, aspect):
    """The flags' linear map on the intrinsic columns as a matrix: J' = J T."""
    T = np.diag(free.astype(np.float64))
    if aspect is not None:
        T[0, 1] = aspect
    return T


@pytest.mark.parametrize("flags,lg", [(F.CALIB_FIX_K3 | F.CALIB_ZERO_TANGENT_DIST, -1), (F.CALIB_FIX_ASPECT_RATIO, 2),
                                      (F.CALIB_RATIONAL_MODEL | F.CALIB_FIX_ASPECT_RATIO | F.CALIB_FIX_K5, 0),
                                      (F.CALIB_RATIONAL_MODEL | F.CALIB_FIX_PRINCIPAL_POINT, -1)])
def test_masked_block_elimination_equals_dense_solve(flags, lg):
    """The masked, aspect-folded elimination against a dense solve of the transformed system (J T, a 1 on the diagonal of every
    fixed parameter), 9-parameter and 12-parameter masks; test_calib_host.test_block_elimination_equals_dense_solve's gate.

    The dampings are -1, 0 and 2.  The gate compares two fp64 solves of one system, and each is only good to the condition number
    of the damped matrix with its diagonal scaled to 1, times 2^-52.  With the damping 1 + 10^lg on a unit diagonal that number is
    at most (1 + 10^lg + n) / 10^lg: under 500 from lg = -1 up (asserted below), so 1e-13 and a tenth of the gate.  At lg = -3 it
    is 4e3 to 8e3 on this scene and on test_calib_host's, 1e-12 to 2e-12: the dense reference is then no better than the gate, and
    the unmasked 12-parameter elimination measures 7e-13 to 5e-12 against it like the masked ones."""
    objs, imgs, _, poses = rational_views(5, 0.3)
    fm = calib._flag_model(flags, K_RATIO, None)
    theta = np.r_[RAT_K[0, 0], RAT_K[1, 1], RAT_K[0, 2], RAT_K[1, 2], RAT_DIST] * 1.02
    if not fm.rational:
        theta[9:] = 0.0
    P = poses + 1e-3
    views = calib._views(objs, imgs)
    N = len(views)
    U, W, V, ga, gb, _ = calib._masked_blocks(views, theta, P, fm.free, fm.aspect)
    dt, dp = calib._schur_step(U, W, V, ga, gb, lg)
    T = _map(fm.free, fm.aspect)
    Js, rs = [], []
    for i, (o, m) in enumerate(views):
        res, _, J = calib._project_full12(o, m, theta, P[i], True)
        Jf = np.zeros((J.shape[0], 12 + 6 * N))
        Jf[:, :12] = J[:, :12] @ T
        Jf[:, 12 + 6 * i:18 + 6 * i] = J[:, 12:]
        Js.append(Jf)
        rs.append(res.ravel())
    J, r = np.concatenate(Js, 0), np.concatenate(rs)
    A = J.T @ J
    fixed = np.flatnonzero(~fm.free)
    A[fixed, fixed] = 1.0
    A[np.diag_indices(A.shape[0])] *= 1.0 + 10.0 ** lg
    x = np.linalg.solve(A, J.T @ r)
    d = 1.0 / np.sqrt(np.diag(A))
    assert np.linalg.cond(A * d[:, None] * d[None, :]) < 500                  # a condition on the input (docstring)
    got = np.r_[dt, dp.ravel()]
    assert np.linalg.norm(got - x) <= 1e-12 * np.linalg.norm(x)
    assert not dt[fixed].any()


@pytest.fixture(scope="module")
def noisy():
    return make_views(62, 20, sigma=0.3)


@pytest.mark.parametrize("flags", ALONE + [TOGETHER], ids=hex)
def test_each_flag_fixes_what_it_says_and_reaches_a_minimum(noisy, flags):
    """sigma = 0.3 px.  Fixed entries come back with the bits they started with, fx = a fy exactly under the aspect tie, and the
    gradient vanishes over the free columns as in test_calib_host.test_optimality_with_noise."""
    objs, imgs, _, _ = noisy
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=flags, camera_matrix=K_RATIO)
    assert r.status == calib.CALIB_OK and r.flags == flags and r.dist_coeffs.shape == (1, 5)
    fm = calib._flag_model(flags, K_RATIO, None)
    views = calib._views(objs, imgs)
    _, start, _ = calib._initialise_flags(views, SIZE, fm)
    th = theta12(r)
    fixed = ~fm.free
    if fm.aspect is not None:
        fixed[0] = False
        a = K_RATIO[0, 0] / K_RATIO[1, 1]
        assert r.camera_matrix[0, 0] == a * r.camera_matrix[1, 1]
        assert abs(start[0] / start[1] - a) <= 1e-15 * a                      # OpenCV's rule on Zhang's K0
    assert np.array_equal(bits(th[fixed]), bits(start[fixed])), (th, start)
    if flags & F.CALIB_ZERO_TANGENT_DIST:
        assert not th[6:8].any()
    assert not th[9:].any()
    # the gradient over the free columns (the fy column carries a times the fx column under the tie) and every pose
    P = np.c_[r.rvecs, r.tvecs]
    T = _map(fm.free, fm.aspect)
    Js, rs = [], []
    for i, (o, m) in enumerate(views):
        res, _, J = calib._project_full12(o, m, th, P[i], True)
        Jf = np.zeros((J.shape[0], 12 + 6 * len(views)))
        Jf[:, :12] = J[:, :12] @ T
        Jf[:, 12 + 6 * i:18 + 6 * i] = J[:, 12:]
        Js.append(Jf)
        rs.append(res.ravel())
    J, res = np.concatenate(Js, 0), np.concatenate(rs)
    assert np.linalg.norm(J.T @ res) <= 1e-9 * np.linalg.norm(J) * np.linalg.norm(res)
    assert 0.2 < r.rms < 0.6 and r.attempts >= r.iterations >= 1


def test_guess_from_the_truth():
    """Noise-free float32 views from the true model: done within a few steps, at the float32 floor of
    test_calib_host.test_truth_recovery_float32."""
    objs, imgs, _, _ = make_views(63, 12)
    plain = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=F.CALIB_USE_INTRINSIC_GUESS, camera_matrix=K_TRUE, dist_coeffs=DIST_TRUE)
    print("guess from the truth: steps", r.iterations, "attempts", r.attempts, "rms", r.rms, "; without the guess", plain.iterations)
    assert r.status == calib.CALIB_OK and r.views_used == 12 and r.dist_coeffs.shape == (1, 5)
    # (the stop rule asks for |dp| < 2^-52 |p|: from the truth too the last steps are spent at the rounding level, most rejected)
    assert r.rms <= 2e-5 and r.iterations <= 10 and r.iterations <= plain.iterations
    assert np.abs(r.camera_matrix - K_TRUE).max() <= 1e-5 * 400 and np.abs(r.dist_coeffs.ravel() - DIST_TRUE).max() <= 1e-5
    # an 8-coefficient guess without RATIONAL_MODEL: 1x8 out, k4 k5 k6 held at the bits given
    d8 = np.r_[DIST_TRUE, 1e-3, -2e-3, 5e-4]
    r8 = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=F.CALIB_USE_INTRINSIC_GUESS, camera_matrix=K_TRUE, dist_coeffs=d8)
    assert r8.status == calib.CALIB_OK and r8.dist_coeffs.shape == (1, 8)
    assert np.array_equal(bits(r8.dist_coeffs.ravel()[5:]), bits(d8[5:]))


@pytest.mark.parametrize("n_views,sigma", [(24, 0.0), (64, 0.3)])
def test_guess_from_a_wrong_camera_reaches_the_same_minimum(n_views, sigma):
    """A K that is 5 % off: the minimum of the call without a guess, to test_gpu_calib.py's REL_K / ABS_DIST, on noise-free views
    and on that file's noisy size, 64 views at sigma = 0.3.  (With fewer noisy views k3 sits in a flat valley, 0.28 or 0.46 for a
    truth of -0.02, and two starts stop 3e-8 apart along it with rms values 3e-16 apart: 24 and 30 views measured so.)"""
    objs, imgs, _, _ = make_views(64, n_views, sigma=sigma)
    plain = calib.calibrate_camera_host_full(objs, imgs, SIZE)
    K = K_TRUE.copy()
    K[:2] *= 1.05
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=F.CALIB_USE_INTRINSIC_GUESS, camera_matrix=K, dist_coeffs=DIST_TRUE)
    gap_k = np.abs(r.camera_matrix - plain.camera_matrix).max() / plain.camera_matrix[0, 0]
    gap_d = np.abs(r.dist_coeffs - plain.dist_coeffs).max()
    print("guess 5 % off: K gap", gap_k, "dist gap", gap_d, "steps", r.iterations, plain.iterations)
    assert r.status == plain.status == calib.CALIB_OK
    assert gap_k <= 1e-8 and gap_d <= 1e-8
    assert abs(r.rms - plain.rms) <= 1e-9 * plain.rms + 1e-12


def test_guess_with_every_intrinsic_fixed_refines_the_poses_alone():
    objs, imgs, _, _ = make_views(65, 6, sigma=0.3)
    every = (F.CALIB_USE_INTRINSIC_GUESS | F.CALIB_FIX_FOCAL_LENGTH | F.CALIB_FIX_PRINCIPAL_POINT | F.CALIB_FIX_K1 | F.CALIB_FIX_K2
             | F.CALIB_FIX_K3)
    dist = np.r_[DIST_TRUE[:2], 0.0, 0.0, DIST_TRUE[4]]
    K = K_TRUE.copy()
    K[0, 0] *= 1.01
    fixed_tangent = every | F.CALIB_ZERO_TANGENT_DIST
    for flags, d in ((fixed_tangent, DIST_TRUE), (fixed_tangent | F.CALIB_FIX_ASPECT_RATIO, DIST_TRUE)):
        r = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=flags, camera_matrix=K, dist_coeffs=d)
        assert r.status == calib.CALIB_OK
        assert np.array_equal(bits(theta12(r)[:9]), bits(np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], dist]))
        fm = calib._flag_model(flags, K, d)
        assert not fm.free.any() and fm.aspect is None
        views = calib._views(objs, imgs)
        _, _, P0 = calib._initialise_flags(views, SIZE, fm)
        P = np.c_[r.rvecs, r.tvecs]
        assert not np.array_equal(P, P0) and np.abs(P - P0).max() <= 1e-3          # they move, from pnp's own minimum
        # N independent pose refinements: a view alone gives the same pose
        one = calib.calibrate_camera_host_full(objs[2:3], imgs[2:3], SIZE, flags=flags, camera_matrix=K, dist_coeffs=d)
        assert np.abs(np.r_[one.rvecs[0], one.tvecs[0]] - P[2]).max() <= 1e-8


@pytest.fixture(scope="module")
def rational_clean():
    objs, imgs, ids_l, poses = rational_views(16, 0.0)
    return objs, imgs, poses, calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, flags=F.CALIB_RATIONAL_MODEL)


def test_rational_scene_noise_free(rational_clean):
    """16 noise-free views: CALIB_OK at the float32 rounding of the image points (measured 1.00e-5 px; the gate is twice that),
    which the 9-parameter model misses by three orders of magnitude on the same pixels."""
    objs, imgs, poses, r = rational_clean
    print("rational, noise-free: rms", r.rms, "steps", r.iterations, "attempts", r.attempts, "dist", r.dist_coeffs.ravel())
    assert r.status == calib.CALIB_OK and r.views_used == 16 and r.dist_coeffs.shape == (1, 8) and r.flags == F.CALIB_RATIONAL_MODEL
    assert r.rms <= 2e-5
    assert r.attempts > r.iterations                                   # the scene rejects steps: the GPU tests rely on it
    truth = np.concatenate([cx.f64(cx.project(o, p, RAT_K, RAT_DIST)) for o, p in zip(objs, poses)], 0)
    assert np.abs(positions(r, objs, imgs) - truth).max() <= 1e-4      # by position: the float32 rounding is 3e-5 px a coordinate
    plain = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE)
    assert plain.rms > 100 * r.rms


def test_rational_scene_with_noise():
    """sigma = 0.3 px: the coefficients wander, the projection does not: the rms is not above the 9-parameter model's."""
    objs, imgs, _, _ = rational_views(16, 0.3)
    r = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE, flags=F.CALIB_RATIONAL_MODEL)
    plain = calib.calibrate_camera_host_full(objs, imgs, RAT_SIZE)
    print("rational, sigma 0.3: rms", r.rms, "default", plain.rms, "steps", r.iterations, "dist", r.dist_coeffs.ravel())
    assert r.status == plain.status == calib.CALIB_OK
    assert r.rms <= plain.rms
    assert np.abs(positions(r, objs, imgs) - positions(plain, objs, imgs)).max() <= 1.0     # px: two fits of the same noisy pixels


def test_rational_fix_k_flags_hold_their_start(rational_clean):
    objs, imgs, _, _ = rational_clean
    d8 = RAT_DIST.copy()
    flags = F.CALIB_RATIONAL_MODEL | F.CALIB_USE_INTRINSIC_GUESS | F.CALIB_FIX_K4 | F.CALIB_FIX_K6 | F.CALIB_FIX_K2
    r = calib.calibrate_camera_host_full(objs[:8], imgs[:8], RAT_SIZE, flags=flags, camera_matrix=RAT_K, dist_coeffs=d8)
    assert r.status == calib.CALIB_OK and r.rms <= 2e-5
    got = r.dist_coeffs.ravel()
    assert np.array_equal(bits(got[[1, 5, 7]]), bits(d8[[1, 5, 7]])) and got[6] != d8[6]


def test_refused_arguments():
    objs, imgs, _, _ = make_views(66, 4)
    call = lambda **kw: calib.calibrate_camera_host_full(objs, imgs, SIZE, **kw)
    for bad in (0x100, 0x200, 0x400, 0x8000, 0x10000, 0x40000, 0x80000, 0x100000, 0x20000, 1 << 30, -1):
        # FIX_K? beyond k6 do not exist; USE_QR, FIX_TANGENT_DIST, thin prism, FIX_S1_S2_S3_S4, tilted, FIX_TAUX_TAUY, USE_LU
        with pytest.raises(ValueError, match="not supported"):
            call(flags=bad)
        with pytest.raises(ValueError):
            call(flags=bad | F.CALIB_FIX_K3)
    for flags in (F.CALIB_FIX_ASPECT_RATIO, F.CALIB_USE_INTRINSIC_GUESS, F.CALIB_USE_INTRINSIC_GUESS | F.CALIB_FIX_K1):
        with pytest.raises(ValueError, match="camera_matrix"):
            call(flags=flags)
    G = F.CALIB_USE_INTRINSIC_GUESS
    for n in (1, 2, 3, 6, 7, 12, 14):
        with pytest.raises(ValueError):
            call(flags=G, camera_matrix=K_TRUE, dist_coeffs=np.zeros(n))
    with pytest.raises(ValueError):
        call(flags=G, camera_matrix=K_TRUE, dist_coeffs=[0.1, np.nan, 0, 0, 0])
    with pytest.raises(ValueError):
        call(flags=G, camera_matrix=K_TRUE, dist_coeffs=[0.1, np.inf, 0, 0])
    for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
        K = K_TRUE.copy()
        K[i, j] = np.nan
        with pytest.raises(ValueError):
            call(flags=G, camera_matrix=K)
    with pytest.raises(ValueError):
        call(flags=G, camera_matrix=np.eye(4))
    with pytest.raises(ValueError, match="USE_INTRINSIC_GUESS"):
        call(flags=F.CALIB_FIX_K3, dist_coeffs=DIST_TRUE)                 # coefficients without the guess flag
    with pytest.raises(ValueError):
        call(flags=1.5)
    with pytest.raises(ValueError):
        calib.calibrate_camera_host(objs, imgs, SIZE, flags=0x100)
    # the device entries check before they touch a device
    kps = [np.c_[m.astype(np.float64), np.arange(len(m))] for m in imgs]
    with pytest.raises(ValueError, match="not supported"):
        calib.calibrate_charuco_device(kps, *BOARD, SIZE, flags=0x100)
    with pytest.raises(ValueError, match="camera_matrix"):
        calib.calibrate_charuco_pool(None, 4, 64, True, *BOARD, SIZE, flags=F.CALIB_FIX_ASPECT_RATIO)


def test_uncertainty_refuses_a_flagged_result():
    objs, imgs, _, _ = make_views(67, 6, sigma=0.3)
    r = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=F.CALIB_FIX_K3)
    assert r.status == calib.CALIB_OK
    with pytest.raises(ValueError, match="held fixed"):
        calib.calibration_uncertainty_host(objs, imgs, r)
    rr = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=F.CALIB_RATIONAL_MODEL)
    with pytest.raises(ValueError):
        calib.calibration_uncertainty_host(objs, imgs, rr)
    # a guess alone frees the default nine
    g = calib.calibrate_camera_host_full(objs, imgs, SIZE, flags=F.CALIB_USE_INTRINSIC_GUESS, camera_matrix=K_TRUE, dist_coeffs=DIST_TRUE)
    assert calib.calibration_uncertainty_host(objs, imgs, g).status == calib.COV_OK


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    R = F.CALIB_RATIONAL_MODEL
    assert lib.dcx_calibrate_flags_workspace_bytes(0, 0) == 0 and lib.dcx_calibrate_flags_workspace_bytes(4, 0x100) == 0
    ws9, ws12 = lib.dcx_calibrate_flags_workspace_bytes(4, F.CALIB_FIX_K3), lib.dcx_calibrate_flags_workspace_bytes(4, R)
    assert ws12 > ws9 > lib.dcx_calibrate_workspace_bytes(4)
    assert lib.dcx_calibrate_flags_workspace_bytes(128, R) > lib.dcx_calibrate_flags_workspace_bytes(64, R) > ws12
    assert calib.flags_workspace_bytes(4, R) == ws12
    res = (ctypes.c_double * 20)()
    cam = (ctypes.c_double * 9)(400, 0, 160, 0, 410, 120, 0, 0, 1)
    d5, d8 = (ctypes.c_double * 5)(-0.2, 0.1, 0, 0, 0), (ctypes.c_double * 8)(-0.2, 0.1, 0, 0, 0, 0.1, 0, 0)
    p = 4096              # a non-null address that is never read: every call below fails a check before any device access
    G, A = F.CALIB_USE_INTRINSIC_GUESS, F.CALIB_FIX_ASPECT_RATIO
    args = [p, p, p, p, 4, 16, 8, 8, 0.02, 320, 240, G, cam, d5, 5, p, ws9 - 1, p, p, res, None]
    assert lib.dcx_calibrate_flags_pool(*args) == -3                       # everything right but a workspace one byte short
    for i in (0, 1, 2, 12, 13, 15, 17, 18, 19):       # null counts, starts, rows, camera, dist (n_dist 5), workspace, status, pose, h_result
        a = list(args)
        a[i] = None
        assert lib.dcx_calibrate_flags_pool(*a) == -1, i
    nan, inf = float("nan"), float("inf")
    for i, v in ((4, 0), (5, -1), (6, 1), (7, 1), (8, nan), (9, 0), (10, 0), (11, G | 0x100), (11, G | 0x40000), (11, -1), (14, 3), (14, 12),
                 (11, F.CALIB_FIX_K3),                                     # coefficients without the guess
                 (12, (ctypes.c_double * 9)(400, 0, 160, 0, nan, 120, 0, 0, 1)), (12, (ctypes.c_double * 9)(400, 1, 160, 0, 410, 120, 0, 0, 1)),
                 (13, (ctypes.c_double * 5)(0, inf, 0, 0, 0))):
        a = list(args)
        a[i] = v
        assert lib.dcx_calibrate_flags_pool(*a) == -1, (i, v)
    for flags in (A, G, A | F.CALIB_FIX_K1):                               # both flags need the camera
        assert lib.dcx_calibrate_flags_pool(*args[:11], flags, None, None, 0, *args[15:]) == -1
    assert lib.dcx_calibrate_flags_pool(*args[:11], A, (ctypes.c_double * 9)(-400, 0, 160, 0, 410, 120, 0, 0, 1), None, 0, *args[15:]) == -1
    # the workspace is checked against the model that runs: 12 parameters with the flag or with live k4 k5 k6 in the guess
    tail = lambda n: [p, n, p, p, res, None]
    assert lib.dcx_calibrate_flags_pool(*args[:11], R, None, None, 0, *tail(ws12 - 1)) == -3
    assert lib.dcx_calibrate_flags_pool(*args[:11], G, cam, d8, 8, *tail(ws12 - 1)) == -3
    assert lib.dcx_calibrate_flags_pool(*args[:11], F.CALIB_ZERO_TANGENT_DIST, None, None, 0, *tail(ws9 - 1)) == -3
