"""An exact restatement of the camera model the pose and calibration solvers minimise, and the scenario grid their edge tests share.

Written from the documented pinhole + distortion model (OpenCV's calib3d documentation, which is what the reference's
cv2.solvePnP / cv2.calibrateCamera use), not from deepcharuco_amd/pnp.py: nothing here imports pnp's _project, _rodrigues,
_right_jacobian or _undistort, no threshold of pnp.py is restated, and no analytic Jacobian exists here at all.

    R = exp([r]x);  (X, Y, Z) = R m + t;  x = X / Z, y = Y / Z;  r2 = x^2 + y^2
    g = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
    x' = x g + 2 p1 x y + p2 (r2 + 2 x^2);  y' = y g + p1 (r2 + 2 y^2) + 2 p2 x y
    u = fx x' + cx, v = fy y' + cy;  coefficients in the order k1 k2 p1 p2 k3 k4 k5 k6

Arithmetic: numpy.longdouble where it has a 64-bit mantissa (x86: eps 1.08e-19), else mpmath numbers in object arrays (slow but
the same code).  ``project_mp`` is a third statement in 40-digit mpmath with the rotation as a true matrix exponential
(mpmath.expm); tests/test_pose_exact_host.py pins the array version to it on a handful of points.

The rotation's closed form I + a [r]x + b [r]x^2, a = sin(th)/th, b = (1 - cos th)/th^2, is evaluated without cancellation for
every th > 0 (b = 2 sin^2(th/2) / th^2), so no series and no threshold is needed; th = 0 exactly takes the limits a = 1, b = 1/2.
"""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps < 1e-18)

if HAVE_LD:
    def _w(a):
        return np.asarray(a, dtype=LD)
    _sqrt, _sin, _cos = np.sqrt, np.sin, np.cos
else:                                                      # pragma: no cover  (no 80-bit long double on this platform)
    import mpmath
    mpmath.mp.dps = 40
    _to_mp = np.vectorize(lambda v: v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v)), otypes=[object])

    def _w(a):
        return _to_mp(np.asarray(a))
    _sqrt, _sin, _cos = mpmath.sqrt, mpmath.sin, mpmath.cos


def f64(a):
    return np.asarray(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the model

def board_points(ids, col_count, row_count, square_len):
    """The reference's table of inner corners (its solve_pnp: the row index runs fastest and is the x coordinate, the column
    index is y, both from 1, times square_len in float64, stored as float32, z = 0), looked up by id -> float32 (N, 3)."""
    table = np.zeros(((col_count - 1) * (row_count - 1), 3), np.float32)
    i = 0
    for c in range(1, col_count):
        for r in range(1, row_count):
            table[i, 0] = r * float(square_len)
            table[i, 1] = c * float(square_len)
            i += 1
    return table[np.asarray(ids).astype(int)]


def grid_xy(ids, row_count):
    """Integer grid position of each id on the board, by the same table."""
    ids = np.asarray(ids).astype(int)
    return np.stack([ids % (row_count - 1), ids // (row_count - 1)], 1)


def dist8(dist):
    k = np.zeros(8)
    if dist is not None:
        d = np.asarray(dist, np.float64).ravel()
        k[:d.size] = d
    return k


def rotation(r):
    """exp([r]x), 3x3 in the working precision."""
    r = _w(r)
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    S = np.array([[0 * r[0], -r[2], r[1]], [r[2], 0 * r[0], -r[0]], [-r[1], r[0], 0 * r[0]]], dtype=r.dtype)
    eye = _w(np.eye(3))
    if th2 == 0:
        return eye + S
    th = _sqrt(th2)
    h = _sin(th / 2)
    S2 = np.array([[sum(S[i, k] * S[k, j] for k in range(3)) for j in range(3)] for i in range(3)], dtype=r.dtype)
    return eye + (_sin(th) / th) * S + (2 * h * h / th2) * S2


def distort(x, y, K, k):
    """Normalised coordinates -> pixels through the full model (working precision arrays)."""
    K, k = _w(K), _w(k)
    r2 = x * x + y * y
    g = (1 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2) / (1 + k[5] * r2 + k[6] * r2 * r2 + k[7] * r2 * r2 * r2)
    xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1)


def camera_points(obj, P, X=None):
    """Board points (N, 3) through the pose P = (rvec, tvec) and, with X, on through a second transform X (a rig's: P is then the
    board's pose in camera 0's frame and X takes that frame to the camera's) -> [X, Y, Z], working precision.  The one statement
    of this step: every projection of the *_exact modules, of either camera model, goes through it."""
    obj, P = _w(obj), _w(P)
    R = rotation(P[:3])
    Q = [R[i, 0] * obj[:, 0] + R[i, 1] * obj[:, 1] + R[i, 2] * obj[:, 2] + P[3 + i] for i in range(3)]
    if X is not None:
        X = _w(X)
        Rx = rotation(X[:3])
        Q = [Rx[i, 0] * Q[0] + Rx[i, 1] * Q[1] + Rx[i, 2] * Q[2] + X[3 + i] for i in range(3)]
    return Q


def project(obj, p, K, dist, X=None):
    """Board points (N, 3), pose p = (rvec, tvec) -> pixels (N, 2) in the working precision; every Z must be positive."""
    Q = camera_points(obj, p, X)
    assert all(z > 0 for z in Q[2]), "a point is not in front of the camera"
    return distort(Q[0] / Q[2], Q[1] / Q[2], K, dist8(dist))


def residuals(obj, img, p, K, dist):
    """projected - observed, (N, 2), working precision."""
    return project(obj, p, K, dist) - _w(img)


def cost(obj, img, p, K, dist):
    r = residuals(obj, img, p, K, dist)
    return float((r * r).sum())


def fd_step(v, j):
    """The central-difference step of entry j of a pose block v = (rvec, tvec): 1e-6 rad, 1e-6 |t|."""
    return _w(1e-6) * (1 if j < 3 else _sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5]))


def jacobian_of(f, *blocks):
    """Jacobian of the residuals f(*blocks) with respect to every entry of every pose block ([n, 6] or [6]), block by block and
    row-major within one, by central differences in the working precision -> float64 [2M, entries].  Steps ``fd_step``:
    truncation ~1e-12 and rounding ~1e-13 of a column's size with a 64-bit mantissa.  The one finite-difference routine of the
    pose costs; fisheye_exact.jacobian_fd, which also differentiates by the intrinsics, has its own scales."""
    blocks = [_w(b) for b in blocks]
    cols = []
    for k, b in enumerate(blocks):
        for idx in np.ndindex(b.shape):
            h = fd_step(b[idx[:-1]], idx[-1])
            d = _w(np.zeros(b.shape))
            d[idx] = h
            hi, lo = f(*blocks[:k], b + d, *blocks[k + 1:]), f(*blocks[:k], b - d, *blocks[k + 1:])
            cols.append(f64(((hi - lo) / (2 * h)).ravel()))
    return np.stack(cols, 1)


def stationarity_of(r, J):
    """Working-precision residuals r and their Jacobian J -> (cost, |J^T r| / (|J| |r|)); 0 for the gradient where r = 0."""
    r = f64(r).ravel()
    nr = np.linalg.norm(r)
    return float(r @ r), (float(np.linalg.norm(J.T @ r) / (np.linalg.norm(J) * nr)) if nr > 0 else 0.0)


def jacobian_fd(obj, img, p, K, dist):
    """2N x 6 Jacobian of the residuals with respect to the pose (``jacobian_of``) -> float64."""
    return jacobian_of(lambda q: residuals(obj, img, q, K, dist), p)


def stationarity(obj, img, p, K, dist):
    """-> (cost, |J^T r| / (|J| |r|)) at pose p, both from this module's residuals and finite differences."""
    return stationarity_of(residuals(obj, img, p, K, dist), jacobian_fd(obj, img, p, K, dist))


def undistort5(pix, K, dist, rounds=5):
    """This module's own inverse of ``distort``: the documented fixed-point iteration x <- (x0 - tangential(x)) / radial(x),
    ``rounds`` times from x = x0 -> normalised coordinates (N, 2), working precision."""
    K, k, pix = _w(K), _w(dist8(dist)), _w(pix)
    x0, y0 = (pix[:, 0] - K[0, 2]) / K[0, 0], (pix[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    for _ in range(rounds):
        r2 = x * x + y * y
        g = (1 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2) / (1 + k[5] * r2 + k[6] * r2 * r2 + k[7] * r2 * r2 * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        x, y = (x0 - dx) / g, (y0 - dy) / g
    return np.stack([x, y], 1)


def project_mp(m, p, K, dist):
    """One board point through the model in 40-digit mpmath, the rotation by mpmath.expm of the skew matrix -> (u, v) mpf."""
    import mpmath
    with mpmath.workdps(40):
        f = mpmath.mpf
        r = [f(float(v)) for v in p[:3]]
        R = mpmath.expm(mpmath.matrix([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]))
        X = [R[i, 0] * f(float(m[0])) + R[i, 1] * f(float(m[1])) + R[i, 2] * f(float(m[2])) + f(float(p[3 + i])) for i in range(3)]
        x, y = X[0] / X[2], X[1] / X[2]
        k = [f(float(v)) for v in dist8(dist)]
        r2 = x * x + y * y
        g = (1 + k[0] * r2 + k[1] * r2 ** 2 + k[4] * r2 ** 3) / (1 + k[5] * r2 + k[6] * r2 ** 2 + k[7] * r2 ** 3)
        xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        return f(float(K[0][0])) * xd + f(float(K[0][2])), f(float(K[1][1])) * yd + f(float(K[1][2]))


def to_mp(v):
    """A working-precision scalar -> mpf, exactly (a long double is the sum of two doubles)."""
    import mpmath
    if not HAVE_LD:
        return v
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - LD(hi)))


# ------------------------------------------------------------------------------------------------ the scenario grid

BOARDS = [(9, 6, 0.02), (6, 9, 0.02), (4, 13, 0.015), (24, 17, 0.004)]           # (col_count, row_count, square_len); 40, 40, 36, 368 ids
K_EDGE = np.array([[310.0, 0, 157.3], [0, 287.0, 123.9], [0, 0, 1]])           # fx / fy = 1.08, principal point off-centre
DIST8 = np.array([-0.2, 0.05, 1e-3, -1e-3, 0.01, 0.02, -0.01, 0.005])
MODELS = {"none": None, "4": DIST8[:4], "5": DIST8[:5], "8": DIST8}
VIEWS = ("fronto", "tiny", "tilt", "pi", "near_pi")
ROWS = (4, 5, 63, 64, 65, 129)                                                   # capped by the board's id count
SIGMAS = (0.0, 0.3)
# rotation axes of the "pi" and "near_pi" views: the optical axis, and axes some 15 degrees off it with every sign pattern of
# their x and y components
PI_AXES = [(0.0, 0.0, 1.0), (0.1, 0.25, 0.96), (0.3, -0.1, 0.95), (-0.2, -0.25, 0.95), (0.25, 0.1, 0.96), (-0.15, 0.2, 0.97)]

Frame = namedtuple("Frame", "kp r t board model view n sigma tag")


def n_ids(board):
    return (board[0] - 1) * (board[1] - 1)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def view_rvec(rng, view, k=0):
    """The true rotation vector of a view class (float64).  "tiny" stays below 1e-6 and "pi" within 1e-7 of pi, so that the
    sine of the rotation angle is at least a factor 10 below the 1e-5 at which a matrix -> vector conversion in the style of
    cvRodrigues2 switches arms; "near_pi" (0.001 - 0.05 rad short of pi) and "tilt" are as far above it."""
    if view == "fronto":
        return np.zeros(3)
    if view == "tiny":
        return _unit(rng.normal(size=3)) * rng.uniform(1e-7, 4e-7)
    if view == "tilt":
        return _unit(rng.normal(size=3)) * np.deg2rad(rng.uniform(5, 50))
    if view == "pi":
        return _unit(PI_AXES[k % len(PI_AXES)]) * (np.pi - rng.uniform(0, 1e-7))
    if view == "near_pi":
        return _unit(PI_AXES[k % len(PI_AXES)]) * (np.pi - rng.uniform(0.001, 0.05))
    raise ValueError(view)


def place(rng, r, board, K):
    """tvec that puts the board's centre near the optical axis at the distance from which its longer side spans about +-100 px."""
    allp = board_points(np.arange(n_ids(board)), *board).astype(np.float64)
    centre = allp.mean(0)
    half = np.abs(allp - centre).max()
    tz = 0.5 * (K[0, 0] + K[1, 1]) * half / 100.0 * rng.uniform(0.9, 1.2)
    return np.array([rng.uniform(-0.03, 0.03) * tz, rng.uniform(-0.03, 0.03) * tz, tz]) - f64(rotation(r)) @ centre


MIN_HEIGHT_PX = 10.0


def general_position(ids, board):
    """What a minimal planar solver needs of a frame of 4 or 5 rows: no id twice and no three ids on, or close to, one line of the
    board grid.  Close: the triangle's height over its longest side, at the +-100 px scale of this grid, is below
    MIN_HEIGHT_PX.  Exactly collinear triples are DEGENERATE by specification.  Nearly collinear ones are dropped here by
    name: the initial pose is the homography through the points, which image noise sigma tilts by about sigma / height rad, and
    a planar target has a second, mirrored local minimum a few tenths of a radian away.  On a CPU run of this grid with the
    exact-collinearity rule alone, the host definition ended in that mirrored minimum on two 4-row sigma = 0.3 px frames whose
    flattest triangle was 0.6 px and 1.8 px high (a true stationary point: gradient 4e-9 by this module's measure, cost 2 - 8
    times the cost at the truth).  A local minimiser started from a homography is not specified to pick the global minimum
    there; 10 px keeps the tilt of the start under 0.03 rad."""
    g = grid_xy(ids, board[1]).astype(np.float64)
    n = len(g)
    if len({tuple(v) for v in g}) < n:
        return False
    px = 200.0 / max(board[0] - 2, board[1] - 2)                  # pixels per grid step when the longer side spans 200 px
    for a in range(n):
        for b in range(a + 1, n):
            for c in range(b + 1, n):
                area2 = abs((g[b, 0] - g[a, 0]) * (g[c, 1] - g[a, 1]) - (g[b, 1] - g[a, 1]) * (g[c, 0] - g[a, 0]))
                longest = max(np.hypot(*(g[b] - g[a])), np.hypot(*(g[c] - g[a])), np.hypot(*(g[c] - g[b])))
                if area2 / longest * px < MIN_HEIGHT_PX:
                    return False
    return True


def draw_ids(rng, board, n):
    """n ids (capped by the board's) without replacement in scrambled order; frames of 4 or 5 rows in general position."""
    n = min(n, n_ids(board))
    while True:
        ids = rng.choice(n_ids(board), n, replace=False)
        if n > 5 or general_position(ids, board):
            return ids


def make_frame(rng, board, dist, view, n, sigma, k=0, K=K_EDGE, tag=""):
    """A frame of the grid: image points by ``project``, plus noise, rounded to float32 as the corner pool holds them."""
    ids = draw_ids(rng, board, n)
    r = view_rvec(rng, view, k)
    t = place(rng, r, board, K)
    img = f64(project(board_points(ids, *board), np.r_[r, t], K, dist))
    if sigma:
        img = img + rng.normal(scale=sigma, size=img.shape)
    kp = np.c_[img.astype(np.float32).astype(np.float64), ids]
    return Frame(kp, r, t, board, None, view, len(ids), sigma, tag)


# Frames that take a later draw of their own stream (frame index -> draw).  Their first draw left the rotation of the
# solver's initial pose with a sine within a factor 10 of 1e-5, where the matrix -> vector conversion switches arms: host and
# device must not be asked to agree on a coin toss.  Measured on the CPU by tests/test_pose_exact_host.py::branch_margin, which
# asserts the margin for the whole grid.  (A noise-free 4-row frame turns float32 rounding into ~1e-6 rad; the roll of a
# noisy view rolled by 180 degrees is a draw from N(0, ~5e-4 rad).)
# One entry has another reason, #37 (9x6, 4 coefficients, tiny, 4 rows, sigma 0.3): its first draw has two local minima (a
# planar target seen square-on mirrors its tilt), and the host definition ends in the higher one: a stationary point by this
# module's measure, cost 0.619 px^2 against 0.398 px^2 at the truth.  A local minimiser is not specified to find the other.
REDRAW = {0: 1, 27: 1, 36: 1, 37: 1, 60: 1, 62: 1, 122: 1, 126: 1, 158: 1, 186: 3, 210: 2, 240: 3, 248: 1, 270: 8, 276: 13, 300: 1,
          306: 2, 330: 4, 332: 2, 336: 1, 360: 1, 420: 2, 467: 1, 480: 1, 492: 1, 525: 1, 540: 2, 542: 1, 587: 2}


def _specs():
    out = []
    for board in BOARDS:
        for model in MODELS:
            k = 0
            for view in VIEWS:
                for n in sorted({min(n, n_ids(board)) for n in ROWS}):       # counts that the cap makes equal are taken once
                    for sigma in SIGMAS:
                        out.append((board, model, view, n, sigma, k))
                        k += 1
    return out


def grid_frame(i, draw=0):
    """Frame i of the grid from draw ``draw`` of its own seeded stream."""
    board, model, view, n, sigma, k = _specs()[i]
    tag = f"#{i} {board[0]}x{board[1]} dist {model} {view} n={min(n, n_ids(board))} sigma={sigma}"
    rng = np.random.default_rng([7000, i, draw])
    return make_frame(rng, board, MODELS[model], view, n, sigma, k, tag=tag)._replace(model=model)


@functools.lru_cache(maxsize=None)
def grid():
    """Every board x distortion model x view class x row count x noise level: 4 models * 5 view classes * 2 noise levels *
    (3 boards * 3 row counts [4, 5, all ids] + the big board * 6 row counts) = 600 frames."""
    return [grid_frame(i, REDRAW.get(i, 0)) for i in range(len(_specs()))]


def pool_rows(f):
    """The frame as a corner pool holds it (id-sorted, stable) -> (board points float32, image points float64, kp sorted)."""
    kp = f.kp[np.argsort(f.kp[:, 2], kind="stable")]
    return board_points(kp[:, 2], *f.board), kp[:, :2], kp


def rot_gap(ra, rb):
    """max |R(ra) - R(rb)|: the distance of two rotation vectors as rotations (near pi, r and r (1 - 2 pi / |r|) are the same
    rotation and far apart as vectors)."""
    return float(np.abs(f64(rotation(ra)) - f64(rotation(rb))).max())


# ------------------------------------------------------------------------------------------------ RANSAC frames

RANSAC_REPROJ, RANSAC_SEED = 3.0, 7


@functools.lru_cache(maxsize=None)
def planted_frames():
    """sigma = 0.3 px views with wrong ids planted (another id of the board, at least two grid steps from the true one: ~25 px
    at this scale against a 3 px threshold) -> list of (Frame, good-row mask).  The big board at 63 / 64 / 65 / 129 rows under
    every distortion model, and 30 rows of each smaller board, tilted, fronto-parallel and rolled by 180 degrees in turn."""
    out = []
    rng = np.random.default_rng(8100)
    cases = [(BOARDS[3], m, n) for m in MODELS for n in (63, 64, 65, 129)] + [(b, m, 30) for b in BOARDS[:3] for m in MODELS]
    for i, (board, model, n) in enumerate(cases):
        view = ("tilt", "fronto", "pi", "near_pi")[i % 4]
        f = make_frame(rng, board, MODELS[model], view, n, 0.3, k=i, tag=f"planted {board[0]}x{board[1]} dist {model} {view} n={n}")
        kp = f.kp.copy()
        bad = rng.choice(n, max(2, n // 8), replace=False)
        g = grid_xy(kp[:, 2], board[1])
        for j in bad:
            while True:
                new = int(rng.integers(0, n_ids(board)))
                if np.abs(grid_xy([new], board[1])[0] - g[j]).max() >= 2:
                    break
            kp[j, 2] = new
        good = np.ones(n, bool)
        good[bad] = False
        out.append((f._replace(kp=kp, model=model), good))
    return out


# ------------------------------------------------------------------------------------------------ calibration views

CALIB_BOARD = (7, 11, 0.016)                    # 6 x 10 = 60 ids, 0.16 m x 0.096 m of corners
CALIB_SIZE = (400, 240)                         # not 4:3
CALIB_K = np.array([[352.0, 0, 203.1], [0, 371.0, 116.2], [0, 0, 1]])
CALIB_DIST = np.array([-0.25, 0.1, 1e-3, -5e-4, -0.02])


def calib_views(seed, n_views, sigma=0.0, board=CALIB_BOARD, K=CALIB_K, dist=CALIB_DIST, tz=(0.2, 0.3)):
    """-> (board points [float32], image points [float32], ids, true poses [n, 6]).  Every fourth view is fronto-parallel or
    rolled by 180 degrees about the optical axis in turn (a quarter of the set: the focal length cannot be observed from such
    views alone), the others are tilted 5 - 60 degrees; the board's centre is near the optical axis at tz[0] - tz[1] m."""
    rng = np.random.default_rng(seed)
    N = n_ids(board)
    centre = board_points(np.arange(N), *board).astype(np.float64).mean(0)
    objs, imgs, ids_l, poses = [], [], [], []
    for i in range(n_views):
        if i % 4 == 0:
            ids = np.arange(N)
            r = np.zeros(3) if i % 8 == 0 else np.array([0.0, 0.0, 1.0]) * (np.pi - rng.uniform(0, 1e-7))
        else:
            while True:
                ids = np.sort(rng.choice(N, int(rng.integers(6, N + 1)), replace=False))
                g = grid_xy(ids, board[1]).astype(np.float64)
                if np.linalg.matrix_rank(g - g.mean(0)) == 2:
                    break
            r = _unit(rng.normal(size=3)) * np.deg2rad(rng.uniform(5, 60))
        t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(*tz)]) - f64(rotation(r)) @ centre
        obj = board_points(ids, *board)
        img = f64(project(obj, np.r_[r, t], K, dist))
        if sigma:
            img = img + rng.normal(scale=sigma, size=img.shape)
        objs.append(obj)
        imgs.append(img.astype(np.float32))
        ids_l.append(ids)
        poses.append(np.r_[r, t])
    return objs, imgs, ids_l, np.array(poses)
